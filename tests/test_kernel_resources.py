"""CPU (cross-compile only): register budget of the step's dominant kernel.

All 4096 LiDAR waves of the headline batch are resident at once only if `k23_lidar_nav` stays
within 128 VGPRs (4 waves per SIMD) -- and spilled VGPRs cost real HBM traffic and latency (17
spilled registers were worth 4.6 % of the step, docs/HISTORY.md section 4).  This compiles the kernel for
gfx950 and reads the resource usage the compiler reports."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_side_by_side_kernel_fits_its_register_budget():
    src = os.path.join(ROOT, "gym_auv_amd", "csrc", "k_step_fused.hip")
    tmp = tempfile.mkdtemp(prefix="auv_res_")
    try:
        subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-c", src,
                        "-o", os.path.join(tmp, "k.o"), "-save-temps"], cwd=tmp, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        asm = [f for f in os.listdir(tmp) if f.endswith("gfx950.s")]
        assert asm, os.listdir(tmp)
        text = open(os.path.join(tmp, asm[0])).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    # metadata blocks: the keys precede/follow .name inside one YAML map
    blocks = re.split(r"\n\s+- \.agpr_count:", text)

    def usage(name):
        blk = [b for b in blocks if re.search(r"\.name:\s+\S*%s" % name, b)]
        assert len(blk) >= 1, name
        return [(int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1)), int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)),
                 int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", b).group(1))) for b in blk]

    # (k_step_roles: the one-launch step -- dynamics, LiDAR, navigation search and finish roles share its allocation)
    for vgpr, spill, lds_static in usage("k_step_roles") + usage("k23_lidar_nav"):
        assert vgpr <= 128, "LiDAR kernel needs %d VGPRs: fewer than 4 waves per SIMD" % vgpr
        assert spill <= 4, "LiDAR kernel spills %d VGPRs to scratch" % spill
        assert lds_static == 0          # the per-wave slice is dynamic LDS, sized by the host
    # the one-launch step keeps nothing in scratch memory (scalar registers spill to VGPR lanes only)
    blk = [b for b in blocks if re.search(r"\.name:\s+\S*k_step_roles", b)]
    assert all(int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)) == 0 for b in blk)
    # one instantiation per kernel: the action dtype is a launch-time flag, not a template parameter (build time)
    assert len(usage("k_step_roles")) == 1
    # k_step_multi (several steps per launch): no more than it needed before its launch geometry moved to auv_multi_geom.h
    # (127 VGPRs, no spill, 16 bytes of private segment)
    blk = [b for b in blocks if re.search(r"\.name:\s+\S*k_step_multi", b)]
    assert len(blk) == 1
    for vgpr, spill, lds_static in usage("k_step_multi"):
        assert vgpr <= 127 and spill == 0 and lds_static == 0, (vgpr, spill, lds_static)
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk[0]).group(1)) <= 16
