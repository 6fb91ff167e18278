"""CPU (cross-compile only): register budget of the frame-stacking kernels (csrc/k12_policy_stacked.hip).

k12_stacked_act shares k6_policy_act's shape -- 512 threads and up to 65 KB of LDS per workgroup, two workgroups per CU -- which needs
at most 128 VGPRs and nothing in scratch memory.  k12_stack_frames is a row copy: a spilled register or a private array there would
mean the ring arithmetic had been turned into memory traffic.  Only the resource metadata is read."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_framestack_kernels_fit_their_register_budget():
    src = os.path.join(ROOT, "gym_auv_amd", "csrc", "k12_policy_stacked.hip")
    tmp = tempfile.mkdtemp(prefix="auv_res12_")
    try:
        subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-c", src,
                        "-o", os.path.join(tmp, "k.o"), "-save-temps"], cwd=tmp, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        asm = [f for f in os.listdir(tmp) if f.endswith("gfx950.s")]
        assert asm, os.listdir(tmp)
        text = open(os.path.join(tmp, asm[0])).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    blocks = [b for b in re.split(r"\n\s+- \.agpr_count:", text) if re.search(r"\.name:\s+\S*k12_", b)]
    names = sorted(re.search(r"\.name:\s+(\S+)", b).group(1) for b in blocks)
    # one act kernel, the row copy at 4, 8 and 16 bytes per lane
    assert len(blocks) == 4 and sum("k12_stacked_act" in x for x in names) == 1 and sum("k12_stack_frames" in x for x in names) == 3, names
    for b in blocks:
        name = re.search(r"\.name:\s+(\S+)", b).group(1)
        vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1))
        private = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1))
        static_lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", b).group(1))
        print("%s: %d VGPRs, %d spilled, %d bytes private, %d bytes static LDS" % (name, vgpr, spill, private, static_lds))
        assert spill == 0 and private == 0, (name, spill, private)
        if "k12_stacked_act" in name:
            assert vgpr <= 128, (name, vgpr)
            assert static_lds == 0, (name, static_lds)      # the tiles are dynamic LDS: nothing in front of the 16-byte aligned base
