"""CPU (cross-compile only): what the renderer's two kernels (csrc/k10_render.hip) take of a wave's resources, in the manner of
tests/test_feedback_hidden_resources.py: neither keeps anything in scratch memory -- no private segment, no spilled vector
register -- and the rasteriser's workgroup stays within 16 KiB of LDS (the staged batch of 256 segments is 8 KiB of it).  Read
from the metadata the compiler writes for gfx950; no instruction is looked at."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_render_kernels_keep_nothing_in_scratch_and_fit_16_kib_of_lds():
    src = os.path.join(ROOT, "gym_auv_amd", "csrc", "k10_render.hip")
    tmp = tempfile.mkdtemp(prefix="auv_res_render_")
    try:
        subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-c", src,
                        "-o", os.path.join(tmp, "k.o"), "-save-temps"], cwd=tmp, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        asm = [f for f in os.listdir(tmp) if f.endswith("gfx950.s")]
        assert asm, os.listdir(tmp)
        text = open(os.path.join(tmp, asm[0])).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    blocks = re.split(r"\n\s+- \.agpr_count:", text)           # one metadata map per kernel
    for name in ("k10_frame_geometry", "k10_raster"):
        blk = [b for b in blocks if re.search(r"\.name:\s+\S*%s" % name, b)]
        assert len(blk) == 1, name
        got = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk[0]).group(1))
               for k in ("private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size")}
        print(name, got)
        assert got["private_segment_fixed_size"] == 0, got
        assert got["vgpr_spill_count"] == 0, got
        if name == "k10_raster":
            assert 8192 <= got["group_segment_fixed_size"] <= 16 * 1024, got


def test_the_sweep_and_the_renderer_share_one_definition_of_the_mover_pentagon():
    """MoverSegs lives in csrc/auv_mover_segs.h alone; k2_lidar.hip (hence k_step_fused.hip, which includes it) and
    k10_render.hip include that header and define no copy."""
    csrc = os.path.join(ROOT, "gym_auv_amd", "csrc")
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".h", ".inc")):
            txt = open(os.path.join(csrc, f)).read()
            assert ("struct MoverSegs" in txt) == (f == "auv_mover_segs.h"), f
    for f in ("k2_lidar.hip", "k10_render.hip"):
        assert '#include "auv_mover_segs.h"' in open(os.path.join(csrc, f)).read()
