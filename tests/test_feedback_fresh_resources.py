"""CPU (cross-compile only): what the closed-loop launches on a fresh world per reset take of a wave's resources, in the manner of
tests/test_feedback_hidden_resources.py and tests/test_multi_fresh_resources.py: `k_fresh_feedback`, `k_fresh_sector_feedback` and
`k_fresh_hidden_feedback` (the body with the feedback law AND the gated slot choice in its finish wave) keep nothing in scratch
memory -- no private segment, no spilled vector register -- stay within 128 vector registers and spill no more scalar registers to
vector lanes than the committed build does.  Read from the metadata the compiler writes for gfx950; no instruction is looked at.
(The kernels' names contain none of k_step_feedback, k_step_sector_feedback, k_step_hidden_feedback, k_step_multi, k_step_record,
k_fresh_multi, k_fresh_record: the sibling tests find their kernels by substring and expect one match.  That the other kernels of
the file were left alone is what those tests hold, unchanged.)"""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
# what the compiler's metadata shows for the committed k_step_fused.hip (k_step_feedback: 21, k_step_sector_feedback and
# k_step_hidden_feedback: 49, k_fresh_record: 16)
SGPR_SPILLS = {"k_fresh_feedback": 30, "k_fresh_sector_feedback": 57, "k_fresh_hidden_feedback": 52}


@pytest.fixture(scope="module")
def metadata():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    src = os.path.join(ROOT, "gym_auv_amd", "csrc", "k_step_fused.hip")
    tmp = tempfile.mkdtemp(prefix="auv_res_feedback_fresh_")
    try:
        subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-c", src,
                        "-o", os.path.join(tmp, "k.o"), "-save-temps"], cwd=tmp, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        asm = [f for f in os.listdir(tmp) if f.endswith("gfx950.s")]
        assert asm, os.listdir(tmp)
        text = open(os.path.join(tmp, asm[0])).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return re.split(r"\n\s+- \.agpr_count:", text)               # one metadata map per kernel


@pytest.mark.parametrize("kernel", sorted(SGPR_SPILLS))
def test_fresh_feedback_kernels_keep_nothing_in_scratch(metadata, kernel):
    blk = [b for b in metadata if re.search(r"\.name:\s+\S*%s" % kernel, b)]
    assert len(blk) == 1
    got = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk[0]).group(1))
           for k in ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count", "sgpr_spill_count")}
    print(kernel, got)
    assert got["private_segment_fixed_size"] == 0, got
    assert got["vgpr_spill_count"] == 0, got
    assert got["vgpr_count"] <= 128, got
    assert got["sgpr_spill_count"] <= SGPR_SPILLS[kernel], got
