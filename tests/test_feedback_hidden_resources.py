"""CPU (cross-compile only): what the closed-loop launch with a hidden layer in its law takes of a wave's resources, in the manner
of tests/test_feedback_sectors_resources.py: `k_step_hidden_feedback` keeps nothing in scratch memory -- no private segment, no
spilled vector register -- stays within 128 vector registers and spills no more scalar registers to vector lanes than the committed
build does (a lane's 2 x 27 parameters pass through registers one batch of eight inputs at a time, and the 24 inputs are taken from
the group by DPP moves where they are multiplied: an array of either does not fit).  Read from the metadata the compiler writes for
gfx950; no instruction is looked at.  (The kernel's name contains none of k_step_feedback, k_step_sector_feedback, k_step_multi,
k_step_record: the sibling tests find their kernels by substring and expect one match.  That the other kernels of the file were
left alone is what those tests hold, unchanged.)"""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SGPR_SPILLS = 49          # what the compiler's metadata shows for the committed k_step_fused.hip (k_step_sector_feedback: 49)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_feedback_hidden_kernel_keeps_nothing_in_scratch():
    src = os.path.join(ROOT, "gym_auv_amd", "csrc", "k_step_fused.hip")
    tmp = tempfile.mkdtemp(prefix="auv_res_feedback_hidden_")
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
    blk = [b for b in blocks if re.search(r"\.name:\s+\S*k_step_hidden_feedback", b)]
    assert len(blk) == 1
    got = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk[0]).group(1))
           for k in ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count", "sgpr_spill_count")}
    print("k_step_hidden_feedback", got)
    assert got["private_segment_fixed_size"] == 0, got
    assert got["vgpr_spill_count"] == 0, got
    assert got["vgpr_count"] <= 128, got
    assert got["sgpr_spill_count"] <= SGPR_SPILLS, got
