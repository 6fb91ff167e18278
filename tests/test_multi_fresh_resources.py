"""CPU (cross-compile only): what the fresh-world multi-step launches take of a wave's resources.

`k_fresh_multi` and `k_fresh_record` are `k_step_multi` / `k_step_record` with the gated slot choice and the coherent restore in
the finish wave's reset (csrc/k_step_multi_body.inc, STEP_MULTI_FW): launched as the same ~600 k one-wave workgroups per 64-step
launch of 4096 environments, they too keep nothing in scratch memory -- no private segment, no spilled vector register -- and stay
within 128 vector registers (4 waves per SIMD).  Read from the metadata the compiler writes for gfx950, as
tests/test_multi_resources.py does; no instruction is looked at."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
# scalar registers spilled to vector lanes: the values this compiler gave at the commit that added the two kernels (14 and 16, read
# from the same metadata with the same flags; k_step_multi and k_step_record stand at 20 and 31)
SGPR_SPILLS = {"k_fresh_multi": 14, "k_fresh_record": 16}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_fresh_multi_step_kernels_keep_nothing_in_scratch():
    src = os.path.join(ROOT, "gym_auv_amd", "csrc", "k_step_fused.hip")
    tmp = tempfile.mkdtemp(prefix="auv_res_fresh_multi_")
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

    def field(blk, key):
        return int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))

    for name, sgpr_spills in SGPR_SPILLS.items():
        blk = [b for b in blocks if re.search(r"\.name:\s+\S*%s" % name, b)]
        assert len(blk) == 1, name
        got = {k: field(blk[0], k) for k in ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count", "sgpr_spill_count")}
        print(name, got)
        assert got["private_segment_fixed_size"] == 0, (name, got)
        assert got["vgpr_spill_count"] == 0, (name, got)
        assert got["vgpr_count"] <= 128, (name, got)
        assert got["sgpr_spill_count"] <= sgpr_spills, (name, got)
