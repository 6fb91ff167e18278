"""CPU (cross-compile only): register budget of k8_clone, the supervised row pass (csrc/k8_ppo_update.hip).

k8_clone is k8_rows with another head: the same launch bounds (512 threads, four workgroups per CU at the narrow widths), the same
LDS tile.  Its head does less than PPO's (no ratio, no clip branch), so it must not need more registers than k8_rows in the same
build, nothing spilled and nothing in scratch memory."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_clone_row_pass_fits_the_register_budget_of_the_ppo_row_pass():
    src = os.path.join(ROOT, "gym_auv_amd", "csrc", "k8_ppo_update.hip")
    tmp = tempfile.mkdtemp(prefix="auv_res8c_")
    try:
        subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-c", src,
                        "-o", os.path.join(tmp, "k.o"), "-save-temps"], cwd=tmp, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        asm = [f for f in os.listdir(tmp) if f.endswith("gfx950.s")]
        assert asm, os.listdir(tmp)
        text = open(os.path.join(tmp, asm[0])).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    got = {}
    for b in re.split(r"\n\s+- \.agpr_count:", text):
        m = re.search(r"\.name:\s+(\S+)", b)
        for key in ("k8_rows", "k8_clone"):
            if m and key in m.group(1):
                assert key not in got, m.group(1)
                got[key] = dict(vgpr=int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1)),
                                spill=int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)),
                                private=int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)),
                                static_lds=int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", b).group(1)))
    print(got)
    assert sorted(got) == ["k8_clone", "k8_rows"], sorted(got)
    for key, r in got.items():
        assert r["spill"] == 0 and r["private"] == 0, (key, r)
        assert r["static_lds"] == 0, (key, r)                        # the tile is dynamic LDS, sized per observation width
    assert got["k8_clone"]["vgpr"] <= got["k8_rows"]["vgpr"] <= 128, got
