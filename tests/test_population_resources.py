"""CPU (cross-compile only): register budget of the population kernels (csrc/k11_population.hip).

k11_population_act shares k9_policy_eval's shape -- 512 threads and up to 65 KB of LDS per workgroup, two workgroups per CU -- which
needs at most 128 VGPRs and nothing in scratch memory.  k11_perturb and k11_es_update are element-wise: a spilled register or a
private array there would mean the hash or the padding test had been turned into memory traffic."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_population_kernels_fit_their_register_budget():
    src = os.path.join(ROOT, "gym_auv_amd", "csrc", "k11_population.hip")
    tmp = tempfile.mkdtemp(prefix="auv_res11_")
    try:
        subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-c", src,
                        "-o", os.path.join(tmp, "k.o"), "-save-temps"], cwd=tmp, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        asm = [f for f in os.listdir(tmp) if f.endswith("gfx950.s")]
        assert asm, os.listdir(tmp)
        text = open(os.path.join(tmp, asm[0])).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    blocks = [b for b in re.split(r"\n\s+- \.agpr_count:", text) if re.search(r"\.name:\s+\S*k11_", b)]
    names = sorted(re.search(r"\.name:\s+(\S+)", b).group(1) for b in blocks)
    assert len(blocks) == 3 and all(any(k in x for x in names) for k in ("k11_population_act", "k11_perturb", "k11_es_update")), names
    for b in blocks:
        name = re.search(r"\.name:\s+(\S+)", b).group(1)
        vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1))
        private = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1))
        static_lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", b).group(1))
        print("%s: %d VGPRs, %d spilled, %d bytes private, %d bytes static LDS" % (name, vgpr, spill, private, static_lds))
        assert spill == 0 and private == 0, (name, spill, private)
        if "k11_population_act" in name:
            assert vgpr <= 128, (name, vgpr)
            assert static_lds == 0, (name, static_lds)      # the tiles are dynamic LDS: nothing in front of the 16-byte aligned base
