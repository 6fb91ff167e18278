"""CPU (cross-compile only): register budget of the population kernels (csrc/k11_population.hip).

k11_population_act shares k9_policy_eval's shape -- 512 threads and up to 65 KB of LDS per workgroup, two workgroups per CU -- which
needs at most 128 VGPRs and nothing in scratch memory.  k11_perturb and k11_es_update are element-wise: a spilled register or a
private array there would mean the hash or the padding test had been turned into memory traffic."""
import os

import pytest

from kernel_resources import HIPCC, describe, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_population_kernels_fit_their_register_budget():
    blocks = [k for k in kernel_resources("k11_population.hip") if "k11_" in k["name"]]
    names = sorted(k["name"] for k in blocks)
    assert len(blocks) == 3 and all(any(n in x for x in names) for n in ("k11_population_act", "k11_perturb", "k11_es_update")), names
    for k in blocks:
        print(describe(k))
        assert k["vgpr_spill"] == 0 and k["private"] == 0, describe(k)
        if "k11_population_act" in k["name"]:
            assert k["vgpr"] <= 128, (k["name"], k["vgpr"])
            assert k["static_lds"] == 0, (k["name"], k["static_lds"])      # the tiles are dynamic LDS: nothing in front of the 16-byte aligned base
