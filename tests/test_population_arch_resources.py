"""CPU (cross-compile only): register budget of the population kernels of the non-default hidden widths (csrc/k14_population_arch.hip).

NINE kernels: act, perturb and update for each of the three listed triples other than the reference's.  All three bodies are templates
(csrc/auv_population_pass.h) -- the perturbation and the ES estimate too, although only pop_live<A> in them depends on the widths:
with the widths compile-time the segment offsets of the padding test fold to constants, as they do in the reference's kernels, and
nothing about the widths travels as a kernel argument.  The act kernels share k9_policy_eval's shape -- 512 threads, up to 65 KB of LDS
per workgroup, two workgroups per CU -- which needs at most 128 VGPRs and nothing in scratch memory; a spill or a private array in
the element-wise two would mean the hash or the padding test had been turned into memory traffic."""
import os

import pytest

from kernel_resources import HIPCC, describe, kernel_resources

TRIPLES = [(128, 128, 64), (128, 64, 64), (64, 64, 64)]
BODIES = ("k14_pop_act", "k14_pop_perturb", "k14_pop_update")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_population_arch_kernels_fit_their_register_budget():
    kernels = kernel_resources("k14_population_arch.hip")
    names = sorted(k["name"] for k in kernels)
    assert len(kernels) == 9 and not any("k11_" in n for n in names), names
    for h1, h2, h3 in TRIPLES:
        arch = "PolArchILi%dELi%dELi%dEE" % (h1, h2, h3)         # (Itanium mangling of PolArch<h1, h2, h3>)
        for body in BODIES:
            assert sum(1 for n in names if body in n and arch in n) == 1, (body, arch, names)
    assert not any("PolArchILi256ELi128ELi64EE" in n for n in names), names      # the reference's triple stays in k11_population.hip
    for k in kernels:
        print(describe(k))
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["private"] == 0, describe(k)
        if "k14_pop_act" in k["name"]:
            assert k["vgpr"] <= 128, (k["name"], k["vgpr"])
            assert k["static_lds"] == 0, (k["name"], k["static_lds"])      # the tiles are dynamic LDS: nothing in front of the 16-byte aligned base
