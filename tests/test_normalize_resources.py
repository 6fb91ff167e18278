"""CPU (cross-compile only): the kernels of csrc/k16_policy_norm.hip within k6's and k12's budgets -- one k16_norm_act per hidden-width
triple, at most 128 VGPRs, nothing in scratch memory, no static LDS; the row, fold and return kernels without scratch."""
from kernel_resources import assert_policy_budget, describe, kernel_resources

SRC = "k16_policy_norm.hip"


def test_one_norm_act_kernel_per_listed_triple_within_the_policy_budget():
    from gym_auv_amd.policy import SUPPORTED_HIDDEN
    acts = [k for k in kernel_resources(SRC) if "k16_norm_act" in k["name"]]
    assert len(acts) == len(SUPPORTED_HIDDEN), [k["name"] for k in acts]
    for h in SUPPORTED_HIDDEN:
        tag = "PolArchILi%dELi%dELi%dEE" % h             # (Itanium mangling of PolArch<h1, h2, h3>)
        mine = [k for k in acts if tag in k["name"]]
        assert len(mine) == 1, (h, [k["name"] for k in acts])
        assert_policy_budget(mine[0])


def test_row_fold_and_return_kernels_use_no_scratch():
    ks = {k["name"]: k for k in kernel_resources(SRC)}
    for want in ("k16_norm_rows", "k16_norm_fold", "k16_return_env", "k16_return_merge", "k16_return_scale"):
        mine = [k for n, k in ks.items() if want in n]
        assert len(mine) == 1, (want, list(ks))
        print(describe(mine[0]))
        assert mine[0]["vgpr_spill"] == 0 and mine[0]["sgpr_spill"] == 0 and mine[0]["private"] == 0, describe(mine[0])
