"""CPU (cross-compile only): register budget of the policy evaluation kernels (csrc/k9_policy_eval.hip).

k9_policy_eval shares k6_policy_act's shape -- 512 threads and up to 65 KB of LDS per workgroup, two workgroups per CU -- which needs
at most 128 VGPRs, and nothing in scratch memory: a spilled register or a private array in its epilogue would put trips to memory
behind every row."""
import os

import pytest

from gym_auv_amd.policy import SUPPORTED_HIDDEN
from kernel_resources import HIPCC, assert_policy_budget, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_policy_eval_kernels_fit_their_register_budget():
    blocks = [k for k in kernel_resources("k9_policy_eval.hip") if "k9_" in k["name"]]
    names = sorted(k["name"] for k in blocks)
    # one evaluation kernel per listed hidden-width triple, and the planner's score
    assert len(blocks) == len(SUPPORTED_HIDDEN) + 1 == 5, names
    assert sum("k9_policy_eval" in x for x in names) == len(SUPPORTED_HIDDEN) and sum("k9_plan_score_v" in x for x in names) == 1, names
    for k in blocks:
        assert_policy_budget(k)                 # (the tiles are dynamic LDS: nothing in front of the 16-byte aligned base)
