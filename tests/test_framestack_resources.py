"""CPU (cross-compile only): register budget of the frame-stacking kernels (csrc/k12_policy_stacked.hip).

k12_stacked_act shares k6_policy_act's shape -- 512 threads and up to 65 KB of LDS per workgroup, two workgroups per CU -- which needs
at most 128 VGPRs and nothing in scratch memory.  k12_stack_frames is a row copy: a spilled register or a private array there would
mean the ring arithmetic had been turned into memory traffic.  Only the resource metadata is read."""
import os

import pytest

from gym_auv_amd.policy import SUPPORTED_HIDDEN
from kernel_resources import HIPCC, assert_policy_budget, describe, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_framestack_kernels_fit_their_register_budget():
    blocks = [k for k in kernel_resources("k12_policy_stacked.hip") if "k12_" in k["name"]]
    names = sorted(k["name"] for k in blocks)
    # one act kernel per listed hidden-width triple, the row copy at 4, 8 and 16 bytes per lane
    assert len(blocks) == len(SUPPORTED_HIDDEN) + 3 == 7, names
    assert sum("k12_stacked_act" in x for x in names) == len(SUPPORTED_HIDDEN) and sum("k12_stack_frames" in x for x in names) == 3, names
    for k in blocks:
        if "k12_stacked_act" in k["name"]:
            assert_policy_budget(k)             # (the tiles are dynamic LDS: nothing in front of the 16-byte aligned base)
        else:
            print(describe(k))
            assert k["vgpr_spill"] == 0 and k["private"] == 0, describe(k)
