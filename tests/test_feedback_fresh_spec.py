"""CPU: `FreshWorlds(closed_loop=True)` -- the opt-in for closed-loop launches on a fresh world per reset: its validation, the
unchanged defaults, and what the host and the header say about the value 2 of auv_fresh_worlds_multi."""
import dataclasses
import os
import re

import pytest

from gym_auv_amd.devgen import FreshWorlds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_defaults_are_unchanged_and_closed_loop_is_off():
    spec = FreshWorlds()
    assert spec.closed_loop is False and spec.multi_step is False
    assert FreshWorlds(depth=3, multi_step=True).closed_loop is False
    # the record of fields is the one earlier callers know: the opt-in is an init-only argument kept as a plain attribute
    assert [f.name for f in dataclasses.fields(spec)] == ["depth", "n_moving", "n_static", "seed", "env_index_base", "batch_cap", "period",
                                                          "multi_step"]
    with pytest.raises(dataclasses.FrozenInstanceError):
        spec.closed_loop = True


@pytest.mark.parametrize("depth", [3, 4, 8])
def test_closed_loop_accepts_three_slots_and_more(depth):
    spec = FreshWorlds(depth=depth, multi_step=True, closed_loop=True)
    assert spec.closed_loop is True and spec.multi_step is True and spec.depth == depth


@pytest.mark.parametrize("depth", [1, 2])
def test_closed_loop_refuses_fewer_than_three_slots(depth):
    with pytest.raises(ValueError, match="depth >= 3"):
        FreshWorlds(depth=depth, multi_step=True, closed_loop=True)


def test_closed_loop_requires_multi_step():
    with pytest.raises(ValueError, match="multi_step=True"):
        FreshWorlds(depth=3, closed_loop=True)
    with pytest.raises(ValueError, match="multi_step=True"):
        FreshWorlds(depth=2, closed_loop=True)


def test_replace_takes_the_opt_in_when_it_is_named():
    spec = FreshWorlds(depth=4, multi_step=True, closed_loop=True)
    assert dataclasses.replace(spec, seed=3, closed_loop=True).closed_loop is True
    assert dataclasses.replace(spec, seed=3, closed_loop=False).closed_loop is False
    with pytest.raises(ValueError, match="multi_step=True"):
        dataclasses.replace(spec, multi_step=False, closed_loop=True)


def test_the_value_two_is_documented_and_kept_by_the_host():
    hdr = open(os.path.join(ROOT, "include", "auv_hip.h")).read()
    doc = hdr[hdr.index("Launches of SEVERAL steps with a fresh world on every reset"):hdr.index("int auv_fresh_worlds_multi(")]
    assert "on == 2" in doc and "auv_step_feedback" in doc
    assert re.search(r"\bint auv_fresh_worlds_multi\(auv_handle_t\* h, int32_t on\);", hdr)            # no new export
    host = open(os.path.join(ROOT, "gym_auv_amd", "csrc", "auv_capi.hip")).read()
    assert "f.feedback = on == 2" in host
    step = open(os.path.join(ROOT, "gym_auv_amd", "csrc", "auv_capi_step.hip")).read()
    assert "AUV_EINVAL, h->fw.feedback)" in step                     # the closed-loop entries' check_multi takes the flag
    env = open(os.path.join(ROOT, "gym_auv_amd", "batched_env.py")).read()
    assert "auv_fresh_worlds_multi(self._h, 2 if spec.closed_loop else 1)" in env
