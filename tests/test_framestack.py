"""CPU: the NumPy mirror of frame stacking (gym_auv_amd/framestack.py: stack_reference) against arrays written out by hand, the
arguments FusedActorCritic(frames=...) refuses, and the new exports in header and binding."""
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hand_case():
    """D = 2, N = 2, k = 3, T = 6.  Environment 0 observes (10 t + 1, 10 t + 2), environment 1 (100 + t, 200 + t); environment 0 is done
    in front of step 2 (its observation there is the first of a new episode)."""
    T, N, D = 6, 2, 2
    obs = np.zeros((T, N, D), dtype=np.float32)
    for t in range(T):
        obs[t, 0] = (10 * t + 1, 10 * t + 2)
        obs[t, 1] = (100 + t, 200 + t)
    done = np.zeros((T, N), dtype=np.uint8)
    done[2, 0] = 1
    want = np.array([
        # environment 0                    environment 1
        [[1, 2, 0, 0, 0, 0],               [100, 200, 0, 0, 0, 0]],                    # t = 0: age 1 -- zeros for j >= age
        [[11, 12, 1, 2, 0, 0],             [101, 201, 100, 200, 0, 0]],                # t = 1: age 2
        [[21, 22, 0, 0, 0, 0],             [102, 202, 101, 201, 100, 200]],            # t = 2: env 0 done -> its frame starts a history
        [[31, 32, 21, 22, 0, 0],           [103, 203, 102, 202, 101, 201]],            # t = 3: env 0 sees only frames of the new episode
        [[41, 42, 31, 32, 21, 22],         [104, 204, 103, 203, 102, 202]],            # t = 4: full again
        [[51, 52, 41, 42, 31, 32],         [105, 205, 104, 204, 103, 203]],            # t = 5: the ring has wrapped
    ], dtype=np.float32)
    return obs, done, want


def test_stack_reference_matches_arrays_written_out_by_hand():
    from gym_auv_amd.framestack import stack_reference
    obs, done, want = _hand_case()
    rows, state = stack_reference(obs, done, 3)
    assert rows.dtype == np.float32 and rows.shape == (6, 2, 6)
    assert np.array_equal(rows, want)
    # zeros for j >= age, and the frame behind a done starts a history
    assert not rows[0, :, 2:].any() and not rows[1, :, 4:].any() and not rows[2, 0, 2:].any() and not rows[3, 0, 4:].any()
    assert np.array_equal(rows[2, 0, :2], obs[2, 0]) and np.array_equal(rows[3, 0, 2:4], obs[2, 0])
    assert state["age"].tolist() == [3, 3] and state["pos"].tolist() == [0, 0] and state["hist"].shape == (2, 3, 2)
    # the ring as the device holds it: slot pos is the newest frame
    assert np.array_equal(state["hist"][:, 0], obs[5]) and np.array_equal(state["hist"][:, 2], obs[4]) and np.array_equal(state["hist"][:, 1], obs[3])


@pytest.mark.parametrize("cut", [1, 2, 3, 5])
def test_stack_reference_continues_from_a_returned_state(cut):
    from gym_auv_amd.framestack import stack_reference
    obs, done, want = _hand_case()
    a, state = stack_reference(obs[:cut], done[:cut], 3)
    keep = {k: v.copy() for k, v in state.items()}
    b, end = stack_reference(obs[cut:], done[cut:], 3, state)
    assert np.array_equal(np.concatenate([a, b]), want)
    assert all(np.array_equal(state[k], keep[k]) for k in keep)              # the state passed in is not modified
    _, one = stack_reference(obs, done, 3)
    assert all(np.array_equal(end[k], one[k]) for k in one)


def test_stack_reference_with_one_frame_is_the_observation_and_bad_arguments_raise():
    from gym_auv_amd.framestack import stack_reference
    obs, done, _ = _hand_case()
    rows, _ = stack_reference(obs, done, 1)
    assert np.array_equal(rows, obs)
    for frames in (0, 9):
        with pytest.raises(ValueError, match="frames"):
            stack_reference(obs, done, frames)
    with pytest.raises(ValueError, match="done_seq"):
        stack_reference(obs, done[:, :1], 3)


def _net(in_dim):
    import torch.nn as nn
    import torch

    def mlp(out):
        return nn.Sequential(nn.Linear(in_dim, 256), nn.Tanh(), nn.Linear(256, 128), nn.Tanh(), nn.Linear(128, 64), nn.Tanh(), nn.Linear(64, out))
    net = nn.Module()
    net.pi, net.v = mlp(2), mlp(1)
    net.log_std = nn.Parameter(torch.zeros(2))
    return net


def test_fused_actor_critic_refuses_a_net_of_the_wrong_width_bf16_and_bad_frame_counts():
    """The checks run before the environment is touched: a stand-in with the two attributes they read is enough."""
    from gym_auv_amd.policy import FusedActorCritic
    env = types.SimpleNamespace(obs_dim=26, device="cpu")
    with pytest.raises(ValueError) as e:
        FusedActorCritic(_net(26), env, rollout=4, frames=4)                 # the net was built for ONE frame
    assert "104" in str(e.value) and "26" in str(e.value) and "in_features" in str(e.value)
    with pytest.raises(ValueError) as e:
        FusedActorCritic(_net(100), env, rollout=4, frames=4)
    assert "104" in str(e.value) and "100" in str(e.value)
    with pytest.raises(ValueError) as e:
        FusedActorCritic(_net(20), env, rollout=4)                           # one frame: the same message, with both numbers
    assert "26" in str(e.value) and "20" in str(e.value) and "in_features" in str(e.value)
    with pytest.raises(ValueError, match="bf16"):
        FusedActorCritic(_net(104), env, rollout=4, frames=4, bf16=True)
    for frames in (0, 9):
        with pytest.raises(ValueError, match="frames"):
            FusedActorCritic(_net(26), env, rollout=4, frames=frames)


def test_frame_stack_refuses_bad_shapes():
    from gym_auv_amd.framestack import FrameStack
    for frames in (0, 9):
        with pytest.raises(ValueError, match="frames"):
            FrameStack((4, 6), frames, device="cpu")
    with pytest.raises(ValueError):
        FrameStack((0, 6), 2, device="cpu")


def test_the_new_exports_are_in_header_and_binding():
    import ctypes as C
    from gym_auv_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "auv_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("auv_policy_act_stacked", "auv_policy_rollout_stacked", "auv_stack_frames"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _capi.EXPORTED_SYMBOLS
        assert hasattr(_capi.load_library(), name)
    assert re.search(r"#define\s+AUV_ABI_VERSION\s+5\b", hdr) and _capi.ABI_VERSION == 5
    assert int(re.search(r"#define\s+AUV_MAX_FRAMES\s+(\d+)", hdr).group(1)) == _capi.MAX_FRAMES == 8
    # auv_policy_stack_t: the plain io block first, then hist, stk, frames
    s = _capi.AuvPolicyStack
    assert s.io.offset == 0 and s.hist.offset == C.sizeof(_capi.AuvPolicyIO) and s.stk.offset == s.hist.offset + 8
    assert s.frames.offset == s.stk.offset + 8 and C.sizeof(s) == C.sizeof(_capi.AuvPolicyIO) + 24


def test_struct_size_matches_the_header(tmp_path):
    import ctypes as C
    import subprocess
    from gym_auv_amd import _capi
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu\\n", '
                   'sizeof(auv_policy_stack_t), offsetof(auv_policy_stack_t, hist), offsetof(auv_policy_stack_t, stk), '
                   'offsetof(auv_policy_stack_t, frames));return 0;}\n' % os.path.join(ROOT, "include", "auv_hip.h"))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    size, o_hist, o_stk, o_frames = map(int, subprocess.check_output([str(exe)]).split())
    s = _capi.AuvPolicyStack
    assert (C.sizeof(s), s.hist.offset, s.stk.offset, s.frames.offset) == (size, o_hist, o_stk, o_frames)
