"""The sixteen act / rollout entries of the fused policy launch -- (act, rollout) x (plain, squash, stacked, norm) x (default widths,
_arch) -- share one implementation per kind and differ by a variant trait.  This module pins what that sharing could silently permute:
every entry reports a bad call under ITS OWN name, fails on the same check with the same text as before, and enqueues nothing.

One 32-environment handle in two slices [0, 16), [16, 32); one call per shared check with exactly one thing wrong.  No call gets as
far as a launch.  The expected strings are the format strings of csrc/auv_capi_learn.hip and csrc/auv_capi_step.hip (check_policy_io,
the variants' own checks, check_slices, the rollouts' argument checks) as they stood before the entries were unified, written out
here."""
import ctypes as C
import functools
import os
import sys
import warnings

import pytest
import torch

from gym_auv_amd.config import effective_reference_config
from gym_auv_amd.scenarios import moving_obstacles_world
from gym_auv_amd.world import build_world, pack_bank

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

DEV = "cuda:0"
N, T, D = 32, 2, 15
BOUNDS = [0, 16, 32]
SLICES = [(0, 16), (16, 16)]
HIDDEN = (256, 128, 64)                                     # the only widths with a bf16 path: params_bf16 reaches the variants' own checks
AUV_EINVAL = -1
VARIANTS = ["", "_squash", "_stacked", "_norm"]
F32_ONLY = {"_squash": "a squashed policy is evaluated in exact f32 only (params_bf16 must be NULL)",
            "_stacked": "stacked rows are evaluated in exact f32 only (params_bf16 must be NULL)",
            "_norm": "normalised rows are evaluated in exact f32 only (params_bf16 must be NULL)"}


def _p(t):
    return C.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def _setup():
    """(env, fused, extra): the handle in two slices, the plain io blocks of a FusedActorCritic, and the buffers the stacked and the
    normalising io blocks point at."""
    import ppo
    from gym_auv_amd.batched_env import BatchedAuvEnv
    from gym_auv_amd.policy import FusedActorCritic
    cfg = effective_reference_config(use_lidar=True)
    cfg.vessel.sensor_use_feasibility_pooling = True
    bank = pack_bank([build_world(moving_obstacles_world(2000 + i)) for i in range(4)])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = BatchedAuvEnv(cfg, bank, N, device=DEV, rewarder="colav")
    assert env.obs_dim == D
    env.set_step_mode("side_by_side")
    env.reset()
    env.set_sub_batches(1, probe_streams=False)
    streams = [torch.cuda.Stream(device=DEV) for _ in SLICES]
    env._slices, env.sub_batches, env._sub_streams = list(SLICES), len(SLICES), streams
    env._bounds_c = (C.c_int32 * 3)(*BOUNDS)
    env._streams_c = (C.c_void_p * 2)(*[s.cuda_stream for s in streams])
    torch.manual_seed(3)
    fused = FusedActorCritic(ppo.ActorCritic(D, hidden=HIDDEN).to(DEV), env, rollout=T, seed=3)
    extra = dict(hist=torch.zeros((N, 2, D), device=DEV), stk=torch.zeros((N, 2), dtype=torch.int32, device=DEV),
                 table=torch.zeros((D, 2), device=DEV), part=torch.zeros((T + 1, 2, 2, D), device=DEV),
                 pcnt=torch.zeros((T + 1, 2), dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    return env, fused, extra


def _ios(variant):
    """Fresh, valid io blocks of both slices for `variant`, and the plain block inside each."""
    from gym_auv_amd import _capi
    env, fused, x = _setup()
    kind = {"": _capi.AuvPolicyIO, "_squash": _capi.AuvPolicyIO, "_stacked": _capi.AuvPolicyStack, "_norm": _capi.AuvPolicyNorm}[variant]
    arr = (kind * 2)()
    for i in range(2):
        inner = arr[i] if kind is _capi.AuvPolicyIO else arr[i].io
        C.memmove(C.byref(inner), C.byref(fused._ios[i]), C.sizeof(_capi.AuvPolicyIO))
        if variant == "_stacked":
            arr[i].hist, arr[i].stk, arr[i].frames = x["hist"].data_ptr(), x["stk"].data_ptr(), 1
        if variant == "_norm":
            arr[i].table, arr[i].part, arr[i].pcnt = x["table"].data_ptr(), x["part"].data_ptr(), x["pcnt"].data_ptr()
            arr[i].part_ld, arr[i].part_base, arr[i].clip_obs = 2, i, 10.0
    return arr, [arr[i] if kind is _capi.AuvPolicyIO else arr[i].io for i in range(2)]


def _cases(variant, rollout):
    """(label, mutate(inner blocks) -> overrides of the call, message behind "<entry>: ")."""
    env, fused, _ = _setup()

    def setf(i, field, value):
        def f(inner):
            setattr(inner[i], field, value)
            return {}
        return f
    out = [("null io", lambda inner: {"io": None}, "bad arguments" if rollout else "null io"),
           ("obs_dim", setf(0, "obs_dim", D + 1), "obs_dim %d, the handle's observation has %d columns" % (D + 1, D)),
           ("slice", lambda inner: {"bounds": [0, 16, 48], "e0": 16, "ne": 32},
            "bounds must run from 0 to %d" % N if rollout else "slice [16, 48) outside [0, %d)" % N),
           ("T", setf(0, "T", 0), "T must be >= 1"),
           ("params", setf(0, "params", fused.params.data_ptr() + 4), "params must be 16-byte, actions_out and ctr 8-byte aligned")]
    if rollout:
        out += [("t0 alone", lambda inner: {"g0": None}, "bad arguments"),
                ("negative counter", lambda inner: {"t0": (C.c_int64 * 2)(0, -1)}, "negative counter for slice 1")]
    if variant in F32_ONLY:
        out.append(("params_bf16", setf(0, "params_bf16", fused.params.data_ptr()), F32_ONLY[variant]))
    return out


@pytest.mark.parametrize("arch_entry", [False, True])
@pytest.mark.parametrize("rollout", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
def test_every_entry_refuses_under_its_own_name_and_enqueues_nothing(variant, rollout, arch_entry):
    from gym_auv_amd import _capi
    from gym_auv_amd.batched_env import _LIB as lib
    env, fused, _ = _setup()
    name = "auv_policy_" + ("rollout" if rollout else "act") + variant + ("_arch" if arch_entry else "")
    fn = getattr(lib, name)
    arch = _capi.AuvPolicyArch(*HIDDEN)
    torch.cuda.synchronize()
    ctr = [b["ctr"].clone() for b in fused.buf]
    actions = fused.actions.clone()
    for label, mutate, text in _cases(variant, rollout):
        arr, inner = _ios(variant)
        o = dict(io=arr, bounds=BOUNDS, e0=0, ne=16, t0=(C.c_int64 * 2)(0, 0), g0=(C.c_int64 * 2)(0, 0))
        o.update(mutate(inner))
        a = [C.byref(arch)] if arch_entry else []
        if rollout:
            rc = fn(env._h, 2, (C.c_int32 * 3)(*o["bounds"]), env._streams_c, o["io"], *a, _p(env.obs), _p(env.reward), _p(env.done), 1, 1,
                    o["t0"], o["g0"])
        else:
            rc = fn(env._h, o["e0"], o["ne"], C.byref(o["io"][0]) if o["io"] is not None else None, *a,
                    C.c_void_p(env._sub_streams[0].cuda_stream))
        msg = lib.auv_last_error().decode()
        print(name, label, rc, msg)
        assert rc == AUV_EINVAL, (name, label, rc, msg)
        assert msg.startswith(name + ": "), (name, label, msg)
        assert msg == name + ": " + text, (name, label, msg)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b["ctr"]) for a, b in zip(ctr, fused.buf)) and torch.equal(actions, fused.actions)
