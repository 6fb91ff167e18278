#!/usr/bin/env python
"""Bit equality of the four fused policy launches between two builds of the library.

    AUV_HIP_LIB=<library A> python tools/policy_ab.py run a.npz
    AUV_HIP_LIB=<library B> python tools/policy_ab.py run b.npz        (each in a fresh process: the library is loaded once)
    python tools/policy_ab.py compare a.npz b.npz                      (exit status 1 unless every array is equal, bit for bit)
    ... run a.npz --hidden 128,64,64                                   (another listed hidden-width triple; default 256,128,64)

`run` drives one fixed scenario through auv_policy_act / auv_policy_rollout (device counters and host-named counters, mu_out /
eps_out set, once with params_bf16), auv_policy_eval (with and without idx; policy only, value only, both; logp on stored actions),
auv_population_act / auv_population_rollout (2 members of 16 rows) and auv_policy_act_stacked / auv_policy_rollout_stacked (frames 1
and 3, episodes that end inside the window), each at an even (6, LiDAR off) and an odd (15, feasibility-pooled LiDAR) observation
width, with 40 environments -- two full tiles and one of 8 rows -- and writes every output to the .npz.  tools/build_variant.sh builds
a second library next to the product one.  With another triple than the default the same scenario goes through the *_arch entries;
the bf16 pass and the population launches, which exist for the default widths only, are left out.

A one-off A/B aid, not an API example: it reaches into private attributes of FusedActorCritic and BatchedAuvEnv (_ios, _sios, _t, _g,
_bounds_c, _streams_c, _sub_streams, _h) to call the C entry points the wrappers do not expose (NULL counters, frames = 1 through the
stacked calls) and has to follow the wrappers when they change."""
import ctypes as C
import hashlib
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

DEV = "cuda:0"
N, MAX_T = 40, 5
HIDDEN = (256, 128, 64)                # --hidden: the nets' hidden widths
WIDTHS = {"d6": dict(use_lidar=False, pooled=False), "d15": dict(use_lidar=True, pooled=True)}


def _env(kind, n=N):
    """The environment of tests/test_gpu_framestack.py (episodes of 5 steps, odd environments three steps into theirs) at the widths of
    tests/test_gpu_policy.py (LiDAR off: 6 columns) and tests/test_gpu_policy_eval.py (pooled: 15 columns)."""
    import torch
    from gym_auv_amd.batched_env import BatchedAuvEnv
    from gym_auv_amd.config import effective_reference_config
    from gym_auv_amd.scenarios import moving_obstacles_world
    from gym_auv_amd.world import build_world, pack_bank
    kw = WIDTHS[kind]
    cfg = effective_reference_config(use_lidar=kw["use_lidar"])
    cfg.vessel.sensor_use_feasibility_pooling = kw["pooled"]
    cfg.episode.max_timesteps = MAX_T
    bank = pack_bank([build_world(moving_obstacles_world(2000 + i) if kw["use_lidar"] else moving_obstacles_world(2000 + i, 0, 0)) for i in range(16)])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = BatchedAuvEnv(cfg, bank, n, device=DEV, rewarder="colav" if kw["use_lidar"] else "pathfollow")
    env.reset()
    zero = torch.zeros((n, 2), dtype=torch.float32, device=DEV)
    for _ in range(3):
        env.step(zero)
    mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
    mask[0::2] = 1
    env.reset(mask)
    torch.cuda.synchronize()
    env.set_sub_batches(1, probe_streams=False)
    assert env.obs_dim == int(kind[1:]), env.obs_dim
    return env


def _net(width, seed=5):
    import ppo
    import torch
    torch.manual_seed(seed)
    net = ppo.ActorCritic(width, hidden=HIDDEN).to(DEV)
    with torch.no_grad():
        net.log_std.copy_(torch.tensor([-0.5, -1.1]))
        for m in net.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.uniform_(-0.3, 0.3)
    return net


def _fused(env, T, frames=1, **kw):
    from gym_auv_amd.policy import FusedActorCritic
    return FusedActorCritic(_net(frames * env.obs_dim), env, rollout=T, debug=True, seed=5, reward_scale=0.01, reward_clip=50.0, frames=frames, **kw)


def _keep(out, tag, fused, env):
    import torch
    torch.cuda.synchronize()
    for name, x in zip("O A LP V R Dn".split(), fused.buffers()):
        out["%s/%s" % (tag, name)] = x.cpu().numpy()
    out[tag + "/actions_out"] = fused.actions.cpu().numpy()
    out[tag + "/mu_out"], out[tag + "/eps_out"] = fused.mu.cpu().numpy(), fused.eps.cpu().numpy()
    out[tag + "/ctr"] = fused.buf[0]["ctr"].cpu().numpy()
    out[tag + "/obs"], out[tag + "/done"] = env.obs.cpu().numpy(), env.done.cpu().numpy()
    if fused.stack is not None:
        out[tag + "/hist"], out[tag + "/stk"] = fused.stack.hist.cpu().numpy(), fused.stack.stk.cpu().numpy()


def _check(lib, rc):
    if rc != 0:
        raise RuntimeError(lib.auv_last_error())


def _entry(lib, name, fused):
    """The C entry `name` for fused's widths: itself for the default triple, name_arch (the triple goes in behind the io argument, the
    fifth of a rollout call and the fourth of an act call) for any other."""
    if fused._arch is None:
        return getattr(lib, name)
    fn, at = getattr(lib, name + "_arch"), 5 if "rollout" in name else 4
    return lambda *a: fn(*a[:at], C.byref(fused._arch), *a[at:])


def _policy(out, kind, bf16):
    """auv_policy_act (device counters), auv_policy_rollout with host-named and with device counters: T = 3 plus the flush launch"""
    import torch
    from gym_auv_amd.batched_env import _LIB
    T = 3
    tag = "policy/%s%s" % (kind, "/bf16" if bf16 else "")
    for how in ("act", "rollout_host", "rollout_device"):
        env = _env(kind)
        fused = _fused(env, T, bf16=bf16)
        fused.begin_rollout()
        if how == "act":
            for _ in range(T):
                fused.act(0)
                env.step_slice(0, fused.actions)
            fused.act(0)
        elif how == "rollout_host":
            fused.rollout(T, flush=True)
        else:
            _check(_LIB, _entry(_LIB, "auv_policy_rollout", fused)(env._h, 1, env._bounds_c, env._streams_c, fused._ios, C.c_void_p(env.obs.data_ptr()),
                                                 C.c_void_p(env.reward.data_ptr()), C.c_void_p(env.done.data_ptr()), T, 1, None, None))
        _keep(out, "%s/%s" % (tag, how), fused, env)
        if how == "act" and not bf16:
            _eval(out, kind, fused)
        env.close()


def _eval(out, kind, fused):
    """auv_policy_eval on M = 40 rows: with and without idx; policy only, value only, both; logp on given actions"""
    import torch
    from gym_auv_amd.policy import policy_eval
    D = fused.in_dim
    g = torch.Generator().manual_seed(11)
    X = torch.randn(N + 9, D, generator=g).to(DEV)
    A = torch.randn(N, 2, generator=g).to(DEV)
    idx = torch.randint(0, N + 9, (N,), generator=g).to(DEV)
    for iname, rows, ix in (("rows", X[:N], None), ("idx", X, idx)):
        for wname, want in (("pi", ("mu", "action", "logp")), ("v", ("value",)), ("both", ("mu", "action", "value", "logp")), ("mu", ("mu",))):
            r = policy_eval(fused.params, D, rows, idx=ix, actions=A if "logp" in want else None, want=want, action_map=fused.action_map,
                            hidden=fused.hidden)
            torch.cuda.synchronize()
            for k, v in r.items():
                out["eval/%s/%s/%s/%s" % (kind, iname, wname, k)] = v.cpu().numpy()


def _population(out, kind):
    """auv_population_act and auv_population_rollout: 2 members of 16 rows, 3 steps plus the flush launch"""
    import torch
    from gym_auv_amd.population import PolicyPopulation, population_act
    env = _env(kind, n=32)
    pop = PolicyPopulation(env, 2, 16, net=_net(env.obs_dim), seed=9)
    pop.perturb(0.05, 1)
    r = population_act(pop.members, pop.obs_dim, pop.G, env.obs, want=("mu", "action"), action_map=pop.action_map)
    torch.cuda.synchronize()
    tag = "population/" + kind
    out[tag + "/members"] = pop.members.cpu().numpy()
    out[tag + "/act/mu"], out[tag + "/act/action"] = r["mu"].cpu().numpy(), r["action"].cpu().numpy()
    fit, ends = pop.rollout(3)
    torch.cuda.synchronize()
    out[tag + "/rollout/action"] = pop.actions.cpu().numpy()
    out[tag + "/rollout/fit"], out[tag + "/rollout/ends"] = pop.fit.cpu().numpy(), pop.ends.cpu().numpy()
    out[tag + "/rollout/member_fit"], out[tag + "/rollout/member_ends"] = fit.cpu().numpy(), ends.cpu().numpy()
    out[tag + "/rollout/obs"] = env.obs.cpu().numpy()
    env.close()


def _stacked(out, kind, frames):
    """auv_policy_rollout_stacked (4 steps plus flush, host-named counters) and auv_policy_act_stacked (device counters); episodes of 5
    steps end inside the window"""
    import torch
    from gym_auv_amd import _capi
    from gym_auv_amd.batched_env import _LIB
    T = 4
    for how in ("rollout", "act"):
        env = _env(kind)
        fused = _fused(env, T, frames=frames)
        if frames > 1:
            sios = fused._sios
        else:                                                  # frames == 1 through the stacked entry points: hist and stk NULL
            sios = (_capi.AuvPolicyStack * 1)()
            sios[0].io, sios[0].hist, sios[0].stk, sios[0].frames = fused._ios[0], None, None, 1
        fused.begin_rollout()
        if how == "rollout":
            t0, g0 = (C.c_int64 * 1)(fused._t[0]), (C.c_int64 * 1)(fused._g[0])
            _check(_LIB, _entry(_LIB, "auv_policy_rollout_stacked", fused)(env._h, 1, env._bounds_c, env._streams_c, sios, C.c_void_p(env.obs.data_ptr()),
                                                         C.c_void_p(env.reward.data_ptr()), C.c_void_p(env.done.data_ptr()), T, 1, t0, g0))
        else:
            st = C.c_void_p(env._sub_streams[0].cuda_stream)
            for _ in range(T):
                _check(_LIB, _entry(_LIB, "auv_policy_act_stacked", fused)(env._h, 0, N, C.byref(sios[0]), st))
                env.step_slice(0, fused.actions)
            _check(_LIB, _entry(_LIB, "auv_policy_act_stacked", fused)(env._h, 0, N, C.byref(sios[0]), st))
        _keep(out, "stacked/%s/f%d/%s" % (kind, frames, how), fused, env)
        if how == "rollout":
            assert float(fused.buffers()[5].sum()) > 0, "no episode ended inside the window"
        env.close()


def run(path, hidden):
    global HIDDEN
    from gym_auv_amd import _capi
    from gym_auv_amd.policy import check_hidden
    HIDDEN = check_hidden(hidden, "--hidden")
    default = HIDDEN == _capi.POLICY_ARCHS[0]
    lib_path = os.environ.get("AUV_HIP_LIB") or _capi.LIB_PATH
    out = {}
    for kind in WIDTHS:
        _policy(out, kind, False)
        if default:
            _population(out, kind)
        for frames in (1, 3):
            _stacked(out, kind, frames)
    if default:
        _policy(out, "d15", True)
    np.savez(path, **out)
    print("%s: hidden %s, %d arrays, library %s sha256 %s" % (path, list(HIDDEN), len(out), lib_path, hashlib.sha256(open(lib_path, "rb").read()).hexdigest()))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            bad.append(k)
    print("%d arrays in %s, %d in %s: %s" % (len(a.files), pa, len(b.files), pb, "all equal bit for bit" if not bad else "DIFFERENT: " + ", ".join(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2], HIDDEN)
    elif len(sys.argv) == 5 and sys.argv[1] == "run" and sys.argv[3] == "--hidden":
        run(sys.argv[2], tuple(int(x) for x in sys.argv[4].split(",")))
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
