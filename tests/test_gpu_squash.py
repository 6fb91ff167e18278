"""-m gpu: the tanh-squashed policy through the C ABI -- auv_policy_act_squash / _rollout_squash / _eval_squash (csrc/k17_policy_squash.hip)
against the plain launches bit for bit and against policy.squash_map_reference in float64; auv_ppo_grad_squash (the squash head of
csrc/auv_ppo_pass.h) against fp64 autograd of ppo_update.squash_loss_terms and, at ent_coef = 0, against auv_ppo_grad bit for bit.

Bounds: tests/golden/squash_bounds.json, derived on the CPU in tests/squash_cases.py from the float32 mirrors (8 x their error against
float64, floors 4 ulp32(|half|) and 1e-5) and held to them by tests/test_squash.py; the update's nets and batches are the ones built
there, moved to the device.

Shapes: act -- 33 environments as the slices [0, 17) (a full tile and one ragged row) and [17, 33) (one full tile); rollout -- 48 as two
chains of 24, T = 3, episodes of 5 steps with the odd environments three steps in; obs_dim 186 and the pooled 15."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

from gym_auv_amd import policy as P

import squash_cases as cases
import test_gpu_normalize as tn

pytestmark = pytest.mark.gpu
DEV = tn.DEV
T = 3
f32, f64 = np.float32, np.float64
MAP = dict(act_mid=cases.MAP_MID, act_half=cases.MAP_HALF)
PLAIN_CLIP = dict(clip_lo=(-0.25, -0.5), clip_hi=(0.25, 0.5))
OBS_DIMS = [15, 186]


def _np(t):
    return t.detach().cpu().numpy()


def _env(obs_dim, slices):
    """tests/test_gpu_normalize.py's environment with another number of environments and other slices."""
    from gym_auv_amd.batched_env import BatchedAuvEnv
    from gym_auv_amd.config import effective_reference_config
    n = slices[-1][0] + slices[-1][1]
    cfg = effective_reference_config(use_lidar=True)
    cfg.episode.max_timesteps = tn.MAX_T
    cfg.vessel.sensor_use_feasibility_pooling = obs_dim == 15
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # (16 worlds for a few dozen auto-resetting environments: fine here)
        env = BatchedAuvEnv(cfg, tn._bank(), n, device=DEV, rewarder="colav")
    assert env.obs_dim == obs_dim
    env.set_step_mode("side_by_side")
    env.reset()
    zero = torch.zeros((n, 2), dtype=torch.float32, device=DEV)
    for _ in range(3):
        env.step(zero)
    mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
    mask[0::2] = 1
    env.reset(mask)
    env.set_sub_batches(1, probe_streams=False)
    streams = [torch.cuda.Stream(device=DEV) for _ in slices]
    env._slices, env.sub_batches, env._sub_streams = list(slices), len(slices), streams
    env._bounds_c = (C.c_int32 * (len(slices) + 1))(*([s[0] for s in slices] + [n]))
    env._streams_c = (C.c_void_p * len(slices))(*[s.cuda_stream for s in streams])
    torch.cuda.synchronize()
    return env


ACT_SLICES = [(0, 17), (17, 16)]


@functools.lru_cache(maxsize=None)
def _act_env(obs_dim):
    return _env(obs_dim, ACT_SLICES)                       # shared by the act tests: they launch the policy and never step it


def _fused(env, hidden, squash, log_std=None, **kw):
    net = tn._net(env.obs_dim, hidden, 5)
    if log_std is not None:
        with torch.no_grad():
            net.log_std.copy_(torch.tensor(log_std))
    extra = dict(MAP) if squash else dict(MAP, **PLAIN_CLIP)
    extra.update(kw)
    return P.FusedActorCritic(net, env, rollout=T, debug=True, seed=5, reward_scale=0.37, reward_clip=50.0, squash=squash, **extra)


def _act_twice(fused):
    """t = 0 and t = 1 on both slices without a step in between: the second launch also stores a transition."""
    fused.begin_rollout()
    for _ in range(2):
        for i in range(len(fused.slices)):
            fused.act(i)
    torch.cuda.synchronize()
    out = {n: getattr(fused, n).clone() for n in ("O", "A", "LP", "V", "R", "Dn", "mu", "eps", "actions")}
    out["ctr"] = torch.stack([b["ctr"] for b in fused.buf])
    return out


def _check_actions(actions, A, what):
    """actions_out against the float64 mirror on the launch's own stored A, per component within the recorded bound."""
    bound = cases.recorded()["actions"]["bound"]
    want = P.squash_map_reference(_np(A).astype(f64), cases.MAP_MID, cases.MAP_HALF, f64)
    d = np.abs(_np(actions).astype(f64) - want).max(axis=0)
    print("%s: actions_out - float64 mirror %s, bounds %s" % (what, d, bound))
    assert np.isfinite(_np(actions)).all() and (d <= np.array(bound)).all(), (what, d, bound)


# ------------------------------------------------------------------------------ 1. the act launch against the plain one
@pytest.mark.parametrize("obs_dim", OBS_DIMS)
@pytest.mark.parametrize("hidden", cases.HIDDEN)
def test_act_launch_stores_what_the_plain_launch_stores_and_squashes_the_action(hidden, obs_dim):
    env = _act_env(obs_dim)
    plain, squashed = _act_twice(_fused(env, hidden, False)), _act_twice(_fused(env, hidden, True))
    for name in ("O", "A", "LP", "V", "R", "Dn", "mu", "eps", "ctr"):
        assert torch.equal(plain[name], squashed[name]), name
    assert [int(x) for x in squashed["ctr"][0][:3]] == [2, 2, 0] and bool(squashed["R"][0].any())
    A = squashed["A"][1]                                   # (the launch at t = 1 wrote the action buffer last)
    assert not torch.equal(A, squashed["mu"]) and bool(torch.isfinite(A).all())
    _check_actions(squashed["actions"], A, "hidden %s obs_dim %d" % (hidden, obs_dim))
    assert not torch.equal(squashed["actions"], plain["actions"])
    # with the components' maps exchanged the buffer would hold something else
    swapped = P.squash_map_reference(_np(A), cases.MAP_MID[::-1], cases.MAP_HALF[::-1], f64)
    assert np.abs(_np(squashed["actions"]) - swapped).max() > 1e-3


# ------------------------------------------------------------------------------ 2. saturation
@pytest.mark.parametrize("bias,log_std", [((25.0, -25.0), (-20.0, -20.0)), ((90.0, -90.0), (-20.0, -20.0)), ((25.0, -90.0), (3.0, 3.0)),
                                          ((-25.0, 90.0), (3.0, -20.0))])
def test_saturated_samples_give_the_edge_of_the_box_exactly_and_never_nan(bias, log_std):
    env = _act_env(15)
    fused = _fused(env, (64, 64, 64), True, log_std=log_std)
    with torch.no_grad():
        fused.net.pi[-1].weight.zero_()                    # mu is the last bias, exactly
        fused.net.pi[-1].bias.copy_(torch.tensor(bias))
    fused.refresh()
    out = _act_twice(fused)
    assert torch.equal(out["mu"], torch.tensor(bias, device=DEV).expand_as(out["mu"]))
    A, act = _np(out["A"][1]), _np(out["actions"])
    for name in ("A", "LP", "V", "actions", "eps"):
        assert bool(torch.isfinite(out[name]).all()), name
    mid, half = np.array(cases.MAP_MID, f32), np.array(cases.MAP_HALF, f32)
    lo, hi = mid - np.abs(half), mid + np.abs(half)
    assert (act >= lo).all() and (act <= hi).all()
    far = np.abs(A) >= 20.0
    assert far.any() and (log_std[0] < 0 or not far.all())
    edge = np.where(A > 0, mid + half, mid - half).astype(f32)
    assert np.array_equal(act[far], edge[far])
    _check_actions(out["actions"], out["A"][1], "bias %s log_std %s" % (bias, log_std))


# ------------------------------------------------------------------------------ 3. the rollout call
@pytest.mark.parametrize("obs_dim,hidden", [(186, (256, 128, 64)), (15, (64, 64, 64)), (15, (128, 64, 64))])
def test_rollout_call_is_the_loop_of_act_launches_and_steps(obs_dim, hidden):
    slices = [(0, 24), (24, 24)]
    env = _env(obs_dim, slices)
    fused = _fused(env, hidden, True)
    fused.begin_rollout()
    seen = []
    for t in range(T):
        for i in range(2):
            fused.act(i)                                   # (the device-counter form)
        torch.cuda.synchronize()
        seen.append((fused.actions.clone(), fused.A[t].clone()))
        for i in range(2):
            env.step_slice(i, fused.actions)
    for i in range(2):
        fused.act(i)                                       # the flush launch
    torch.cuda.synchronize()
    want = [x.clone() for x in fused.buffers()] + [env.obs.clone(), env.reward.clone(), env.done.clone()]
    ctr = [b["ctr"].clone() for b in fused.buf]
    env.close()
    env2 = _env(obs_dim, slices)
    f2 = _fused(env2, hidden, True)
    f2.begin_rollout()
    f2.rollout(T, flush=True)                              # (host-named counters, the flush inside the call)
    torch.cuda.synchronize()
    got = [x.clone() for x in f2.buffers()] + [env2.obs.clone(), env2.reward.clone(), env2.done.clone()]
    for x, y, name in zip(want, got, ("O", "A", "LP", "V", "R", "Dn", "obs", "reward", "done")):
        assert torch.equal(x, y), name
    for i in range(2):
        assert torch.equal(ctr[i][:3], f2.buf[i]["ctr"][:3]) and int(ctr[i][0]) == T + 1
    assert bool(want[5].any())                             # episodes did end inside the rollout
    for act, A in seen:
        _check_actions(act, A, "rollout step")
    env2.close()


# ------------------------------------------------------------------------------ 4. the eval launch
@pytest.mark.parametrize("obs_dim", OBS_DIMS)
@pytest.mark.parametrize("hidden", cases.HIDDEN)
def test_eval_squashes_the_mean_as_the_act_launch_would_and_leaves_mean_and_value_alone(hidden, obs_dim):
    env = _act_env(obs_dim)
    # sigma = exp(-200) is zero in float32: the act launch then samples a = mu exactly and maps that
    fused = _fused(env, hidden, True, log_std=(-200.0, -200.0))
    out = _act_twice(fused)
    assert torch.equal(out["A"][1], out["mu"])
    act = fused.predict(env.obs, out=torch.empty_like(fused.actions))
    r = P.policy_eval(fused.params, fused.in_dim, env.obs, want=("mu", "value", "action"), action_map=fused.action_map, squash=True,
                      hidden=hidden)
    plain = P.policy_eval(fused.params, fused.in_dim, env.obs, want=("mu", "value"), hidden=hidden)
    torch.cuda.synchronize()
    assert torch.equal(act, out["actions"]) and torch.equal(r["action"], out["actions"])
    assert torch.equal(r["mu"], plain["mu"]) and torch.equal(r["value"], plain["value"]) and torch.equal(r["mu"], out["mu"])
    assert torch.equal(r["value"], out["V"][1])
    _check_actions(act, r["mu"], "eval hidden %s obs_dim %d" % (hidden, obs_dim))
    # log pi of pre-squash actions: the plain entry's bits
    other = _act_twice(_fused(env, hidden, True))
    lp, v, mu = _fused(env, hidden, True).evaluate(other["O"][1], other["A"][1])
    torch.cuda.synchronize()
    assert torch.equal(lp, other["LP"][1]) and torch.equal(v, other["V"][1])


# ------------------------------------------------------------------------------ 5. / 6. the update
@functools.lru_cache(maxsize=None)
def _rows(hidden, saturated):
    return cases.make_rows(cases.UPDATE_OBS_DIM, hidden, saturated=saturated)      # CPU float32, shared, never modified


def _updater(hidden, ent_coef, squash=True):
    from gym_auv_amd.ppo_update import FusedPPOUpdate
    net = cases.make_net(cases.UPDATE_OBS_DIM, hidden, dtype=torch.float32).to(DEV)
    return FusedPPOUpdate(net, clip=cases.CLIP, vf_coef=cases.VF_COEF, ent_coef=ent_coef, max_batch=512, squash=squash)


def _grad(upd, rows, idx, B):
    dev = [x.to(DEV).contiguous() for x in rows]
    g, s = upd.grad(*dev, idx=None if idx is None else idx.to(DEV), B=B)
    torch.cuda.synchronize()
    return g.clone(), s.clone()


@pytest.mark.parametrize("ent_coef", cases.ENT_COEFS)
@pytest.mark.parametrize("hidden", cases.HIDDEN)
def test_squash_gradient_and_statistics_against_fp64_autograd(hidden, ent_coef):
    key = "update/%d-%d-%d/ent%g" % (hidden + (ent_coef,))
    bounds = cases.recorded()["update"]
    upd = _updater(hidden, ent_coef)
    plain = _updater(hidden, ent_coef, squash=False) if ent_coef == 0.0 else None
    for k, h, B, form, e, sat in cases.update_cases():
        if h != hidden or e != ent_coef:
            continue
        assert k == (key + "/saturated" if sat else key)
        rows, idx = _rows(hidden, sat), cases.make_index(B, form)
        g, s = _grad(upd, rows, idx, B)
        g_ref, s_ref = cases.reference(cases.UPDATE_OBS_DIM, hidden, rows, idx, B, ent_coef)
        dg = float((g.double().cpu() - g_ref).abs().max())
        ds = float((s.double().cpu() - s_ref).abs().max())
        print("%s B %d idx %s: grad - fp64 %.3g (bound %.3g), stats - fp64 %.3g (bound %.3g), entropy %.6g, d log_std %s"
              % (k, B, form, dg, bounds[k]["bound_grad"], ds, bounds[k]["bound_stats"], float(s[7]), g[-2:].tolist()))
        assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(s).all())
        assert float(s[5]) == 0.0                          # no non-finite input
        assert dg <= bounds[k]["bound_grad"] and ds <= bounds[k]["bound_stats"], (k, B, form, dg, ds)
        # the same call again: the same bits
        g2, s2 = _grad(upd, rows, idx, B)
        assert torch.equal(g, g2) and torch.equal(s, s2)
        if plain is not None:
            gp, sp = _grad(plain, rows, idx, B)
            assert torch.equal(g, gp), (k, B, form)        # without the entropy term: auv_ppo_grad's bits
            assert torch.equal(s[:7], sp[:7]) and float(sp[7]) == 0.0 and float(s[7]) != 0.0
        if sat:
            assert float(s[7]) < -40.0                     # rows 90 out weigh on the mean entropy: 2 (log 2 - 90) each


def test_a_non_finite_action_counts_as_a_bad_input():
    hidden = (64, 64, 64)
    upd = _updater(hidden, 0.01)
    rows = [x.clone() for x in _rows(hidden, False)]
    rows[1][3, 1] = float("inf")
    g, s = _grad(upd, rows, None, 16)
    assert float(s[5]) == 1.0


@pytest.mark.parametrize("hidden", [(256, 128, 64), (64, 64, 64)])
def test_a_step_reaches_the_attached_squash_policy_as_refresh_would(hidden):
    from gym_auv_amd.ppo_update import FusedPPOUpdate
    env = _act_env(15)
    fused = _fused(env, hidden, True)
    upd = FusedPPOUpdate(fused.net, clip=cases.CLIP, vf_coef=cases.VF_COEF, ent_coef=0.01, max_batch=64, squash=True)
    with pytest.raises(ValueError, match="squash"):
        FusedPPOUpdate(tn._net(15, hidden, 5), max_batch=64, squash=False).attach(fused)
    upd.attach(fused)
    before = _act_twice(fused)
    O, A, LP = before["O"][0].contiguous(), before["A"][0].contiguous(), before["LP"][0].contiguous()
    g = torch.Generator().manual_seed(1)
    ADV, RET = (torch.randn(O.shape[0], generator=g).to(DEV) for _ in range(2))
    p0 = fused.params.clone()
    upd.step(O, A, LP, ADV, RET)
    after = _act_twice(fused)                              # the attached buffer: the updated weights, no refresh()
    packed = fused.params.clone()
    fused.refresh()
    torch.cuda.synchronize()
    assert not torch.equal(p0, packed) and torch.equal(packed, fused.params)
    again = _act_twice(fused)
    assert not torch.equal(before["mu"], after["mu"])
    for name in ("V", "mu"):                               # (the samples differ: the generator's step has moved on)
        assert torch.equal(after[name], again[name]), name
    assert not torch.equal(after["eps"], again["eps"])
    _check_actions(after["actions"], after["A"][1], "after a step")
