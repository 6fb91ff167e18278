"""-m gpu: what an act launch does behind its matrix chains -- the Gaussian draw, the sample, log pi, the action map, the stored
transition (csrc/auv_policy_forward.h: pol_gauss, pol_act_sample, pol_logp, pol_act_map, pol_act_end) -- and the advantage kernel
(k6_gae in csrc/k6_policy.hip) against the float64 mirrors of gym_auv_amd/policy.py, within the bounds recorded in
tests/golden/policy_epilogue_bounds.json (derived in tests/policy_epilogue_cases.py from the float32 restatement; tests/test_policy_epilogue.py
shows what they catch).  Wherever the epilogue needs mu the launch's own mu_out is used: the matrix chains are not under test here.

The environment is the one of tests/test_gpu_normalize.py: N = 40 as the slices [0, 24) and [24, 40) on two streams (the first ends in a
ragged tile of 8), T = 3, max_timesteps = 5 with the odd environments three steps in, so episodes end inside the rollouts."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gym_auv_amd import policy as P

import policy_epilogue_cases as cases
import test_gpu_normalize as tn

pytestmark = pytest.mark.gpu
DEV = tn.DEV
N, T, SLICES = cases.N, cases.T, cases.SLICES
assert (tn.N, tn.T, tn.SLICES) == (N, T, SLICES)
CASES = [(186, (256, 128, 64)), (15, (64, 64, 64))]
MAP = dict(act_half=(0.5, 0.25), act_mid=(0.25, -0.125), clip_lo=(-0.25, -0.5), clip_hi=(0.25, 0.5))
SCALE = 0.37
CANARY = 77.0
f32, f64 = np.float32, np.float64


def _np(t):
    return t.detach().cpu().numpy()


def _fused(env, hidden, log_std=cases.LOG_STDS[0], seed=cases.SEED, rollout=T, **kw):
    net = tn._net(env.obs_dim, hidden, seed)
    with torch.no_grad():
        net.log_std.copy_(torch.tensor(log_std))
    return P.FusedActorCritic(net, env, rollout=rollout, debug=True, seed=seed, **kw)


def _mirror_eps(seed, i, step, dtype=f64):
    """eps [cnt, 2] of chain i's launch at generator step `step`: keyed by the GLOBAL environment index."""
    lo, cnt = SLICES[i]
    return P.policy_noise(P.chain_seed(seed, i), step, lo + np.arange(cnt)[:, None], np.arange(2)[None, :], dtype)


class Run:
    """Two rollouts of T steps back to back, launch by launch (act + step_slice on both slices, then the flush launches), with everything
    a launch saw and left: per sampling launch the chains' generator steps, eps, mu and the action buffer; per launch the raw reward and
    done it was to store; per rollout the buffers behind the flush."""

    def __init__(self, obs_dim, hidden, log_std, reward_clip, custom_map):
        self.env = env = tn._env(obs_dim)
        self.fused = fused = _fused(env, hidden, log_std, reward_scale=SCALE, reward_clip=reward_clip, **(MAP if custom_map else {}))
        self.log_std = _np(fused.net.log_std).astype(f32)
        self.steps, self.eps, self.mu, self.actions, self.raw, self.buffers, self.ctr = [], [], [], [], [], [], []
        for r in range(cases.ROLLOUTS):
            fused.begin_rollout()
            raw = []
            for t in range(T + 1):
                torch.cuda.synchronize()
                raw.append((_np(env.reward).copy(), _np(env.done).copy()))
                steps = list(fused._g)
                before = fused.eps.clone()
                for i in range(2):
                    fused.act(i)
                torch.cuda.synchronize()
                self.ctr.append([_np(b["ctr"]).copy() for b in fused.buf])
                if t == T:
                    assert torch.equal(fused.eps, before)          # the flush launch samples nothing
                    break
                self.steps.append(steps)
                self.eps.append(_np(fused.eps).copy()), self.mu.append(_np(fused.mu).copy()), self.actions.append(_np(fused.actions).copy())
                for i in range(2):
                    env.step_slice(i, fused.actions)
            self.raw.append(raw)
            self.buffers.append([_np(x).copy() for x in (fused.A, fused.LP, fused.V, fused.R, fused.Dn)])


@functools.lru_cache(maxsize=None)
def _run_cached(obs_dim, hidden, log_std, reward_clip, custom_map):
    return Run(obs_dim, hidden, log_std, reward_clip, custom_map)


def _run(obs_dim, hidden, log_std=cases.LOG_STDS[0], reward_clip=0.0, custom_map=False):
    return _run_cached(obs_dim, tuple(hidden), tuple(log_std), float(reward_clip), bool(custom_map))


def _launches(run):
    """(k, r, t) of the sampling launches: k counts them, r the rollout, t the position in it."""
    return [(r * T + t, r, t) for r in range(cases.ROLLOUTS) for t in range(T)]


# ------------------------------------------------------------------------------ a. the draw
@pytest.mark.parametrize("obs_dim,hidden", CASES)
def test_every_draw_is_the_mirror_of_its_seed_step_environment_and_component(obs_dim, hidden):
    bound = cases.recorded_bound("eps")
    run = _run(obs_dim, hidden)
    ref = cases.noise_inputs(f64)[0]
    worst = 0.0
    for k, r, t in _launches(run):
        # the launches so far on either chain: the first rollout's flush counted, nothing reset by begin_rollout
        assert run.steps[k] == [cases.SAMPLE_STEPS[k]] * 2 == [r * (T + 1) + t] * 2
        want = np.concatenate([_mirror_eps(cases.SEED, i, run.steps[k][i]) for i in range(2)])
        assert np.array_equal(want, ref[k])                        # (the inputs the bound was derived on)
        assert np.isfinite(run.eps[k]).all()
        worst = max(worst, float(np.abs(run.eps[k].astype(f64) - want).max()))
    for j, c in enumerate(run.ctr):                                # device counters: t moves to T + 1 and back to 0, the step never back
        assert [int(x[1]) for x in c] == [j + 1] * 2 and [int(x[0]) for x in c] == [j % (T + 1) + 1] * 2 and [int(x[2]) for x in c] == [0, 0]
    print("eps: device - float64 %.3g, bound %.3g" % (worst, bound))
    assert worst <= bound
    # another seed: other draws, the mirror's
    env = tn._env(obs_dim)
    other = _fused(env, hidden, seed=cases.OTHER_SEED)
    other.begin_rollout()
    for i in range(2):
        other.act(i)
    torch.cuda.synchronize()
    got = _np(other.eps).astype(f64)
    want = np.concatenate([_mirror_eps(cases.OTHER_SEED, i, 0) for i in range(2)])
    assert (got != run.eps[0]).all() and float(np.abs(got - want).max()) <= bound
    env.close()
    # far out in the tail: the step below 2^16 at which chain 0 draws its smallest u1 over its 24 environments and both components
    # (searched here on the CPU; the bounds file records the same step)
    i = cases.SEARCH_CHAIN
    lo, cnt = SLICES[i]
    u1, _ = P.policy_noise_fields(P.chain_seed(cases.SEED, i), np.arange(1 << 16)[:, None, None], lo + np.arange(cnt)[None, :, None],
                                  np.arange(2)[None, None, :])
    step = int(np.argmin(u1.reshape(1 << 16, -1).min(axis=1)))
    assert float(u1[step].min()) < 2.0 ** -20 and (step, float(u1[step].min())) == cases.searched_step()
    fused = run.fused
    fused.begin_rollout()
    with torch.cuda.stream(run.env._sub_streams[i]):
        fused.buf[i]["ctr"][1] = step
    fused._g[i] = step
    fused.eps.fill_(CANARY)
    torch.cuda.synchronize()
    fused.act(i)
    torch.cuda.synchronize()
    got = _np(fused.eps)
    want = _mirror_eps(cases.SEED, i, step)
    d = float(np.abs(got[lo:lo + cnt].astype(f64) - want).max())
    print("eps at step %d (u1 = %.3g, |eps| up to %.3f): device - float64 %.3g, bound %.3g" % (step, u1[step].min(), np.abs(want).max(), d, bound))
    assert np.isfinite(got).all() and d <= bound and (got[lo + cnt:] == CANARY).all()
    assert int(fused.buf[i]["ctr"][1]) == step + 1


# ------------------------------------------------------------------------------ b. sample and log-probability
@pytest.mark.parametrize("log_std", cases.LOG_STDS)
@pytest.mark.parametrize("obs_dim,hidden", CASES)
def test_sample_and_log_probability_against_float64_on_the_launches_own_mu_and_eps(obs_dim, hidden, log_std):
    run = _run(obs_dim, hidden, log_std, 0.0, log_std == cases.LOG_STDS[1])
    ba, bl = cases.recorded_bound("A", log_std), cases.recorded_bound("LP", log_std)
    assert np.array_equal(run.log_std, np.array(log_std, dtype=f32))
    da = dl = 0.0
    for k, r, t in _launches(run):
        A, LP = run.buffers[r][0][t], run.buffers[r][1][t]
        da = max(da, float(np.abs(A.astype(f64) - P.sample_reference(run.mu[k], run.log_std, run.eps[k])).max()))
        dl = max(dl, float(np.abs(LP.astype(f64) - P.logp_reference(A, run.mu[k], run.log_std)).max()))
        assert np.isfinite(A).all() and np.isfinite(LP).all()
    print("log_std %s: A device - float64 %.3g (bound %.3g), LP %.3g (bound %.3g)" % (log_std, da, ba, dl, bl))
    assert da <= ba and dl <= bl


# ------------------------------------------------------------------------------ c. a non-default action map
@pytest.mark.parametrize("obs_dim,hidden", CASES)
def test_a_map_that_differs_per_component_is_applied_bit_for_bit(obs_dim, hidden):
    run = _run(obs_dim, hidden, cases.LOG_STDS[1], 0.0, True)
    assert run.fused.action_map == (MAP["act_mid"], MAP["act_half"], MAP["clip_lo"], MAP["clip_hi"])
    lo_hit, hi_hit, inside = np.zeros(2, int), np.zeros(2, int), np.zeros(2, int)
    for k, r, t in _launches(run):
        A = run.buffers[r][0][t]
        want = P.action_map_reference(A, MAP["act_mid"], MAP["act_half"], MAP["clip_lo"], MAP["clip_hi"])
        assert np.array_equal(run.actions[k], want), k
        # the power-of-two halves make mid + half * clamp one rounding: the float64 statement gives the same bits
        c = np.minimum(np.maximum(A.astype(f64), MAP["clip_lo"]), MAP["clip_hi"])
        assert np.array_equal(want, (np.array(MAP["act_mid"]) + np.array(MAP["act_half"]) * c).astype(f32))
        lo_hit += (A < np.array(MAP["clip_lo"], f32)).sum(0)
        hi_hit += (A > np.array(MAP["clip_hi"], f32)).sum(0)
        inside += ((A > np.array(MAP["clip_lo"], f32)) & (A < np.array(MAP["clip_hi"], f32))).sum(0)
        # with the components' maps exchanged the buffer would hold something else
        assert not np.array_equal(run.actions[k], P.action_map_reference(A, *[MAP[n][::-1] for n in ("act_mid", "act_half", "clip_lo", "clip_hi")]))
    print("clip_lo hit %s, clip_hi hit %s, inside %s" % (lo_hit, hi_hit, inside))
    assert (lo_hit > 0).all() and (hi_hit > 0).all() and (inside > 0).all()


# ------------------------------------------------------------------------------ d. the stored transition
def _check_transition(run, clip):
    clipped = kept = dones = 0
    for r in range(cases.ROLLOUTS):
        R, Dn = run.buffers[r][3], run.buffers[r][4]
        for t in range(1, T + 1):                                  # (t = T: the flush launch stores row T - 1)
            rew, done = run.raw[r][t]
            c = rew if clip == 0.0 else np.minimum(np.maximum(rew, f32(-clip)), f32(clip))
            want = c * f32(SCALE)
            assert want.dtype == f32 and np.array_equal(R[t - 1], want), (r, t)
            assert np.array_equal(Dn[t - 1], (done != 0).astype(f32)), (r, t)
            clipped += int((np.abs(rew) > f32(clip)).sum()) if clip else 0
            kept += int((np.abs(rew) < f32(clip)).sum()) if clip else rew.size
            dones += int((done != 0).sum())
    return clipped, kept, dones


@pytest.mark.parametrize("obs_dim,hidden", CASES)
def test_reward_scale_and_clip_and_done_are_stored_bit_for_bit(obs_dim, hidden):
    free = _run(obs_dim, hidden)                                   # reward_clip = 0: the clip is off
    assert free.fused._ios[0].reward_clip == 0.0
    clipped, kept, dones = _check_transition(free, 0.0)
    assert dones > 0 and dones < kept                              # episodes ended inside the rollouts, and not everywhere
    # the same run with a clip inside the rewards it saw: their median magnitude
    mags = np.abs(np.concatenate([free.raw[r][t][0] for r in range(cases.ROLLOUTS) for t in range(1, T + 1)]))
    clip = float(f32(np.median(mags)))
    assert clip > 0.0
    run = _run(obs_dim, hidden, cases.LOG_STDS[0], clip, False)
    for r in range(cases.ROLLOUTS):
        for t in range(T + 1):
            assert np.array_equal(run.raw[r][t][0], free.raw[r][t][0]) and np.array_equal(run.raw[r][t][1], free.raw[r][t][1])
    clipped, kept, dones = _check_transition(run, clip)
    print("reward_clip %.6g: %d rows clipped, %d kept, %d dones; |reward| %.3g .. %.3g" % (clip, clipped, kept, dones, mags.min(), mags.max()))
    assert clipped > 0 and kept > 0
    assert not np.array_equal(run.buffers[0][3], free.buffers[0][3])


# ------------------------------------------------------------------------------ e. what a launch leaves alone
@pytest.mark.parametrize("obs_dim,hidden", CASES)
def test_a_launch_writes_its_slice_and_its_row_and_nothing_behind_the_flush(obs_dim, hidden):
    env = tn._env(obs_dim)
    fused = _fused(env, hidden, reward_scale=SCALE)
    names = ("A", "LP", "V", "R", "Dn", "actions", "mu", "eps")
    bufs = [getattr(fused, n) for n in names]
    for b in bufs:
        b.fill_(CANARY)
    lo1 = SLICES[1][0]
    fused.begin_rollout()
    torch.cuda.synchronize()
    fused.act(0)
    torch.cuda.synchronize()
    for n, b in zip(names, bufs):
        x = _np(b)
        if n in ("R", "Dn"):
            assert (x == CANARY).all(), n                          # no transition is complete at t = 0
        elif n in ("A", "LP", "V"):
            assert (x[0, :lo1] != CANARY).all() and (x[0, lo1:] == CANARY).all() and (x[1:] == CANARY).all(), n
        else:
            assert (x[:lo1] != CANARY).all() and (x[lo1:] == CANARY).all(), n
    env.step_slice(0, fused.actions)
    fused.act(0)                                                   # t = 1 on chain 0: rows 1 of A, LP, V, row 0 of R, Dn
    torch.cuda.synchronize()
    keep0 = _np(fused.A)[0].copy()
    for n in ("A", "LP", "V", "R", "Dn"):
        x = _np(getattr(fused, n))
        rows = (0, 1) if n in ("A", "LP", "V") else (0,)
        for t in range(T):
            assert (x[t, lo1:] == CANARY).all(), (n, t)
            assert (x[t, :lo1] != CANARY).all() if t in rows else (x[t, :lo1] == CANARY).all(), (n, t)
    assert np.array_equal(_np(fused.A)[0], keep0) and (_np(fused.actions)[lo1:] == CANARY).all()
    # the rest of the rollout on both chains, through the flush
    env.step_slice(0, fused.actions)
    fused.act(0)
    for t in range(T):
        fused.act(1)
        env.step_slice(1, fused.actions)
    env.step_slice(0, fused.actions)
    for i in range(2):
        fused.act(i)
    torch.cuda.synchronize()
    for n in ("A", "LP", "V", "R", "Dn"):
        assert (_np(getattr(fused, n)) != CANARY).all(), n
    assert [int(b["ctr"][0]) for b in fused.buf] == [T + 1] * 2 and [int(b["ctr"][1]) for b in fused.buf] == [T + 1] * 2
    keep = [b.clone() for b in bufs]
    for i in range(2):
        fused.act(i)                                               # behind the flush: nothing is written, only the generator moves on
    torch.cuda.synchronize()
    for n, a, b in zip(names, keep, bufs):
        assert torch.equal(a, b), n
    assert [int(b["ctr"][0]) for b in fused.buf] == [T + 1] * 2 and [int(b["ctr"][1]) for b in fused.buf] == [T + 2] * 2
    env.close()


# ------------------------------------------------------------------------------ f. the advantage kernel
def _gae_env(n):
    import warnings
    from gym_auv_amd.batched_env import BatchedAuvEnv
    from gym_auv_amd.config import effective_reference_config
    cfg = effective_reference_config(use_lidar=True)
    cfg.vessel.sensor_use_feasibility_pooling = True
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = BatchedAuvEnv(cfg, tn._bank(), n, device=DEV, rewarder="colav")
    env.reset()
    env.set_sub_batches(1, probe_streams=False)
    torch.cuda.synchronize()
    return env


def _gae_call(env, R, V, Dn, last_v, gamma, lam, Tn, Nn, pad=64):
    """auv_gae on the caller's tensors into buffers `pad` floats longer than T * N, canary-filled: (adv, ret) [T, N] as NumPy."""
    adv = torch.full((Tn * Nn + pad,), CANARY, dtype=torch.float32, device=DEV)
    ret = torch.full((Tn * Nn + pad,), CANARY, dtype=torch.float32, device=DEV)
    lib = tn._lib()
    rc = lib.auv_gae(env._h, tn._p(R), tn._p(V), tn._p(Dn), tn._p(last_v), gamma, lam, tn._p(adv), tn._p(ret), Tn, Nn,
                     C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0, lib.auv_last_error()
    torch.cuda.synchronize()
    a, r = _np(adv), _np(ret)
    assert (a[Tn * Nn:] == CANARY).all() and (r[Tn * Nn:] == CANARY).all()
    return a[:Tn * Nn].reshape(Tn, Nn).copy(), r[:Tn * Nn].reshape(Tn, Nn).copy()


@pytest.mark.parametrize("Tn,Nn", cases.GAE_SHAPES)
def test_gae_against_float64_at_block_edges_extreme_parameters_and_forced_dones(Tn, Nn):
    env = _gae_env(Nn)
    fused = _fused(env, (64, 64, 64), rollout=Tn, store_obs=False)
    dev = lambda x: torch.as_tensor(x, device=DEV)                 # noqa: E731
    for gamma, lam in cases.GAE_PARAMS:
        for dones in cases.GAE_DONES:
            bound = cases.recorded_gae_bound(Tn, Nn, gamma, lam, dones)
            R, V, Dn, last_v = cases.gae_inputs(Tn, Nn, dones)
            if dones == "random" and Nn > 2:
                assert Dn[Tn - 1, 1] == 1.0 and Dn[0, 2] == 1.0
            Rd, Vd, Dd, Ld = dev(R), dev(V), dev(Dn), dev(last_v)
            adv, ret = _gae_call(env, Rd, Vd, Dd, Ld, gamma, lam, Tn, Nn)
            want = P.gae_reference(R, V, Dn, last_v, gamma, lam)[0]
            d = float(np.abs(adv.astype(f64) - want).max())
            print("T %d N %d gamma %g lam %g dones %s: device - float64 %.3g, bound %.3g" % (Tn, Nn, gamma, lam, dones, d, bound))
            assert np.isfinite(adv).all() and d <= bound, (gamma, lam, dones)
            assert np.array_equal(ret, adv + V), (gamma, lam, dones)                       # one float32 addition
            m = Dn == 1.0
            assert np.array_equal(adv[m], (R - V)[m]), (gamma, lam, dones)                 # the masked terms are exact zeros
            # a rerun gives the same bits
            adv2, ret2 = _gae_call(env, Rd, Vd, Dd, Ld, gamma, lam, Tn, Nn)
            assert np.array_equal(adv, adv2) and np.array_equal(ret, ret2)
            # another environment's inputs move that environment's column only
            c = min(3, Nn - 1)
            R1, V1, Dn1, L1 = R.copy(), V.copy(), Dn.copy(), last_v.copy()
            R1[:, c] += f32(1.0)
            V1[:, c] *= f32(0.5)
            Dn1[:, c] = f32(1.0) - Dn1[:, c]
            L1[c] += f32(1.0)
            adv1, ret1 = _gae_call(env, dev(R1), dev(V1), dev(Dn1), dev(L1), gamma, lam, Tn, Nn)
            keep = np.arange(Nn) != c
            assert np.array_equal(adv1[:, keep], adv[:, keep]) and np.array_equal(ret1[:, keep], ret[:, keep])
            assert not np.array_equal(adv1[:, c], adv[:, c]) and not np.array_equal(ret1[:, c], ret[:, c])
            # FusedActorCritic.gae on the same data: the same bits
            fused.R.copy_(Rd), fused.Dn.copy_(Dd)
            a3, r3 = fused.gae(Vd, Ld, gamma, lam)
            torch.cuda.synchronize()
            assert a3.shape == (Tn, Nn) and np.array_equal(_np(a3), adv) and np.array_equal(_np(r3), ret)
    env.close()
