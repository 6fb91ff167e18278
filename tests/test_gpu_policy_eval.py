"""-m gpu: the fused actor-critic on arbitrary rows (csrc/k9_policy_eval.hip, auv_policy_eval: FusedActorCritic.predict / value /
evaluate, policy.policy_eval) and the value-terminated planner score (auv_plan_score_v).

Against the rollout launch (csrc/k6_policy.hip) every comparison is BITWISE: the matrix chains are the same code (pol_prefetch /
pol_layer in the same order with the same template arguments) and the epilogue is the same expression on the same floats.  Against
the torch modules the tolerances are those tests/test_gpu_policy.py holds the same chains to: 1e-5 on the means, 1e-5 * max(1, max |v|)
on the values (f32 MFMA chains against f32 GEMMs: same precision, another summation order).  The plan score is bitwise against the
plain float32 loop of its contract."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from gym_auv_amd import planning
from gym_auv_amd.config import effective_reference_config
from gym_auv_amd.policy import SUPPORTED_HIDDEN
from gym_auv_amd.scenarios import moving_obstacles_world
from gym_auv_amd.world import build_world, pack_bank

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
DEV = "cuda:0"
CANARY = -777.25


def _net(obs_dim, seed=0):
    import ppo
    torch.manual_seed(seed)
    net = ppo.ActorCritic(obs_dim).to(DEV)
    with torch.no_grad():
        net.log_std.copy_(torch.tensor([-0.5, -1.1]))
        for m in net.modules():                      # weights of ordinary size, biases that matter
            if isinstance(m, torch.nn.Linear):
                m.bias.uniform_(-0.3, 0.3)
    return net


def _setup(n, k, T, use_lidar=True, seed=0, pooled=False, auto_reset=True, **kw):
    """(the helper of tests/test_gpu_policy.py, plus a feasibility-pooled observation: 6 + 9 sectors = 15 columns)"""
    from gym_auv_amd.batched_env import BatchedAuvEnv
    from gym_auv_amd.policy import FusedActorCritic
    cfg = effective_reference_config(use_lidar=use_lidar)
    cfg.vessel.sensor_use_feasibility_pooling = bool(pooled)
    bank = pack_bank([build_world(moving_obstacles_world(2000 + i) if use_lidar else moving_obstacles_world(2000 + i, 0, 0)) for i in range(16)])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = BatchedAuvEnv(cfg, bank, n, device=DEV, rewarder="colav" if use_lidar else "pathfollow", auto_reset=auto_reset)
    env.reset()
    env.set_sub_batches(k, probe_streams=False)
    net = _net(env.obs_dim, seed)
    fused = FusedActorCritic(net, env, rollout=T, debug=True, seed=seed, **kw)
    return env, net, fused


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1. bitwise against the rollout launch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,use_lidar,pooled", [(1000, 3, True, False), (17, 1, True, False), (300, 2, False, False), (100, 2, True, True)])
def test_eval_equals_the_rollout_launch_bit_for_bit(n, k, use_lidar, pooled):
    """K0p = 192 (186 columns), 32 (6 columns; 15 pooled), a ragged last tile (1000 = 62 x 16 + 8, 300, 100) and one tile smaller than
    16 rows plus one full (17)."""
    T = 3
    env, net, fused = _setup(n, k, T, use_lidar, pooled=pooled)
    assert env.obs_dim == (15 if pooled else 186 if use_lidar else 6)
    lo_a = torch.as_tensor(env.action_space.low, device=DEV)
    hi_a = torch.as_tensor(env.action_space.high, device=DEV)
    fused.begin_rollout()
    det = torch.empty((n, 2), device=DEV)
    for t in range(T):
        obs = env.obs.clone()
        torch.cuda.synchronize()
        for i in range(env.sub_batches):
            fused.act(i)
        torch.cuda.synchronize()
        O, A, LP, V, R, Dn = fused.buffers()
        lp, v, mu = fused.evaluate(obs, A[t])
        fused.predict(obs, out=det)
        v2 = fused.value(obs)
        torch.cuda.synchronize()
        assert _bits(mu, fused.mu)
        assert _bits(v, V[t]) and _bits(v2, V[t])
        assert torch.equal(det, torch.max(torch.min(fused.mu, hi_a), lo_a))
        assert _bits(lp, LP[t])
        for i in range(env.sub_batches):
            env.step_slice(i, fused.actions)
        torch.cuda.synchronize()
    env.close()


# ---- 2. the whole rollout buffer in one call -------------------------------------------------------------------------------------
def test_eval_of_a_whole_rollout_buffer_in_one_call():
    T, N = 6, 1000                                   # 6000 rows: 375 tiles
    env, net, fused = _setup(N, 3, T, reward_scale=0.01)
    fused.begin_rollout()
    fused.rollout(T)
    torch.cuda.synchronize()
    O, A, LP, V, R, Dn = fused.buffers()
    lp, v, mu = fused.evaluate(O.reshape(T * N, env.obs_dim), A.reshape(T * N, 2))
    torch.cuda.synchronize()
    assert _bits(lp, LP.reshape(-1)) and _bits(v, V.reshape(-1))
    env.close()


# ---- 3. against torch, no environment --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs_dim", [1, 6, 31, 32, 33, 186])
def test_eval_matches_the_torch_modules_without_an_environment(obs_dim):
    from gym_auv_amd.policy import pack_policy_params, policy_eval
    net = _net(obs_dim, seed=obs_dim)
    params = pack_policy_params(net, obs_dim)
    g = torch.Generator(device=DEV).manual_seed(100 + obs_dim)
    Xall = torch.rand((1000, obs_dim), device=DEV, generator=g) * 2 - 1
    Aall = torch.randn((1000, 2), device=DEV, generator=g)
    with torch.no_grad():
        mu_ref, v_ref = net.pi(Xall), net.v(Xall).squeeze(-1)
        lp_ref = net.log_prob(mu_ref, Aall)
    for M in (1, 16, 17, 1000):
        r = policy_eval(params, obs_dim, Xall[:M].contiguous(), actions=Aall[:M].contiguous(), want=("mu", "value", "logp", "action"))
        torch.cuda.synchronize()
        assert tuple(r["mu"].shape) == (M, 2) and tuple(r["value"].shape) == (M,)
        e_mu, e_v = float((r["mu"] - mu_ref[:M]).abs().max()), float((r["value"] - v_ref[:M]).abs().max())
        print("obs_dim %d M %d: |mu - ref| %.2e |v - ref| %.2e" % (obs_dim, M, e_mu, e_v))
        assert e_mu <= 1e-5
        assert e_v <= 1e-5 * max(1.0, float(v_ref[:M].abs().max()))
        assert torch.equal(r["action"], r["mu"])                                     # (no map given: the identity, unclipped)
        # log pi: d lp / d mu = z / sigma per component, so the 1e-5 allowed on mu allows 1e-5 * sum_c |z_c| / sigma_c; plus a few
        # roundings of the terms themselves (4 ulp of the largest |lp|)
        sigma = net.log_std.exp()
        z = (Aall[:M] - mu_ref[:M]) / sigma
        tol = 1e-5 * float((z.abs() / sigma).sum(-1).max()) + 4 * 1.2e-7 * float(lp_ref[:M].abs().max())
        assert float((r["logp"] - lp_ref[:M]).abs().max()) <= tol


# ---- 3b. rows too wide for the LDS a launch gets unasked, at every compiled hidden-width triple ------------------------------------
@pytest.mark.parametrize("hidden", SUPPORTED_HIDDEN)
def test_eval_of_wide_rows_needs_the_prepared_instantiation(hidden):
    """obs_dim 1000: K0p = 1024 and the tiles take 64 (1024 + 8 + max(H1, H3) + 8) bytes -- more than the 64 KiB a kernel may ask for
    without hipFuncAttributeMaxDynamicSharedMemorySize, less than the 160 KiB the entry allows.  The launch therefore succeeds only if
    the host dispatch set the attribute on the very instantiation it then launches.  17 rows: one full tile and one of a single row.
    Reference: the torch modules in fp64 on the same weights.  Tolerance: 1e-5 was set for rows of at most 186 columns, so it is
    measured here -- four times the error of torch's own fp32 CPU forward against that fp64 result (the factor covers another
    summation order), and never less than 1e-5."""
    import copy
    import ppo
    from gym_auv_amd.policy import pack_policy_params, policy_eval
    obs_dim, M = 1000, 17
    lds = 64 * (1024 + 8 + max(hidden[0], hidden[2]) + 8)
    assert 64 * 1024 < lds < 160 * 1024
    torch.manual_seed(1000 + hidden[0] + hidden[1])
    net = ppo.ActorCritic(obs_dim, hidden=hidden)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.uniform_(-0.3, 0.3)
    X = torch.rand((M, obs_dim), generator=torch.Generator().manual_seed(17)) * 2 - 1
    net64 = copy.deepcopy(net).double()
    with torch.no_grad():
        mu64, v64 = net64.pi(X.double()), net64.v(X.double()).squeeze(-1)
        mu32, v32 = net.pi(X), net.v(X).squeeze(-1)
    net = net.to(DEV)
    r = policy_eval(pack_policy_params(net, obs_dim, hidden=hidden), obs_dim, X.to(DEV), want=("mu", "value"), hidden=hidden)
    torch.cuda.synchronize()
    assert tuple(r["mu"].shape) == (M, 2) and tuple(r["value"].shape) == (M,)
    for name, got, ref32, ref64 in (("mu", r["mu"], mu32, mu64), ("value", r["value"], v32, v64)):
        e32 = float((ref32.double() - ref64).abs().max())
        e = float((got.cpu().double() - ref64).abs().max())
        tol = max(1e-5, 4.0 * e32)
        print("hidden %s %s: |kernel - fp64| %.3e, |torch fp32 - fp64| %.3e, allowed %.3e" % (hidden, name, e, e32, tol))
        assert e <= tol, (hidden, name, e, e32)


# ---- 4. addressing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs_dim", [6, 186])
def test_eval_addressing_window_gather_canaries(obs_dim):
    from gym_auv_amd.policy import pack_policy_params, policy_eval
    net = _net(obs_dim, seed=7)
    params = pack_policy_params(net, obs_dim)
    g = torch.Generator(device=DEV).manual_seed(5)
    R = 200
    wide = torch.rand((R, obs_dim + 5), device=DEV, generator=g) * 2 - 1
    win = wide[:, 3:3 + obs_dim]                                  # ldx = obs_dim + 5 (odd): rows are 4-byte aligned only
    assert win.stride(0) == obs_dim + 5 and not win.is_contiguous()
    A = torch.randn((R, 2), device=DEV, generator=g)
    want = ("mu", "action", "value", "logp")
    amap = ((0.1, -0.2), (0.5, 2.0), (-0.3, -0.1), (0.2, 0.05))
    # a column window == its contiguous copy
    a = policy_eval(params, obs_dim, win, actions=A, want=want, action_map=amap)
    b = policy_eval(params, obs_dim, win.contiguous(), actions=A, want=want, action_map=amap)
    torch.cuda.synchronize()
    for w in want:
        assert _bits(a[w], b[w]), w
    cl = torch.max(torch.min(a["mu"], torch.tensor(amap[3], device=DEV)), torch.tensor(amap[2], device=DEV))
    assert torch.equal(a["action"], torch.tensor(amap[0], device=DEV) + torch.tensor(amap[1], device=DEV) * cl)
    # a gather with repeats == the contiguous call on X[idx]; M = 17
    M = 17
    idx = torch.tensor([5, 199, 0, 5, 5, 77, 198, 1, 0, 120, 121, 122, 60, 199, 3, 2, 5], device=DEV, dtype=torch.int64)
    Am = A[:M].contiguous()
    for X in (win, win.contiguous()):                             # (the 4-byte and, for an even obs_dim, the 8-byte path)
        ga = policy_eval(params, obs_dim, X, idx=idx, actions=Am, want=want, action_map=amap)
        gb = policy_eval(params, obs_dim, win[idx].contiguous(), actions=Am, want=want, action_map=amap)
        torch.cuda.synchronize()
        for w in want:
            assert _bits(ga[w], gb[w]), w
    # outputs one tile longer than M keep their canary past row M
    big = {w: torch.full((M + 16,) + ((2,) if w in ("mu", "action") else ()), CANARY, device=DEV) for w in want}
    c = policy_eval(params, obs_dim, win, idx=idx, actions=Am, want=want, action_map=amap, out={w: big[w][:M] for w in want})
    torch.cuda.synchronize()
    for w in want:
        assert _bits(c[w], ga[w]) and bool((big[w][M:] == CANARY).all()), w
    # a value-only call leaves mu / action / logp buffers alone, and the other way round
    for w in want:
        big[w].fill_(CANARY)
    policy_eval(params, obs_dim, win, idx=idx, want=("value",), out={"value": big["value"][:M]})
    torch.cuda.synchronize()
    assert _bits(big["value"][:M], ga["value"])
    assert all(bool((big[w] == CANARY).all()) for w in ("mu", "action", "logp"))
    big["value"].fill_(CANARY)
    policy_eval(params, obs_dim, win, idx=idx, actions=Am, want=("mu", "action", "logp"), action_map=amap,
                out={w: big[w][:M] for w in ("mu", "action", "logp")})
    torch.cuda.synchronize()
    assert bool((big["value"] == CANARY).all()) and all(_bits(big[w][:M], ga[w]) for w in ("mu", "action", "logp"))
    # action_ld = 2 into a slice [e0, e0 + M) of an [N][2] buffer
    N, e0 = 64, 9
    acts = torch.full((N, 2), CANARY, device=DEV)
    policy_eval(params, obs_dim, win, idx=idx, want=("action",), action_map=amap, out={"action": acts[e0:e0 + M]})
    torch.cuda.synchronize()
    assert _bits(acts[e0:e0 + M], ga["action"]) and bool((acts[:e0] == CANARY).all()) and bool((acts[e0 + M:] == CANARY).all())
    # a wider row stride of the action output
    wide_a = torch.full((M, 3), CANARY, device=DEV)
    policy_eval(params, obs_dim, win, idx=idx, want=("action",), action_map=amap, out={"action": wide_a[:, :2]})
    torch.cuda.synchronize()
    assert _bits(wide_a[:, :2], ga["action"]) and bool((wide_a[:, 2] == CANARY).all())


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def test_eval_refusals():
    import ctypes as C
    from gym_auv_amd import _capi
    from gym_auv_amd.batched_env import _LIB
    from gym_auv_amd.policy import pack_policy_params, policy_eval
    D = 6
    net = _net(D)
    params = pack_policy_params(net, D)
    X = torch.rand((20, D), device=DEV)
    A = torch.rand((20, 2), device=DEV)
    with pytest.raises(ValueError):
        policy_eval(params, D, X, want=("logp",))                                        # logp without actions
    with pytest.raises(ValueError):
        policy_eval(params, D, X, want=())                                               # no output
    with pytest.raises(ValueError):
        policy_eval(params, D, X.double(), want=("value",))                              # dtype
    with pytest.raises(ValueError):
        policy_eval(params, D, X.cpu(), want=("value",))                                 # device
    with pytest.raises(ValueError):
        policy_eval(params, D, X, actions=torch.rand((20, 4), device=DEV)[:, ::2], want=("logp",))    # non-contiguous A
    with pytest.raises(ValueError):
        policy_eval(params, D, X, idx=torch.zeros(3, dtype=torch.int32, device=DEV), want=("value",))
    with pytest.raises(ValueError):
        policy_eval(params[:-4], D, X, want=("value",))
    with pytest.raises(ValueError):
        policy_eval(params, D, X.t().contiguous().t(), want=("value",))                  # strided columns
    # M = 0: empty tensors, nothing launched
    r = policy_eval(params, D, X[:0], actions=A[:0], want=("mu", "action", "value", "logp"))
    assert tuple(r["mu"].shape) == (0, 2) and tuple(r["action"].shape) == (0, 2) and tuple(r["value"].shape) == (0,) and tuple(r["logp"].shape) == (0,)
    r = policy_eval(params, D, X, idx=torch.zeros(0, dtype=torch.int64, device=DEV), want=("value",))
    assert tuple(r["value"].shape) == (0,)
    # the C entry point itself refuses, before anything is enqueued
    v = torch.empty(20, device=DEV)

    def call(**kw):
        ev = _capi.AuvPolicyEval()
        ev.params, ev.X, ev.ldx, ev.obs_dim, ev.M, ev.action_ld = params.data_ptr(), X.data_ptr(), D, D, 20, 2
        ev.value = v.data_ptr()
        for k_, x in kw.items():
            setattr(ev, k_, x)
        return _LIB.auv_policy_eval(0, C.byref(ev), None)
    assert call(value=None) == _capi_einval()
    assert call(logp=v.data_ptr()) == _capi_einval()
    assert call(obs_dim=0) == _capi_einval()
    assert call(obs_dim=1 << 20) == _capi_einval()
    assert call(ldx=D - 1) == _capi_einval()
    assert call(M=-1) == _capi_einval()
    assert call(M=0) == 0
    assert call() == 0
    torch.cuda.synchronize()
    # FusedActorCritic: sampling stays with act / rollout
    env, net2, fused = _setup(32, 1, 2)
    with pytest.raises(ValueError, match="act"):
        fused.predict(deterministic=False)
    with pytest.raises(ValueError):
        fused.predict(env.obs[:5])                                                       # does not fit self.actions, no out given
    env.close()


def _capi_einval():
    return -1                                                                            # AUV_EINVAL (include/auv_hip.h)


# ---- 6. closed loop is deterministic and resumable -------------------------------------------------------------------------------
def test_closed_loop_with_predict_is_deterministic_and_value_calls_change_nothing():
    """20 steps of predict() + env.step from the same reset state (a snapshot taken behind the reset, restored before every run):
    the same STATE and COUNTERS bit for bit, also with value() / evaluate() calls between the steps."""
    env, net, fused = _setup(96, 1, 2)
    torch.cuda.synchronize()
    snap = env.snapshot()

    def loop(with_value):
        env.restore(snap)
        for t in range(20):
            fused.predict()
            if with_value:
                fused.value()
            env.step(fused.actions)
            if with_value:
                fused.value(), fused.evaluate(env.obs, fused.actions)
        torch.cuda.synchronize()
        return env.read("STATE").clone(), env.read("COUNTERS").clone(), env.obs.clone()
    first = loop(False)
    second = loop(False)
    third = loop(True)
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert int(first[1][:, 0].max()) >= 1                                             # (the environments did step)
    assert int(fused.buf[0]["ctr"][0]) == 0 and int(fused.buf[0]["ctr"][1]) == 0     # no rollout position, no generator step was spent
    env.close()


# ---- 7. auv_plan_score_v against the contract's loop -----------------------------------------------------------------------------
def _assert_scores(s, b, ws, wb, where):
    np.testing.assert_array_equal(s.cpu().numpy().view(np.uint32), ws.view(np.uint32), err_msg=str(where))
    np.testing.assert_array_equal(b.cpu().numpy(), wb, err_msg=str(where))


@pytest.mark.parametrize("T", [1, 5, 16])
def test_plan_score_v_equals_the_reference_loop_bit_for_bit(T):
    env, net, fused = _setup(8, 1, 2)                       # (a handle: the scoring needs only its device)
    n, group, gamma = 96, 8, 0.99
    g = torch.Generator(device=DEV).manual_seed(40 + T)
    rew = torch.randn((T, n), device=DEV, generator=g) * 3
    term = torch.randn((n,), device=DEV, generator=g) * 50
    done = torch.zeros((T, n), dtype=torch.uint8, device=DEV)
    done[0, 0:8] = 1                                        # group 0: done at t = 0
    done[T - 1, 8:16] = 1                                   # group 1: done at t = T - 1
    done[0, 16], done[T - 1, 17] = 1, 1                     # group 2: mixed; the rest: nowhere
    done[:, 40] = 1                                         # done everywhere: the first counts
    s, b = planning.plan_score(env, rew, done, group, gamma, terminal=term)
    torch.cuda.synchronize()
    ws, wb = planning.reference_plan_score_terminal(rew.cpu().numpy(), done.cpu().numpy(), group, gamma, term.cpu().numpy())
    _assert_scores(s, b, ws, wb, "plain")
    s0, b0 = planning.plan_score(env, rew, done, group, gamma)
    sn, bn = planning.plan_score(env, rew, done, group, gamma, terminal=None)
    torch.cuda.synchronize()
    assert _bits(s0, sn) and torch.equal(b0, bn)            # terminal = None: auv_plan_score
    assert not _bits(s0[24:32], s[24:32])                    # (the terminal does reach a score without a done)
    # NaN terminal where a done exists: never read -- finite and auv_plan_score's
    t2 = term.clone()
    t2[0:16] = float("nan")
    s2, b2 = planning.plan_score(env, rew, done, group, gamma, terminal=t2)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(s2[0:16]).all()) and _bits(s2[0:16], s0[0:16])
    _assert_scores(s2, b2, *planning.reference_plan_score_terminal(rew.cpu().numpy(), done.cpu().numpy(), group, gamma, t2.cpu().numpy()), "nan-done")
    # NaN terminal where no done exists: the score is NaN and never wins; a group of all NaN gives best 0
    t3 = term.clone()
    t3[24:27] = float("nan")                                # part of group 3
    t3[32:40] = float("nan")                                # all of group 4
    s3, b3 = planning.plan_score(env, rew, done, group, gamma, terminal=t3)
    torch.cuda.synchronize()
    assert bool(torch.isnan(s3[24:27]).all()) and bool(torch.isnan(s3[32:40]).all())
    assert int(b3[3]) >= 3 and int(b3[4]) == 0
    _assert_scores(s3, b3, *planning.reference_plan_score_terminal(rew.cpu().numpy(), done.cpu().numpy(), group, gamma, t3.cpu().numpy()), "nan-free")
    # a group that does not fit the packed geometry (a wave to itself), and bad terminals
    s4, b4 = planning.plan_score(env, rew, done, 12, gamma, terminal=term)
    torch.cuda.synchronize()
    _assert_scores(s4, b4, *planning.reference_plan_score_terminal(rew.cpu().numpy(), done.cpu().numpy(), 12, gamma, term.cpu().numpy()), "group 12")
    with pytest.raises(ValueError):
        planning.plan_score(env, rew, done, group, gamma, terminal=term[:-1])
    with pytest.raises(ValueError):
        planning.plan_score(env, rew, done, group, gamma, terminal=term.double())
    env.close()


# ---- 8. the planner --------------------------------------------------------------------------------------------------------------
def test_planner_with_a_terminal_value_and_a_policy_prior():
    B, K, T = 4, 16, 4
    env, net, fused = _setup(B, 1, 2)
    for t in range(3):
        fused.predict()
        env.step(fused.actions)
    planner = planning.ShootingPlanner(env, candidates=K, horizon=T, gamma=0.97, seed=3, value=fused, value_scale=100.0)
    act, seqs, pred = planner.plan(seed=3)
    torch.cuda.synchronize()
    last = planner.last
    assert tuple(last["terminal"].shape) == (B * K,)
    assert _bits(last["terminal"], fused.value(planner.sim.obs) * 100.0)
    ws, wb = planning.reference_plan_score_terminal(last["reward"].cpu().numpy(), last["done"].cpu().numpy(), K, 0.97, last["terminal"].cpu().numpy())
    _assert_scores(last["score"], last["best"], ws, wb, "planner")
    chosen = torch.arange(B, device=DEV) * K + last["best"].long()
    assert torch.equal(seqs, last["ring"][:, chosen, :]) and _bits(pred, last["score"][chosen])
    # an eager callable gives the same terminal up to the torch modules' 1e-5 (x the scale), through the same scoring
    with torch.no_grad():
        p_eager = planning.ShootingPlanner(env, candidates=K, horizon=T, gamma=0.97, seed=3, value=lambda o: net.v(o).squeeze(-1), value_scale=100.0)
        p_eager.plan(seed=3)
    torch.cuda.synchronize()
    assert torch.equal(p_eager.last["ring"], last["ring"])
    assert float((p_eager.last["terminal"] - last["terminal"]).abs().max()) <= 100.0 * 1e-5 * max(1.0, float(last["terminal"].abs().max()) / 100.0)
    p_eager.close()
    # prior: K = 1, one iteration -- the chosen sequence is predict() at the real observation, T times
    p_prior = planning.ShootingPlanner(env, candidates=1, horizon=T, gamma=0.97, seed=3, prior=fused)
    a1, s1, _ = p_prior.plan(seed=3)
    det = fused.predict().clone()
    torch.cuda.synchronize()
    assert torch.equal(a1, det) and torch.equal(s1, det[None].expand(T, B, 2))
    assert "terminal" not in p_prior.last
    p_prior.close()
    # both None: the planner of before
    p_none = planning.ShootingPlanner(env, candidates=K, horizon=T, gamma=0.97, seed=3, value=None, prior=None)
    p_old = planning.ShootingPlanner(env, candidates=K, horizon=T, gamma=0.97, seed=3)
    x, y = p_none.plan(seed=11), p_old.plan(seed=11)
    torch.cuda.synchronize()
    assert all(_bits(u, v) for u, v in zip(x, y)) and "terminal" not in p_none.last
    with pytest.raises(ValueError):
        planning.ShootingPlanner(env, candidates=K, horizon=T, value=3.0)
    p_none.close(), p_old.close(), planner.close(), env.close()
