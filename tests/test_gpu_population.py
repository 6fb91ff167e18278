"""-m gpu: a population of policies in one launch (csrc/k11_population.hip; gym_auv_amd/population.py).

Every comparison is BITWISE.  The population launch against auv_policy_eval on the same rows with the same block: the matrix chains
are the same code (pol_prefetch / pol_layer in the same order with the same template arguments) and the epilogue is the same
expression on the same floats.  The perturbation and the ES update against the NumPy mirrors of their contract: integer hashing, exact
conversions and single rounded float32 operations in a stated order.  The rollout call against a Python loop of act -> env.step on a
second handle from the same seed."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from gym_auv_amd import population as pop
from gym_auv_amd.config import effective_reference_config
from gym_auv_amd.scenarios import polygon_world
from gym_auv_amd.world import build_world, pack_bank

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
DEV = "cuda:0"
CANARY = -777.25
EINVAL = -1                                                     # AUV_EINVAL (include/auv_hip.h)
AMAP = ((0.1, -0.2), (0.5, 2.0), (-0.3, -0.1), (0.2, 0.05))


def _net(obs_dim, seed=0):
    import ppo
    torch.manual_seed(seed)
    net = ppo.ActorCritic(obs_dim).to(DEV)
    with torch.no_grad():
        for m in net.modules():                      # weights of ordinary size, biases that matter
            if isinstance(m, torch.nn.Linear):
                m.bias.uniform_(-0.3, 0.3)
    return net


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _np_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


_BLOCKS = {}


def _blocks(obs_dim):
    """(full packed buffers of three differently seeded nets, their policy halves stacked as members with a stride wider than a
    block): made once per obs_dim, never written again."""
    if obs_dim not in _BLOCKS:
        from gym_auv_amd.policy import pack_policy_params
        nf = pop.member_floats(obs_dim)
        params = [pack_policy_params(_net(obs_dim, seed=10 + s), obs_dim) for s in range(3)]
        members = torch.zeros((3, nf + 8), device=DEV)
        for p in range(3):
            members[p, :nf].copy_(params[p][:nf])
        torch.cuda.synchronize()
        _BLOCKS[obs_dim] = (params, members)
    return _BLOCKS[obs_dim]


# ---- 1. the population launch == auv_policy_eval per member, bit for bit ------------------------------------------------------------
@pytest.mark.parametrize("obs_dim", [6, 15, 186])
@pytest.mark.parametrize("P,G,M", [(3, 16, 48), (2, 32, 64), (3, 32, 80), (3, 16, 41)])
def test_act_equals_policy_eval_of_each_member_bit_for_bit(obs_dim, P, G, M):
    """(3, 32, 80): a ragged last member whose last tile is full; (3, 16, 41): a partial last tile.  ldx = obs_dim + 5 (odd for an
    even obs_dim: rows 4-byte aligned only) and the contiguous copy (the 8-byte path where obs_dim is even)."""
    from gym_auv_amd.policy import policy_eval
    params, members = _blocks(obs_dim)
    g = torch.Generator(device=DEV).manual_seed(1000 + obs_dim + M)
    wide = torch.rand((M, obs_dim + 5), device=DEV, generator=g) * 2 - 1
    win = wide[:, 3:3 + obs_dim]
    assert win.stride(0) == obs_dim + 5 > obs_dim
    for X in (win, win.contiguous()):
        mu = torch.full((M + 16, 2), CANARY, device=DEV)
        act = torch.full((M + 16, 2), CANARY, device=DEV)
        r = pop.population_act(members[:P], obs_dim, G, X, want=("mu", "action"), action_map=AMAP, out={"mu": mu[:M], "action": act[:M]})
        torch.cuda.synchronize()
        for p in range(P):
            lo, hi = p * G, min((p + 1) * G, M)
            if lo >= hi:
                continue
            ref = policy_eval(params[p], obs_dim, X[lo:hi], want=("mu", "action"), action_map=AMAP)
            torch.cuda.synchronize()
            assert _bits(r["mu"][lo:hi], ref["mu"]), (p, "mu")
            assert _bits(r["action"][lo:hi], ref["action"]), (p, "action")
        assert bool((mu[M:] == CANARY).all()) and bool((act[M:] == CANARY).all())      # rows >= M are untouched
    # members do differ: member 1's rows through member 0's block give other bits
    other = policy_eval(params[0], obs_dim, win[G:min(2 * G, M)], want=("mu",))["mu"]
    torch.cuda.synchronize()
    assert not _bits(r["mu"][G:min(2 * G, M)], other)
    # action_ld = 2 straight into rows [e0, e0 + M) of an [N][2] buffer; a wider row stride
    N, e0 = M + 40, 8
    buf = torch.full((N, 2), CANARY, device=DEV)
    pop.population_act(members[:P], obs_dim, G, win, want=("action",), action_map=AMAP, out={"action": buf[e0:e0 + M]})
    wide_a = torch.full((M, 3), CANARY, device=DEV)
    pop.population_act(members[:P], obs_dim, G, win, want=("action",), action_map=AMAP, out={"action": wide_a[:, :2]})
    torch.cuda.synchronize()
    assert _bits(buf[e0:e0 + M], r["action"]) and bool((buf[:e0] == CANARY).all()) and bool((buf[e0 + M:] == CANARY).all())
    assert _bits(wide_a[:, :2], r["action"]) and bool((wide_a[:, 2] == CANARY).all())


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------
def test_act_refusals_enqueue_nothing():
    from gym_auv_amd import _capi
    from gym_auv_amd.batched_env import _LIB
    D = 6
    params, members = _blocks(D)
    nf = pop.member_floats(D)
    stride = members.stride(0)
    X = torch.rand((48, D), device=DEV)
    mu = torch.full((48, 2), CANARY, device=DEV)
    act = torch.full((48, 2), CANARY, device=DEV)
    fit = torch.full((48,), CANARY, device=DEV)
    ends = torch.full((48,), 7, dtype=torch.int32, device=DEV)
    rew = torch.ones(48, device=DEV)
    done = torch.ones(48, dtype=torch.uint8, device=DEV)

    def call(**kw):
        io = _capi.AuvPopulationIO()
        io.members, io.stride, io.G = members.data_ptr(), stride, 16
        io.X, io.ldx, io.M, io.obs_dim, io.action_ld = X.data_ptr(), D, 48, D, 2
        io.mu, io.action, io.act, io.accumulate = mu.data_ptr(), act.data_ptr(), 1, 0
        for k_, x in kw.items():
            setattr(io, k_, x)
        return _LIB.auv_population_act(0, C.byref(io), None)
    for bad in (dict(G=0), dict(G=-16), dict(G=24), dict(G=8), dict(members=members.data_ptr() + 4), dict(members=None),
                dict(stride=nf - 4), dict(stride=nf + 2), dict(obs_dim=0), dict(obs_dim=1 << 20), dict(ldx=D - 1), dict(action_ld=1),
                dict(mu=None, action=None), dict(act=0), dict(M=-1), dict(X=None),
                dict(accumulate=1), dict(accumulate=1, reward_in=rew.data_ptr(), done_in=done.data_ptr(), fit=fit.data_ptr())):
        assert call(**bad) == EINVAL, bad
    torch.cuda.synchronize()
    assert bool((mu == CANARY).all()) and bool((act == CANARY).all()) and bool((fit == CANARY).all()) and bool((ends == 7).all())
    assert call(M=0) == 0
    torch.cuda.synchronize()
    assert bool((mu == CANARY).all())
    # accumulation alone (the flush launch) touches fit / ends only; with act it does both
    acc = dict(accumulate=1, reward_in=rew.data_ptr(), done_in=done.data_ptr(), fit=fit.data_ptr(), ends=ends.data_ptr())
    fit.zero_()
    assert call(act=0, mu=None, action=None, M=41, **acc) == 0
    torch.cuda.synchronize()
    assert bool((mu == CANARY).all()) and bool((fit[:41] == 1).all()) and bool((fit[41:] == 0).all())
    assert bool((ends[:41] == 8).all()) and bool((ends[41:] == 7).all())
    assert call(**acc) == 0 and call() == 0
    torch.cuda.synchronize()
    assert bool((fit == torch.tensor([2.0] * 41 + [1.0] * 7, device=DEV)).all()) and not bool((mu == CANARY).any())
    # the Python surface refuses what the launch would
    with pytest.raises(ValueError):
        pop.population_act(members, D, 24, X)
    with pytest.raises(ValueError):
        pop.population_act(members[:2], D, 16, X)                                       # 48 rows need three members
    with pytest.raises(ValueError):
        pop.population_act(members[:, :nf - 4], D, 16, X)
    with pytest.raises(ValueError):
        pop.population_act(members, D, 16, X.double())
    with pytest.raises(ValueError):
        pop.population_act(members, D, 16, X, want=("value",))


# ---- 3. perturb == its mirror --------------------------------------------------------------------------------------------------------
def _lib_dev():
    from gym_auv_amd.batched_env import _LIB
    return _LIB


def _perturb(theta, members, P, obs_dim, sigma, seed, gen):
    rc = _lib_dev().auv_population_perturb(0, C.c_void_p(theta.data_ptr()), C.c_void_p(members.data_ptr()), members.stride(0), P, obs_dim, sigma, seed,
                                           gen, None)
    assert rc == 0, rc


def _theta(obs_dim, seed):
    """a base block with padding at zero, as packing leaves it"""
    rs = np.random.RandomState(seed)
    nf = pop.member_floats(obs_dim)
    return np.where(pop.padding_mask(obs_dim), 0.0, rs.randn(nf) * 0.3).astype(np.float32)


@pytest.mark.parametrize("obs_dim", [6, 186])
@pytest.mark.parametrize("P", [2, 8])
def test_perturb_equals_the_mirror_bit_for_bit(obs_dim, P):
    nf = pop.member_floats(obs_dim)
    mask = pop.padding_mask(obs_dim)
    th = _theta(obs_dim, 3)
    theta = torch.as_tensor(th, device=DEV)
    seed, sigma = 0x1234567890abcdef, 0.02
    got = {}
    for gen in (0, 7):
        for stride in (nf, nf + 12):
            members = torch.full((P, stride), CANARY, device=DEV)
            _perturb(theta, members, P, obs_dim, sigma, seed, gen)
            again = torch.full((P, stride), 1.0, device=DEV)
            _perturb(theta, again, P, obs_dim, sigma, seed, gen)
            torch.cuda.synchronize()
            m = members.cpu().numpy()
            assert _np_bits(m, pop.perturb_reference(th, P, obs_dim, sigma, seed, gen, stride=stride)), (gen, stride)
            assert _np_bits(m[:, :nf][:, mask], np.broadcast_to(th[mask], (P, int(mask.sum()))))      # padding keeps the base
            assert (m[:, :nf][:, ~mask] != th[~mask]).mean() > 0.99
            assert _bits(members, again)                                                       # the same key, the same bytes
            got[gen] = m[:, :nf]
    assert not np.array_equal(got[0], got[7])                                                  # another generation, other bytes
    assert torch.equal(theta.cpu(), torch.as_tensor(th))                                       # the base is only read
    for bad in (dict(stride=nf - 4), dict(stride=nf + 1), dict(P=0), dict(sigma=float("nan")), dict(obs_dim=0)):
        a = dict(stride=nf, P=P, obs_dim=obs_dim, sigma=sigma)
        a.update(bad)
        assert _lib_dev().auv_population_perturb(0, C.c_void_p(theta.data_ptr()), C.c_void_p(members.data_ptr()), a["stride"], a["P"], a["obs_dim"],
                                                 a["sigma"], seed, 0, None) == EINVAL, bad


# ---- 4. update == its mirror ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs_dim", [6, 186])
@pytest.mark.parametrize("P", [2, 8])
def test_update_equals_the_mirror_bit_for_bit(obs_dim, P):
    nf = pop.member_floats(obs_dim)
    mask = pop.padding_mask(obs_dim)
    th = _theta(obs_dim, 4)
    rs = np.random.RandomState(P)
    w_np = rs.randn(P).astype(np.float32)
    seed, sigma, gen = 99, 0.02, 5
    LIB = _lib_dev()

    def run(w, lr):
        theta = torch.as_tensor(th, device=DEV)
        grad = torch.full((nf,), CANARY, device=DEV)
        wd = torch.as_tensor(w, device=DEV)
        assert LIB.auv_population_update(0, C.c_void_p(theta.data_ptr()), C.c_void_p(wd.data_ptr()), C.c_void_p(grad.data_ptr()), P, obs_dim, sigma, lr,
                                         seed, gen, None) == 0
        torch.cuda.synchronize()
        return grad.cpu().numpy(), theta.cpu().numpy()
    for lr in (0.0, 0.01):
        grad, new = run(w_np, lr)
        want_g, want_t = pop.es_update_reference(th, w_np, obs_dim, sigma, lr, seed, gen)
        assert _np_bits(grad, want_g), lr
        assert _np_bits(new, want_t), lr
        assert not grad[mask].view(np.uint32).any() and _np_bits(new[mask], th[mask])
        if lr == 0.0:
            assert _np_bits(new, th)                                                           # theta untouched
        else:
            assert (new[~mask] != th[~mask]).mean() > 0.9
    grad, new = run(np.full(P, 0.37, np.float32), 0.01)
    assert not grad.view(np.uint32).any() and _np_bits(new, th)                                # equal weights: all zero bits
    theta = torch.as_tensor(th, device=DEV)
    grad_d = torch.zeros(nf, device=DEV)
    wd = torch.as_tensor(w_np, device=DEV)
    for bad in (dict(P=P + 1), dict(P=0), dict(sigma=0.0), dict(sigma=-1.0), dict(lr=float("inf")), dict(obs_dim=0)):
        a = dict(P=P, obs_dim=obs_dim, sigma=sigma, lr=0.01)
        a.update(bad)
        assert LIB.auv_population_update(0, C.c_void_p(theta.data_ptr()), C.c_void_p(wd.data_ptr()), C.c_void_p(grad_d.data_ptr()), a["P"], a["obs_dim"],
                                         a["sigma"], a["lr"], seed, gen, None) == EINVAL, bad


# ---- 5. the rollout call == a host loop of act -> step -----------------------------------------------------------------------------
def _env(n=32, max_timesteps=3):
    from gym_auv_amd.batched_env import BatchedAuvEnv
    cfg = effective_reference_config(use_lidar=True)
    cfg.episode.max_timesteps = max_timesteps
    bank = pack_bank([build_world(polygon_world(700 + i, n_polygons=10, n_circles=6, n_moving=5)) for i in range(4)])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = BatchedAuvEnv(cfg, bank, n, device=DEV, auto_reset=True)
    env.reset()
    return env


def _population(env, P, seed=3):
    p = pop.PolicyPopulation(env, P, net=_net(env.obs_dim, seed=21), seed=seed)
    p.perturb(0.05, 0)                                           # members that differ
    return p


@pytest.mark.parametrize("bounds", [None, (0, 16)])
def test_rollout_equals_a_host_loop_of_act_and_step_bit_for_bit(bounds):
    """32 environments, two members of 16, T = 6 with max_timesteps = 3: every environment auto-resets inside the window.  One chain on
    the caller's stream, and two chains of 16."""
    T = 6
    a, b = _env(), _env()
    pa, pb = _population(a, 2), _population(b, 2)
    assert (pa.P, pa.G) == (2, 16) and not _bits(pa.members[0], pa.members[1])
    fitness, ends = pa.rollout(T, bounds=bounds)
    fit = torch.zeros(32, device=DEV)
    cnt = torch.zeros(32, dtype=torch.int32, device=DEV)
    for t in range(T):
        pb.act()
        b.step(pb.actions)
        fit = fit + b.reward                                     # float32, one rounded add per step, in step order
        cnt = cnt + b.done.to(torch.int32)
    torch.cuda.synchronize()
    assert _bits(pa.fit, fit) and torch.equal(pa.ends, cnt)
    assert int(cnt.sum()) > 0 and bool((fit != 0).any())
    assert _bits(pa.actions, pb.actions) and _bits(a.obs, b.obs) and _bits(a.reward, b.reward) and torch.equal(a.done, b.done)
    for f in ("STATE", "COUNTERS", "WORLD_IDX"):
        assert torch.equal(a.read(f), b.read(f)), f
    assert _bits(fitness, fit.view(2, 16).mean(dim=1)) and torch.equal(ends, cnt.view(2, 16).sum(dim=1))
    # a second window starts from zero: the accumulators are cleared, and the first launch of a call adds nothing
    f2, _ = pa.rollout(1)
    torch.cuda.synchronize()
    assert _bits(pa.fit, a.reward)
    with pytest.raises(ValueError):
        pa.rollout(1, bounds=(0, 8))
    a.close(), b.close()


def test_rollout_refuses_slices_that_split_a_member():
    from gym_auv_amd.batched_env import _LIB
    env = _env()
    p = _population(env, 1)                                      # one member of 32 rows
    st = torch.cuda.current_stream()
    ios = (p._io_type * 2)(p._io(), p._io())
    rc = _LIB.auv_population_rollout(env._h, 2, (C.c_int32 * 3)(0, 16, 32), (C.c_void_p * 2)(st.cuda_stream, st.cuda_stream), ios,
                                     C.c_void_p(env.obs.data_ptr()), C.c_void_p(env.reward.data_ptr()), C.c_void_p(env.done.data_ptr()), 1, 1)
    assert rc == EINVAL
    torch.cuda.synchronize()
    assert not bool(p.fit.any()) and int(env.read("COUNTERS")[:, 0].max()) == 0      # nothing stepped
    env.close()


# ---- 6. one ES generation on the device == the mirrors -----------------------------------------------------------------------------
def test_one_es_generation_on_the_device_equals_the_mirrors():
    env = _env(64, max_timesteps=4)
    p = pop.PolicyPopulation(env, 4, net=_net(env.obs_dim, seed=5), seed=77)
    sigma, lr, gen = 0.05, 0.02, 3
    th0 = p.theta.cpu().numpy()
    assert not th0[pop.padding_mask(env.obs_dim)].any()
    p.perturb(sigma, gen)
    fitness, ends = p.rollout(5)
    w = p.centered_ranks(fitness)
    p.update(w, lr, sigma, gen)
    torch.cuda.synchronize()
    assert _np_bits(p.members.cpu().numpy(), pop.perturb_reference(th0, 4, env.obs_dim, sigma, 77, gen))
    wn = w.cpu().numpy()
    assert np.allclose(sorted(wn), np.linspace(-0.5, 0.5, 4))
    assert int(np.argmax(wn)) == int(torch.argmax(fitness))
    grad, new = pop.es_update_reference(th0, wn, env.obs_dim, sigma, lr, 77, gen)
    assert _np_bits(p.grad.cpu().numpy(), grad) and _np_bits(p.theta.cpu().numpy(), new)
    assert not np.array_equal(new, th0)
    # the champion through a FusedActorCritic: predict() then gives the base block's deterministic action
    from gym_auv_amd.policy import FusedActorCritic
    fused = FusedActorCritic(_net(env.obs_dim, seed=6), env, rollout=2)
    p.base_state_into(fused)
    p.members.copy_(p.theta.unsqueeze(0).expand(4, p.stride))
    fused.predict()
    p.act()
    torch.cuda.synchronize()
    assert _bits(fused.actions, p.actions)
    env.close()
