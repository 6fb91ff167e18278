"""-m gpu: the population of policies at the other hidden widths of POL_ARCH_LIST (csrc/auv_population_pass.h, k14_population_arch.hip;
the auv_population_*_arch entries; gym_auv_amd/population.py with hidden=).

Every comparison but one is BITWISE, as in tests/test_gpu_population.py: the population launch against auv_policy_eval_arch on the same
rows with the same block at the same widths (the same pol_trunk<false, A>, the same epilogue), the perturbation and the ES update
against the NumPy mirrors of their contract, the rollout call against a host loop of act -> env.step on a second handle from the same
seed.  The one that is not: the means against a torch fp32 forward of the same modules at 1e-5 absolute, the project's standing bar for
the policy kernels, so that the bitwise comparison does not rest on k9 alone.

Shapes: obs_dim 6 (K0p = 32, narrower than every H2: the X tile's width is set by Y2) and 186 (K0p = 192, wider than H2 = 64 and 128:
set by X); (P, G, M) = (3, 16, 41), a ragged last tile, with members 8 floats further apart than a block -- a launch that took the
reference's member size or ignored the stride would read another block -- and (2, 32, 64), two tiles per member."""
import ctypes as C
import os
import sys
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gym_auv_amd import _capi
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
DEFAULT = (256, 128, 64)
OTHERS = [(128, 128, 64), (128, 64, 64), (64, 64, 64)]


def _lib():
    from gym_auv_amd.batched_env import _LIB
    return _LIB


def _arch(hidden):
    return _capi.AuvPolicyArch(*hidden)


def _net(obs_dim, hidden, seed=0):
    import ppo
    torch.manual_seed(seed)
    net = ppo.ActorCritic(obs_dim, hidden=hidden).to(DEV)
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


def _blocks(obs_dim, hidden):
    """(three differently seeded nets, their full packed buffers, their policy halves as members `nf + 8` floats apart with a canary
    in the gap): made once per (obs_dim, hidden), never written again."""
    key = (obs_dim, hidden)
    if key not in _BLOCKS:
        from gym_auv_amd.policy import pack_policy_params
        nf = pop.member_floats(obs_dim, hidden)
        nets = [_net(obs_dim, hidden, seed=10 + s) for s in range(3)]
        params = [pack_policy_params(n, obs_dim, hidden=hidden) for n in nets]
        members = torch.full((3, nf + 8), CANARY, device=DEV)
        for p in range(3):
            members[p, :nf].copy_(params[p][:nf])
        torch.cuda.synchronize()
        _BLOCKS[key] = (nets, params, members)
    return _BLOCKS[key]


def _rows(obs_dim, M):
    g = torch.Generator(device=DEV).manual_seed(1000 + obs_dim + M)
    return torch.rand((M, obs_dim), device=DEV, generator=g) * 2 - 1


# ---- 1. the population launch == auv_policy_eval_arch per member, bit for bit ----------------------------------------------------------
@pytest.mark.parametrize("hidden", OTHERS)
@pytest.mark.parametrize("obs_dim", [6, 186])
@pytest.mark.parametrize("P,G,M,wide", [(3, 16, 41, True), (2, 32, 64, False)])
def test_act_equals_policy_eval_of_each_member_bit_for_bit(hidden, obs_dim, P, G, M, wide):
    from gym_auv_amd.policy import policy_eval
    _, params, gapped = _blocks(obs_dim, hidden)
    nf = pop.member_floats(obs_dim, hidden)
    members = gapped[:P] if wide else gapped[:P, :nf].contiguous()
    assert members.stride(0) == (nf + 8 if wide else nf) and nf < pop.member_floats(obs_dim)
    X = _rows(obs_dim, M)
    mu = torch.full((M + 16, 2), CANARY, device=DEV)
    act = torch.full((M + 16, 2), CANARY, device=DEV)
    r = pop.population_act(members, obs_dim, G, X, want=("mu", "action"), action_map=AMAP, out={"mu": mu[:M], "action": act[:M]}, hidden=hidden)
    torch.cuda.synchronize()
    for p in range(P):
        lo, hi = p * G, min((p + 1) * G, M)
        ref = policy_eval(params[p], obs_dim, X[lo:hi], want=("mu", "action"), action_map=AMAP, hidden=hidden)
        torch.cuda.synchronize()
        assert _bits(r["mu"][lo:hi], ref["mu"]), (p, "mu")
        assert _bits(r["action"][lo:hi], ref["action"]), (p, "action")
    # the action is the map applied to the mean: mid + half * clip(mu, lo, hi), a rounded product and a rounded sum
    mid, half, lo_c, hi_c = (torch.tensor(v, device=DEV) for v in AMAP)
    assert _bits(r["action"], mid + half * torch.minimum(torch.maximum(r["mu"], lo_c), hi_c))
    assert bool((r["action"] != r["mu"]).any())
    assert bool((mu[M:] == CANARY).all()) and bool((act[M:] == CANARY).all())          # rows >= M are untouched
    assert bool((gapped[:, nf:] == CANARY).all())                                       # the members are only read
    # members do differ: member 1's rows through member 0's block give other bits
    other = policy_eval(params[0], obs_dim, X[G:min(2 * G, M)], want=("mu",), hidden=hidden)["mu"]
    torch.cuda.synchronize()
    assert not _bits(r["mu"][G:min(2 * G, M)], other)


# ---- 2. the means against the torch modules -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", OTHERS)
def test_act_matches_a_torch_forward_of_each_member(hidden):
    obs_dim, P, G, M = 186, 3, 16, 41
    nets, _, gapped = _blocks(obs_dim, hidden)
    X = _rows(obs_dim, M)
    mu = pop.population_act(gapped[:P], obs_dim, G, X, want=("mu",), hidden=hidden)["mu"]
    torch.cuda.synchronize()
    for p in range(P):
        lo, hi = p * G, min((p + 1) * G, M)
        with torch.no_grad():
            ref = nets[p].pi(X[lo:hi])
        e = float((mu[lo:hi] - ref).abs().max())
        print("hidden %s member %d: |mu - torch| %.2e" % (list(hidden), p, e))
        assert e <= 1e-5


# ---- 3. the default triple through the _arch entries == the plain entries -----------------------------------------------------------
def _perturb(hidden, theta, members, P, obs_dim, sigma, seed, gen, plain=False):
    head = (0, C.c_void_p(theta.data_ptr()), C.c_void_p(members.data_ptr()), members.stride(0), P, obs_dim, sigma, seed, gen)
    rc = _lib().auv_population_perturb(*head, None) if plain else _lib().auv_population_perturb_arch(*head, C.byref(_arch(hidden)), None)
    assert rc == 0, (rc, _lib().auv_last_error())


def _update(hidden, theta, w, grad, P, obs_dim, sigma, lr, seed, gen, plain=False):
    head = (0, C.c_void_p(theta.data_ptr()), C.c_void_p(w.data_ptr()), C.c_void_p(grad.data_ptr()), P, obs_dim, sigma, lr, seed, gen)
    rc = _lib().auv_population_update(*head, None) if plain else _lib().auv_population_update_arch(*head, C.byref(_arch(hidden)), None)
    assert rc == 0, (rc, _lib().auv_last_error())


def _theta(obs_dim, hidden, seed):
    """a base block with padding at zero, as packing leaves it"""
    rs = np.random.RandomState(seed)
    nf = pop.member_floats(obs_dim, hidden)
    return np.where(pop.padding_mask(obs_dim, hidden), 0.0, rs.randn(nf) * 0.3).astype(np.float32)


@pytest.mark.parametrize("obs_dim", [6, 186])
def test_default_triple_through_the_arch_entries_equals_the_plain_entries(obs_dim):
    _, _, gapped = _blocks(obs_dim, DEFAULT)
    P, G, M = 3, 16, 41
    X = _rows(obs_dim, M)
    a = pop.population_act(gapped[:P], obs_dim, G, X, want=("mu", "action"), action_map=AMAP)
    b = pop.population_act(gapped[:P], obs_dim, G, X, want=("mu", "action"), action_map=AMAP, hidden=DEFAULT, arch_entry=True)
    torch.cuda.synchronize()
    assert _bits(a["mu"], b["mu"]) and _bits(a["action"], b["action"]) and bool(a["mu"].abs().sum() > 0)
    nf = pop.member_floats(obs_dim)
    assert int(_lib().auv_population_member_floats_arch(obs_dim, C.byref(_arch(DEFAULT)))) == nf
    theta = torch.as_tensor(_theta(obs_dim, DEFAULT, 3), device=DEV)
    m0, m1 = torch.full((4, nf + 4), CANARY, device=DEV), torch.full((4, nf + 4), 1.0, device=DEV)
    _perturb(DEFAULT, theta, m0, 4, obs_dim, 0.02, 77, 5, plain=True)
    _perturb(DEFAULT, theta, m1, 4, obs_dim, 0.02, 77, 5)
    w = torch.as_tensor(np.array([0.5, -0.25, 0.1, 0.3], np.float32), device=DEV)
    t0, t1 = theta.clone(), theta.clone()
    g0, g1 = torch.full((nf,), CANARY, device=DEV), torch.full((nf,), 1.0, device=DEV)
    _update(DEFAULT, t0, w, g0, 4, obs_dim, 0.02, 0.01, 77, 5, plain=True)
    _update(DEFAULT, t1, w, g1, 4, obs_dim, 0.02, 0.01, 77, 5)
    torch.cuda.synchronize()
    assert _bits(m0, m1) and _bits(g0, g1) and _bits(t0, t1) and not _bits(t0, theta)


# ---- 4. perturb and update == their mirrors ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", OTHERS)
@pytest.mark.parametrize("obs_dim", [6, 186])
@pytest.mark.parametrize("P", [2, 8])
def test_perturb_equals_the_mirror_bit_for_bit(hidden, obs_dim, P):
    nf = pop.member_floats(obs_dim, hidden)
    mask = pop.padding_mask(obs_dim, hidden)
    th = _theta(obs_dim, hidden, 3)
    theta = torch.as_tensor(th, device=DEV)
    seed, sigma = 0x1234567890abcdef, 0.02
    got = {}
    for gen, stride in ((0, nf), (7, nf + 12)):
        members = torch.full((P, stride), CANARY, device=DEV)
        _perturb(hidden, theta, members, P, obs_dim, sigma, seed, gen)
        torch.cuda.synchronize()
        m = members.cpu().numpy()
        assert _np_bits(m, pop.perturb_reference(th, P, obs_dim, sigma, seed, gen, stride=stride, hidden=hidden)), (gen, stride)
        assert _np_bits(m[:, :nf][:, mask], np.broadcast_to(th[mask], (P, int(mask.sum()))))      # padding keeps the base
        assert not m[:, nf:].view(np.uint32).any()                                                  # the tail is zero
        assert (m[:, :nf][:, ~mask] != th[~mask]).mean() > 0.99
        got[gen] = m[:, :nf]
    assert not np.array_equal(got[0], got[7])                                                  # another generation, other bytes
    assert torch.equal(theta.cpu(), torch.as_tensor(th))                                       # the base is only read


@pytest.mark.parametrize("hidden", OTHERS)
@pytest.mark.parametrize("obs_dim", [6, 186])
@pytest.mark.parametrize("P", [2, 8])
def test_update_equals_the_mirror_bit_for_bit(hidden, obs_dim, P):
    nf = pop.member_floats(obs_dim, hidden)
    mask = pop.padding_mask(obs_dim, hidden)
    th = _theta(obs_dim, hidden, 4)
    w_np = np.random.RandomState(P).randn(P).astype(np.float32)
    seed, sigma, gen = 99, 0.02, 5

    def run(w, lr):
        theta = torch.as_tensor(th, device=DEV)
        buf = torch.full((nf + 8,), CANARY, device=DEV)
        _update(hidden, theta, torch.as_tensor(w, device=DEV), buf[:nf], P, obs_dim, sigma, lr, seed, gen)
        torch.cuda.synchronize()
        assert bool((buf[nf:] == CANARY).all())                                                # nothing behind the block
        return buf[:nf].cpu().numpy(), theta.cpu().numpy()
    for lr in (0.0, 0.01):
        grad, new = run(w_np, lr)
        want_g, want_t = pop.es_update_reference(th, w_np, obs_dim, sigma, lr, seed, gen, hidden=hidden)
        assert _np_bits(grad, want_g), lr
        assert _np_bits(new, want_t), lr
        assert not grad[mask].view(np.uint32).any() and _np_bits(new[mask], th[mask])          # padding: exactly 0, theta's own
        if lr == 0.0:
            assert _np_bits(new, th)                                                           # theta untouched
        else:
            assert (new[~mask] != th[~mask]).mean() > 0.9
    grad, new = run(np.full(P, 0.37, np.float32), 0.01)
    assert not grad.view(np.uint32).any() and _np_bits(new, th)                                # equal weights: all zero bits


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


@pytest.mark.parametrize("bounds", [None, (0, 16)])
def test_rollout_equals_a_host_loop_of_act_and_step_bit_for_bit(bounds):
    """32 environments, two members of 16, T = 6 with max_timesteps = 3: every environment auto-resets inside the window.  One chain on
    the caller's stream, and two chains of 16.  [64, 64, 64]: auv_population_rollout_arch against auv_population_act_arch + step."""
    T, hidden = 6, (64, 64, 64)
    a, b = _env(), _env()
    pa = pop.PolicyPopulation(a, 2, net=_net(a.obs_dim, hidden, seed=21), seed=3)
    pb = pop.PolicyPopulation(b, 2, net=_net(b.obs_dim, hidden, seed=21), seed=3)
    for p in (pa, pb):
        assert p.hidden == hidden and p._arch is not None and p.nf == pop.member_floats(a.obs_dim, hidden) == p.members.shape[1]
        p.perturb(0.05, 0)                                       # members that differ
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
    assert int(cnt.sum()) > 0 and bool(pa.ends.any()) and bool((fit != 0).any())               # episodes did end inside the window
    assert _bits(pa.actions, pb.actions) and _bits(a.obs, b.obs) and _bits(a.reward, b.reward) and torch.equal(a.done, b.done)
    for f in ("STATE", "COUNTERS", "WORLD_IDX"):
        assert torch.equal(a.read(f), b.read(f)), f
    assert _bits(fitness, fit.view(2, 16).mean(dim=1)) and torch.equal(ends, cnt.view(2, 16).sum(dim=1))
    a.close(), b.close()


# ---- 6. one ES generation on the device == the mirrors -----------------------------------------------------------------------------
def test_one_es_generation_on_the_device_equals_the_mirrors():
    hidden = (128, 64, 64)
    env = _env(64, max_timesteps=4)
    p = pop.PolicyPopulation(env, 4, net=_net(env.obs_dim, hidden, seed=5), seed=77)
    assert p.hidden == hidden and p._arch is not None
    sigma, lr, gen = 0.05, 0.02, 3
    th0 = p.theta.cpu().numpy()
    assert th0.shape == (pop.member_floats(env.obs_dim, hidden),) and not th0[pop.padding_mask(env.obs_dim, hidden)].any()
    p.perturb(sigma, gen)
    fitness, ends = p.rollout(5)
    w = p.centered_ranks(fitness)
    p.update(w, lr, sigma, gen)
    torch.cuda.synchronize()
    assert _np_bits(p.members.cpu().numpy(), pop.perturb_reference(th0, 4, env.obs_dim, sigma, 77, gen, hidden=hidden))
    wn = w.cpu().numpy()
    assert np.allclose(sorted(wn), np.linspace(-0.5, 0.5, 4))
    assert int(np.argmax(wn)) == int(torch.argmax(fitness))
    grad, new = pop.es_update_reference(th0, wn, env.obs_dim, sigma, lr, 77, gen, hidden=hidden)
    assert _np_bits(p.grad.cpu().numpy(), grad) and _np_bits(p.theta.cpu().numpy(), new)
    assert not np.array_equal(new, th0)
    # the champion through a FusedActorCritic of the same widths: predict() then gives the base block's deterministic action
    from gym_auv_amd.policy import FusedActorCritic
    fused = FusedActorCritic(_net(env.obs_dim, hidden, seed=6), env, rollout=2)
    p.base_state_into(fused)
    p.members.copy_(p.theta.unsqueeze(0).expand(4, p.stride))
    fused.predict()
    p.act()
    torch.cuda.synchronize()
    assert _bits(fused.actions, p.actions)
    with pytest.raises(ValueError):
        p.base_state_into(SimpleNamespace(env=env, hidden=DEFAULT, params=fused.params))              # other widths: refused
    env.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def _widest_obs_dim(hidden):
    """The largest obs_dim whose tiles fit the 160 KiB an entry allows: X [16][max(K0p, H2) + 8] and Y1 [16][max(H1, H3) + 8] floats
    (csrc/auv_policy_mfma.h), K0p = obs_dim rounded up to 32."""
    h1, h2, h3 = hidden
    k0p = (160 * 1024 // (4 * 16) - 8 - (max(h1, h3) + 8)) // 32 * 32
    assert k0p > h2
    return k0p


def test_refusals_enqueue_nothing():
    LIB = _lib()
    D, small, mid = 6, (64, 64, 64), (128, 128, 64)
    _, _, gapped = _blocks(D, small)
    nf_small, nf_mid = pop.member_floats(D, small), pop.member_floats(D, mid)
    members = gapped[:, :nf_small].contiguous()
    assert nf_small < nf_mid
    X = torch.rand((48, D), device=DEV)
    mu = torch.full((48, 2), CANARY, device=DEV)
    act = torch.full((48, 2), CANARY, device=DEV)
    out_members = torch.full((2, nf_small), CANARY, device=DEV)
    grad = torch.full((nf_small,), CANARY, device=DEV)
    theta = torch.as_tensor(_theta(D, small, 1), device=DEV)
    theta0 = theta.clone()
    w = torch.ones(2, device=DEV)

    def act_call(arch, **kw):
        io = _capi.AuvPopulationIO()
        io.members, io.stride, io.G = members.data_ptr(), nf_small, 16
        io.X, io.ldx, io.M, io.obs_dim, io.action_ld = X.data_ptr(), D, 48, D, 2
        io.mu, io.action, io.act, io.accumulate = mu.data_ptr(), act.data_ptr(), 1, 0
        for k_, x in kw.items():
            setattr(io, k_, x)
        return LIB.auv_population_act_arch(0, C.byref(io), None if arch is None else C.byref(_arch(arch)), None)

    def perturb_call(arch, stride=nf_small, obs_dim=D):
        return LIB.auv_population_perturb_arch(0, C.c_void_p(theta.data_ptr()), C.c_void_p(out_members.data_ptr()), stride, 2, obs_dim, 0.02, 1, 0,
                                               None if arch is None else C.byref(_arch(arch)), None)

    def update_call(arch, obs_dim=D):
        return LIB.auv_population_update_arch(0, C.c_void_p(theta.data_ptr()), C.c_void_p(w.data_ptr()), C.c_void_p(grad.data_ptr()), 2, obs_dim, 0.02,
                                              0.01, 1, 0, None if arch is None else C.byref(_arch(arch)), None)
    wide = _widest_obs_dim(small)
    assert wide == 2464 and _widest_obs_dim(mid) == 2400
    for name, rc in (("arch NULL", act_call(None)), ("(64, 64, 128)", act_call((64, 64, 128))), ("(256, 128, 128)", act_call((256, 128, 128))),
                     ("a [64, 64, 64] stride with [128, 128, 64]", act_call(mid)),
                     ("obs_dim past the LDS tile", act_call(small, obs_dim=wide + 1, ldx=wide + 1, stride=pop.member_floats(wide + 1, small))),
                     ("obs_dim past the [128, 128, 64] LDS tile", act_call(mid, obs_dim=2401, ldx=2401, stride=pop.member_floats(2401, mid))),
                     ("perturb: arch NULL", perturb_call(None)), ("perturb: (64, 64, 128)", perturb_call((64, 64, 128))),
                     ("perturb: (256, 128, 128)", perturb_call((256, 128, 128))), ("perturb: stride of another triple", perturb_call(mid)),
                     ("perturb: obs_dim past the LDS tile", perturb_call(small, stride=pop.member_floats(wide + 1, small), obs_dim=wide + 1)),
                     ("update: arch NULL", update_call(None)), ("update: (64, 64, 128)", update_call((64, 64, 128))),
                     ("update: (256, 128, 128)", update_call((256, 128, 128))), ("update: obs_dim past the LDS tile", update_call(small, obs_dim=wide + 1))):
        assert rc == EINVAL, (name, rc)
    torch.cuda.synchronize()
    assert bool((mu == CANARY).all()) and bool((act == CANARY).all()) and bool((out_members == CANARY).all()) and bool((grad == CANARY).all())
    assert _bits(theta, theta0)
    # the widest obs_dim itself passes every check (M = 0 launches nothing), and the call as it stands goes through
    assert act_call(small, obs_dim=wide, ldx=wide, stride=pop.member_floats(wide, small), M=0) == 0
    assert act_call(small) == 0
    torch.cuda.synchronize()
    assert not bool((mu == CANARY).any()) and not bool((act == CANARY).any())
    # the rollout entry: refused before a step is enqueued
    env = _env()
    p = pop.PolicyPopulation(env, 2, net=_net(env.obs_dim, small, seed=21), seed=3)
    st = torch.cuda.current_stream()
    ios = (p._io_type * 1)(p._io())
    for arch in (None, (64, 64, 128), (256, 128, 128), mid):
        rc = LIB.auv_population_rollout_arch(env._h, 1, (C.c_int32 * 2)(0, 32), (C.c_void_p * 1)(st.cuda_stream), ios,
                                             None if arch is None else C.byref(_arch(arch)), C.c_void_p(env.obs.data_ptr()),
                                             C.c_void_p(env.reward.data_ptr()), C.c_void_p(env.done.data_ptr()), 1, 1)
        assert rc == EINVAL, arch
    torch.cuda.synchronize()
    assert not bool(p.fit.any()) and int(env.read("COUNTERS")[:, 0].max()) == 0      # nothing stepped
    env.close()
    # the Python surface refuses what the entries would
    with pytest.raises(ValueError):
        pop.population_act(members, D, 16, X, hidden=(64, 64, 128))
    with pytest.raises(ValueError):
        pop.population_act(members, D, 16, X, hidden=mid)                                # blocks too small for these widths
