"""-m gpu: the supervised (clone) step of the fused updater (FusedPPOUpdate.clone_grad / clone_step, csrc/k8_ppo_update.hip: k8_clone)
against autograd of ppo_update.clone_loss_terms on the torch modules of examples/ppo.py.  Random tensors, 5000 stored rows.

Gradient parity, by the rule of tests/test_gpu_ppo_update.py: per parameter tensor e(x) = max |x - g64| / max |g64| with g64 = autograd
in fp64, g32 the same in fp32; required e(fused) <= max(8 e(g32), 1e-5), and the same bound per statistic."""
import copy
import functools
import os
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

DEV = "cuda:0"
N_ROWS, VF, ENT = 5000, 0.5, 0.01
NAMES = ["pi.W1", "pi.b1", "pi.W2", "pi.b2", "pi.W3", "pi.b3", "pi.W4", "pi.b4", "v.W1", "v.b1", "v.W2", "v.b2", "v.W3", "v.b3", "v.W4", "v.b4", "log_std"]


def ordered(net):
    """The module's parameters in the flat vector's order: policy net, value net, log_std."""
    return list(net.pi.parameters()) + list(net.v.parameters()) + [net.log_std]


def make_net(obs_dim, seed=0):
    import ppo
    torch.manual_seed(seed)
    net = ppo.ActorCritic(obs_dim).to(DEV)
    with torch.no_grad():
        net.log_std.copy_(torch.tensor([-0.5, -1.1]))
        for m in list(net.pi) + list(net.v):
            if isinstance(m, torch.nn.Linear):
                m.bias.uniform_(-0.3, 0.3)
    return net


def make_data(obs_dim, seed=1, n_rows=N_ROWS):
    """O, A, RET, W [n_rows]: about a quarter of the weights are zero, the others spread over (0, 2)."""
    torch.manual_seed(seed)
    O = torch.randn(n_rows, obs_dim, device=DEV)
    A = 0.5 * torch.randn(n_rows, 2, device=DEV)
    RET = torch.randn(n_rows, device=DEV)
    W = 2.0 * torch.rand(n_rows, device=DEV)
    W[torch.rand(n_rows, device=DEV) < 0.25] = 0.0
    return O, A, RET, W


@functools.lru_cache(maxsize=None)
def case(obs_dim):
    """Shared by every test of one width: the module, the rows, the updater (max_batch 4096).  Nothing here is modified afterwards."""
    from gym_auv_amd.ppo_update import FusedPPOUpdate
    net = make_net(obs_dim)
    data = make_data(obs_dim)
    upd = FusedPPOUpdate(net, vf_coef=VF, ent_coef=ENT, max_batch=4096)
    return net, data, upd


def autograd_reference(net, dtype, data, idx, kind, weighted):
    from gym_auv_amd.ppo_update import clone_loss_terms
    n = copy.deepcopy(net).to(dtype)
    o, a, ret, w = (x[idx].to(dtype) for x in data)
    if not weighted:
        w = torch.ones_like(w)
    loss, bc, vf = clone_loss_terms(n, o, a, ret, w, kind, VF, ENT)
    loss.backward()
    with torch.no_grad():
        dev = (a - n.pi(o)).abs().max(dim=1).values
        mx = torch.where(w > 0, dev, torch.zeros_like(dev)).max()
    stats = torch.stack([loss.detach(), bc.detach(), vf.detach(), mx, w.sum()])
    return [p.grad.double().reshape(-1) for p in ordered(n)], stats.double()


def split(flat, net):
    out, off = [], 0
    for p in ordered(net):
        out.append(flat[off:off + p.numel()].double())
        off += p.numel()
    assert off == flat.numel()
    return out


def err(x, ref):
    return float((x - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def assert_parity(net, data, upd, idx, kind, weighted, tag):
    g64, s64 = autograd_reference(net, torch.float64, data, idx, kind, weighted)
    g32, s32 = autograd_reference(net, torch.float32, data, idx, kind, weighted)
    O, A, RET, W = data
    g, stats = upd.clone_grad(O, A, RET, W if weighted else None, idx, kind=kind)
    gf, stats = split(g.clone(), net), stats.clone().double()
    worst = []
    for name, x, a, b in zip(NAMES, gf, g32, g64):
        ef, e32 = err(x, b), err(a, b)
        print("%s %-7s e(fused) %.3e e(g32) %.3e ratio %.2f" % (tag, name, ef, e32, ef / max(e32, 1e-30)))
        if not ef <= max(8 * e32, 1e-5):
            worst.append((name, ef, e32))
    assert not worst, worst
    for k in range(5):                                               # loss, bc, vf, max |a - mu|, the sum of the weights
        den = max(abs(float(s64[k])), 1e-30)
        ef, e32 = abs(float(stats[k] - s64[k])) / den, abs(float(s32[k] - s64[k])) / den
        print("%s stats[%d] %.9g fp64 %.9g e(fused) %.3e e(g32) %.3e" % (tag, k, float(stats[k]), float(s64[k]), ef, e32))
        assert ef <= max(8 * e32, 1e-5), (k, float(stats[k]), float(s64[k]), ef, e32)
    assert stats[5:].tolist() == [0.0, 0.0, 0.0]                     # no non-finite input; the two spare slots
    return gf, stats


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", ["nll", "mse"])
@pytest.mark.parametrize("B", [1, 15, 17, 33, 4095])
@pytest.mark.parametrize("obs_dim", [6, 15, 186])
def test_gradient_and_stats_match_autograd(obs_dim, B, kind, weighted):
    """B = 1, 15, 17, 33, 4095: a batch of one row; last row tiles of 15 rows and of one row after one, two and 255 full tiles."""
    net, data, upd = case(obs_dim)
    torch.manual_seed(100 + B)
    idx = torch.randperm(N_ROWS, device=DEV)[:B].contiguous()
    if weighted and B == 1:
        idx = (data[3] > 0).nonzero()[:1, 0].contiguous()             # (one row of weight zero has no gradient to compare)
    _, stats = assert_parity(net, data, upd, idx, kind, weighted, "obs_dim %3d B %4d %s w %d" % (obs_dim, B, kind, weighted))
    if not weighted:
        assert float(stats[4]) == float(B)
    elif B >= 33:
        assert float((data[3][idx] == 0).float().mean()) > 0.1       # the batch does hold rows of weight zero


@pytest.mark.parametrize("kind", ["nll", "mse"])
def test_repeated_rows_in_idx_count_every_time(kind):
    net, data, upd = case(15)
    idx = torch.tensor([3, 3, 3, 7, 7, 4999, 0, 3] * 4 + [7], device=DEV)      # 33 rows, five distinct
    assert_parity(net, data, upd, idx, kind, True, "repeats %s" % kind)


def test_gather_is_bit_identical_to_contiguous_rows():
    net, data, upd = case(15)
    torch.manual_seed(5)
    idx = torch.randperm(N_ROWS, device=DEV)[:1000].contiguous()
    g, s = upd.clone_grad(*data, idx)
    g, s = g.clone(), s.clone()
    packed = tuple(x[idx].contiguous() for x in data)
    g2, s2 = upd.clone_grad(*packed)
    assert torch.equal(g, g2) and torch.equal(s, s2)
    g3, s3 = upd.clone_grad(*(torch.cat([x, x[:7]]) for x in packed), B=1000)      # a prefix of stored rows, without idx
    assert torch.equal(g, g3) and torch.equal(s, s3)
    assert g.abs().max() > 0 and float(s[4]) > 0


@pytest.mark.parametrize("obs_dim,B,kind", [(186, 4096, "nll"), (6, 7, "mse")])
def test_two_calls_give_the_same_bits(obs_dim, B, kind):
    net, data, upd = case(obs_dim)
    idx = torch.arange(B, device=DEV) * (N_ROWS // B)
    g, s = upd.clone_grad(*data, idx, kind=kind)
    g, s = g.clone(), s.clone()
    g2, s2 = upd.clone_grad(*data, idx, kind=kind)
    assert torch.equal(g, g2) and torch.equal(s, s2)


@pytest.mark.parametrize("kind", ["nll", "mse"])
def test_rows_of_weight_zero_contribute_exactly_nothing(kind):
    """All weights zero: both nets' gradients are exactly 0, log_std's is exactly -ent_coef (the entropy term alone)."""
    net, data, upd = case(15)
    O, A, RET, W = data
    idx = torch.arange(0, 100, device=DEV)
    g, s = upd.clone_grad(O, A, RET, torch.zeros_like(W), idx, kind=kind)
    assert torch.equal(g[:-2], torch.zeros_like(g[:-2]))
    assert g[-2:].tolist() == [-float(torch.tensor(ENT, dtype=torch.float32))] * 2
    assert s[1:5].tolist() == [0.0, 0.0, 0.0, 0.0]                   # bc, vf, max |a - mu| over no row, the sum of the weights


def test_non_finite_inputs_are_counted_exactly():
    """stats[5] = the number of non-finite values among the GATHERED rows of O, A, RET and W (W only when it is given)."""
    net, data, upd = case(15)
    O, A, RET, W = (x.clone() for x in data)
    idx = torch.arange(0, 200, 2, device=DEV)                        # rows 0, 2, .., 198: seven row tiles of 16
    nan, inf = float("nan"), float("inf")
    O[0, 0], O[0, 14], O[34, 7], O[198, 3] = nan, inf, -inf, nan     # 4, in the first, a middle and the last (ragged) tile
    A[2, 0], A[2, 1], A[66, 1] = nan, inf, nan                       # 3, both components of one row, the second alone
    RET[130], RET[196] = -inf, nan                                   # 2
    W[4], W[100], W[198] = inf, nan, nan                             # 3
    O[1, 0], A[3, 1], RET[4999], W[5], W[199] = nan, nan, nan, inf, nan         # odd rows, and rows past the minibatch: not gathered
    _, stats = upd.clone_grad(O, A, RET, W, idx)
    assert float(stats[5]) == 12.0, float(stats[5])
    _, stats = upd.clone_grad(O, A, RET, None, idx, kind="mse")
    assert float(stats[5]) == 9.0, float(stats[5])
    _, stats = upd.clone_grad(*data, idx)
    assert float(stats[5]) == 0.0


def test_arguments_are_refused_with_a_message():
    net, data, upd = case(6)
    O, A, RET, W = data
    with pytest.raises(RuntimeError, match="max_batch"):
        upd.clone_grad(O, A, RET, W, torch.arange(4097, device=DEV) % N_ROWS)
    with pytest.raises(ValueError, match="kind"):
        upd.clone_grad(O, A, RET, W, kind="huber")
    with pytest.raises(ValueError):
        upd.clone_grad(O.double(), A, RET)
    with pytest.raises(ValueError):
        upd.clone_grad(O, A, RET, W[:-1].contiguous())
    with pytest.raises(ValueError):
        upd.clone_grad(O, A[:, :1].contiguous(), RET)


def expected_policy_buffer(net, obs_dim):
    """What FusedActorCritic.refresh() packs from the module (gym_auv_amd/policy.py): pack_linear per layer, biases, log_std."""
    from gym_auv_amd import _capi
    from gym_auv_amd.policy import pack_linear, _pad16
    lib = _capi.load_library()
    p = torch.zeros(int(lib.auv_policy_param_floats(obs_dim)), device=DEV)
    off = 0
    for seq in (net.pi, net.v):
        for j, l in enumerate(m for m in seq if isinstance(m, torch.nn.Linear)):
            out_p, in_p = (l.out_features if j < 3 else 16), (_pad16(obs_dim) if j == 0 else l.in_features)
            p[off:off + out_p * in_p].copy_(pack_linear(l.weight.detach(), out_p, in_p))
            off += out_p * in_p
            p[off:off + l.out_features].copy_(l.bias.detach())
            off += out_p
    p[off:off + 2].copy_(net.log_std.detach())
    assert off + 4 == p.numel()
    return p


def test_a_clone_step_moves_the_packed_copies_and_the_attached_policy_buffer():
    """A clone step then a PPO step on one updater = the PPO step on a fresh updater load()ed with the intermediate theta (and
    Adam's state), bit for bit: the forward and transposed copies follow the clone step.  The attached policy buffer is bitwise
    what refresh() would pack, after every clone step."""
    from gym_auv_amd import _capi
    from gym_auv_amd.ppo_update import FusedPPOUpdate
    obs_dim = 15
    net, net2 = make_net(obs_dim, seed=3), make_net(obs_dim, seed=4)
    O, A, RET, W = make_data(obs_dim, seed=2, n_rows=300)
    torch.manual_seed(9)
    LP, ADV = -1.0 + 0.1 * torch.randn(300, device=DEV), torch.randn(300, device=DEV)
    upd = FusedPPOUpdate(net, lr=1e-3, vf_coef=VF, ent_coef=ENT, max_batch=256)
    buf = torch.zeros(int(_capi.load_library().auv_policy_param_floats(obs_dim)), device=DEV)
    upd.attach(types.SimpleNamespace(bf16=False, env=types.SimpleNamespace(obs_dim=obs_dim), params=buf))
    idx = torch.arange(3, 203, device=DEV)
    before = upd.theta.clone()
    for step, kind in enumerate(("nll", "mse")):
        row = upd.clone_step(O, A, RET, W, idx, kind=kind)
        assert row[8] > 0 and row[9] > 0 and upd.n_steps == step + 1
        assert torch.equal(buf, expected_policy_buffer(net, obs_dim)), step
    assert not torch.equal(before, upd.theta)
    fresh = FusedPPOUpdate(net2, lr=1e-3, vf_coef=VF, ent_coef=ENT, max_batch=256)
    fresh.theta.copy_(upd.theta), fresh.m.copy_(upd.m), fresh.v.copy_(upd.v)
    fresh.t = upd.t
    fresh.load()
    r1 = upd.step(O, A, LP, ADV, RET, idx).clone()
    g1 = upd.g.clone()
    r2 = fresh.step(O, A, LP, ADV, RET, idx).clone()
    assert torch.equal(g1, fresh.g) and torch.equal(r1, r2) and torch.equal(upd.theta, fresh.theta)
    assert torch.equal(buf, expected_policy_buffer(net, obs_dim))


@pytest.mark.parametrize("kind", ["nll", "mse"])
def test_fifty_clone_steps_descend_like_torch_adam(kind):
    """A seeded teacher at obs_dim 15, 2048 rows, 50 steps at B 256 (no norm clipping: the twin has none).  The twin starts from the
    same weights and sees the same minibatches with clone_loss_terms and torch.optim.Adam.  Required: final loss on all rows
    <= the twin's + 10 % of the twin's improvement -- the margin of two Adam trajectories that differ by rounding."""
    from gym_auv_amd.ppo_update import FusedPPOUpdate, clone_loss_terms
    obs_dim, n_rows, B, lr = 15, 2048, 256, 1e-3
    teacher, net = make_net(obs_dim, seed=21), make_net(obs_dim, seed=22)
    twin = copy.deepcopy(net)
    torch.manual_seed(23)
    with torch.no_grad():
        O = torch.randn(n_rows, obs_dim, device=DEV)
        A = (teacher.pi(O) + 0.1 * torch.randn(n_rows, 2, device=DEV)).contiguous()
        RET = teacher.v(O).squeeze(-1).contiguous()
        W = (0.5 + torch.rand(n_rows, device=DEV)).contiguous()

    def total(n):
        with torch.no_grad():
            return float(clone_loss_terms(n, O, A, RET, W, kind, VF, ENT)[0])
    initial = total(twin)
    upd = FusedPPOUpdate(net, lr=lr, vf_coef=VF, ent_coef=ENT, max_norm_pi=0.0, max_norm_v=0.0, max_batch=B)
    opt = torch.optim.Adam(ordered(twin), lr=lr)
    gen = torch.Generator(device=DEV).manual_seed(24)
    for _ in range(50):
        idx = torch.randint(0, n_rows, (B,), generator=gen, device=DEV)
        upd.clone_step(O, A, RET, W, idx, kind=kind)
        opt.zero_grad()
        clone_loss_terms(twin, O[idx], A[idx], RET[idx], W[idx], kind, VF, ENT)[0].backward()
        opt.step()
    fused, ref = total(net), total(twin)
    print("%s: initial %.6f twin %.6f fused %.6f (non-finite inputs seen: %d)" % (kind, initial, ref, fused, int(upd.log[:50, 5].sum())))
    assert initial - ref > 0.05 * abs(initial), (initial, ref)      # the twin did descend
    assert fused <= ref + 0.1 * (initial - ref), (initial, ref, fused)
