"""-m gpu: the fused PPO update (gym_auv_amd/ppo_update.py, csrc/k8_ppo_update.hip) against autograd on the torch modules of
examples/ppo.py, for the reference's architecture (scripts/run.py:332-357).  No environment handle: random tensors, 5000 stored rows.

Gradient parity: per parameter tensor e(x) = max |x - g64| / max |g64| with g64 = autograd on the module in fp64, g32 the same in fp32;
required e(fused) <= max(8 e(g32), 1e-5) (8x: another summation order and pol_tanh's 2e-7 against libm; 1e-5: DESIGN section 2).  A row
within rounding of a clip boundary flips branch between precisions, so such rows are replaced before anything is compared."""
import copy
import functools
import math
import os
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

DEV = "cuda:0"
N_ROWS, CLIP, VF, ENT = 5000, 0.2, 0.5, 0.01


def ordered(net):
    """The module's parameters in the flat vector's order: policy net, value net, log_std."""
    return list(net.pi.parameters()) + list(net.v.parameters()) + [net.log_std]


def make_net(obs_dim, seed=0, device=DEV):
    import ppo
    torch.manual_seed(seed)
    net = ppo.ActorCritic(obs_dim).to(device)
    with torch.no_grad():
        net.log_std.copy_(torch.tensor([-0.5, -1.1]))
        for m in list(net.pi) + list(net.v):
            if isinstance(m, torch.nn.Linear):
                m.bias.uniform_(-0.3, 0.3)
    return net


def loss_terms(net, o, a, lp, adv, ret):
    """minibatch_step's loss (examples/ppo.py), and what its diagnostics row holds."""
    mu = net.pi(o)
    ratio = (net.log_prob(mu, a) - lp).exp()
    pg = -torch.min(ratio * adv, ratio.clamp(1 - CLIP, 1 + CLIP) * adv).mean()
    vf = 0.5 * (net.v(o).squeeze(-1) - ret).pow(2).mean()
    loss = pg + VF * vf - ENT * net.entropy()
    return loss, pg, vf, ratio


def make_data(net, obs_dim, seed=1, device=DEV, n_rows=N_ROWS):
    """O, A, LP, ADV, RET [n_rows]: actions sampled from the net, LP from a slightly perturbed copy of it, so that the ratios spread
    over both clip boundaries; rows within 1e-4 of a boundary (in fp64) or with |adv| < 1e-6 are replaced by rows at ratio 1."""
    torch.manual_seed(seed)
    with torch.no_grad():
        O = torch.randn(n_rows, obs_dim, device=device)
        mu = net.pi(O)
        A = mu + net.log_std.exp() * torch.randn_like(mu)
        old = copy.deepcopy(net)
        for p in old.pi.parameters():
            p.add_(0.15 * torch.randn_like(p) * p.abs().max())
        old.log_std.add_(torch.tensor([0.03, -0.03], device=device))
        LP = old.log_prob(old.pi(O), A)
        ADV, RET = torch.randn(n_rows, device=device), torch.randn(n_rows, device=device)
        n64 = copy.deepcopy(net).double()

        def ratio64():
            return (n64.log_prob(n64.pi(O.double()), A.double()) - LP.double()).exp()
        r = ratio64()
        near = ((r - (1 - CLIP)).abs() < 1e-4) | ((r - (1 + CLIP)).abs() < 1e-4) | (ADV.abs() < 1e-6)
        LP[near] = (LP.double() + r.log())[near].float()            # ratio 1 up to fp32 rounding of LP
        ADV[near] = 1.0
        r = ratio64()
        assert not (((r - (1 - CLIP)).abs() < 1e-4) | ((r - (1 + CLIP)).abs() < 1e-4) | (ADV.abs() < 1e-6)).any()
        assert (r < 1 - CLIP).float().mean() > 0.02 and (r > 1 + CLIP).float().mean() > 0.02
    return O, A, LP, ADV, RET


def autograd_reference(net, dtype, data, idx):
    n = copy.deepcopy(net).to(dtype)
    o, a, lp, adv, ret = ((x if idx is None else x[idx]).to(dtype) for x in data)                # (idx None: every stored row)
    loss, pg, vf, ratio = loss_terms(n, o, a, lp, adv, ret)
    loss.backward()
    clipped = ((adv > 0) & (ratio > 1 + CLIP)) | ((adv < 0) & (ratio < 1 - CLIP))
    stats = torch.stack([loss.detach(), pg.detach(), vf.detach(), adv.abs().max(), ratio.detach().max(), clipped.to(dtype).mean()])
    return [p.grad.double().reshape(-1) for p in ordered(n)], stats.double()


@functools.lru_cache(maxsize=None)
def case(obs_dim):
    """Shared by every test of one width: the module, the rows, the updater (max_batch 4096).  Nothing here is modified afterwards."""
    from gym_auv_amd.ppo_update import FusedPPOUpdate
    net = make_net(obs_dim)
    data = make_data(net, obs_dim)
    upd = FusedPPOUpdate(net, clip=CLIP, vf_coef=VF, ent_coef=ENT, max_batch=4096)
    return net, data, upd


def split(flat, net):
    out, off = [], 0
    for p in ordered(net):
        out.append(flat[off:off + p.numel()].double())
        off += p.numel()
    assert off == flat.numel()
    return out


def err(x, ref):
    return float((x - ref).abs().max() / ref.abs().max())


NAMES = ["pi.W1", "pi.b1", "pi.W2", "pi.b2", "pi.W3", "pi.b3", "pi.W4", "pi.b4", "v.W1", "v.b1", "v.W2", "v.b2", "v.W3", "v.b3", "v.W4", "v.b4", "log_std"]


def assert_parity(net, data, upd, idx, tag, names=NAMES):
    """upd.grad on rows idx against autograd in fp64 by the rule of the module's docstring, for the tensors `names` and for the
    statistics; every figure is printed before it is asserted.  Returns the fused gradient per tensor, the statistics row (copies,
    as float64) and the reference gradients in fp64 and fp32."""
    g64, s64 = autograd_reference(net, torch.float64, data, idx)
    g32, s32 = autograd_reference(net, torch.float32, data, idx)
    g, stats = upd.grad(*data, idx)
    gf, stats = split(g.clone(), net), stats.clone().double()
    worst = []
    for name, x, a, b in zip(NAMES, gf, g32, g64):
        if name not in names:
            continue
        ef, e32 = err(x, b), err(a, b)
        print("%s %-7s e(fused) %.3e e(g32) %.3e ratio %.2f" % (tag, name, ef, e32, ef / max(e32, 1e-30)))
        if not ef <= max(8 * e32, 1e-5):
            worst.append((name, ef, e32))
    assert not worst, worst
    # loss, pg, vf, max |adv|, max ratio, the clipped fraction: the same bound
    for j, k in enumerate((0, 1, 2, 3, 4, 6)):
        den = max(abs(float(s64[j])), 1e-30)                         # (a clipped fraction of 0 in a small batch: then exactly 0)
        ef, e32 = abs(float(stats[k] - s64[j])) / den, abs(float(s32[j] - s64[j])) / den
        print("%s stats[%d] %.9g fp64 %.9g e(fused) %.3e e(g32) %.3e" % (tag, k, float(stats[k]), float(s64[j]), ef, e32))
        assert ef <= max(8 * e32, 1e-5), (k, float(stats[k]), float(s64[j]), ef, e32)
    return gf, stats, g64, g32


@pytest.mark.parametrize("B", [1, 7, 15, 16, 17, 33, 1000, 4095, 4096])
@pytest.mark.parametrize("obs_dim", [6, 15, 186])
def test_gradient_and_stats_match_autograd(obs_dim, B):
    """B = 1, 15, 17, 33, 4095: a batch of one row; last row tiles of 15 rows and of one row after one, two and 255 full tiles."""
    net, data, upd = case(obs_dim)
    torch.manual_seed(100 + B)
    idx = torch.randperm(N_ROWS, device=DEV)[:B].contiguous()
    _, stats, _, _ = assert_parity(net, data, upd, idx, "obs_dim %3d B %4d" % (obs_dim, B))
    assert float(stats[5]) == 0.0 and float(stats[7]) == 0.0         # no non-finite input; the spare slot
    if B >= 1000:
        assert 0.0 < float(stats[6]) < 1.0


def test_gather_is_bit_identical_to_contiguous_rows():
    net, data, upd = case(15)
    torch.manual_seed(5)
    idx = torch.randperm(N_ROWS, device=DEV)[:1000].contiguous()
    g, s = upd.grad(*data, idx)
    g, s = g.clone(), s.clone()
    packed = tuple(x[idx].contiguous() for x in data)
    g2, s2 = upd.grad(*packed, None)
    assert torch.equal(g, g2) and torch.equal(s, s2)
    assert float(s[6]) > 0.0 and g.abs().max() > 0


@pytest.mark.parametrize("obs_dim,B", [(186, 4096), (6, 7)])
def test_two_calls_give_the_same_bits(obs_dim, B):
    net, data, upd = case(obs_dim)
    idx = torch.arange(B, device=DEV) * (N_ROWS // B)
    g, s = upd.grad(*data, idx)
    g, s = g.clone(), s.clone()
    g2, s2 = upd.grad(*data, idx)
    assert torch.equal(g, g2) and torch.equal(s, s2)


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


def assert_adam_step(upd, net, tp, opt, before, step, say=True):
    """One step of the updater against the same step of torch.optim.Adam on the twin's parameters `tp` (`before`: their values in
    front of the step), by the rules of test_clip_and_adam_match_torch_and_repack_the_policy_buffer.  Returns the largest
    difference of a parameter element in ulp."""
    off, worst = 0, 0.0
    for p, q, p0 in zip(tp, ordered(net), before):
        sl = slice(off, off + p.numel())
        off += p.numel()
        assert q.data_ptr() == upd.theta[sl].data_ptr() and torch.equal(q.detach().reshape(-1), upd.theta[sl])
        st = opt.state[p]
        assert torch.allclose(upd.m[sl], st["exp_avg"].reshape(-1), rtol=2e-6, atol=1e-30), step
        assert torch.allclose(upd.v[sl], st["exp_avg_sq"].reshape(-1), rtol=2e-6, atol=1e-30), step
        p1 = p.detach()
        scale = torch.maximum(torch.maximum(p0.abs(), p1.abs()), (p1 - p0).abs())
        ulp = torch.exp2(torch.floor(torch.log2(scale.double())) - 23)          # float32 spacing at `scale`
        n_ulp = (q.detach().double() - p1.double()).abs() / ulp
        if say:
            print("step %d %-12s largest difference %.2f ulp, %d of %d elements differ" % (step, tuple(p.shape), float(n_ulp.max()), int((n_ulp > 0).sum()), p.numel()))
        assert float(n_ulp.max()) <= 2.0, (step, tuple(p.shape), float(n_ulp.max()))
        worst = max(worst, float(n_ulp.max()))
    assert off == upd.theta.numel()
    return worst


def test_clip_and_adam_match_torch_and_repack_the_policy_buffer():
    """Three steps on a fixed random gradient (policy group clipped, value group not) against examples/ppo.clip_grad_norm +
    torch.optim.Adam on a twin.  Norms rtol 1e-6, m and v rtol 2e-6, every parameter within 2 ulp of the twin's, PER ELEMENT: the ulp
    is the float32 spacing at max(|p before the step|, |p after it|, |the step|) of the twin's element -- the operands and the result of
    `p -= step`; the step's size sets the scale for an element that is carried to or across zero, which has no ulp of its own to measure
    a last-bit difference of the step against.  The attached policy buffer is BITWISE what refresh() would pack, after load and after
    every step; the module's parameters are views of the flat vector."""
    import ppo
    from gym_auv_amd import _capi
    from gym_auv_amd.ppo_update import FusedPPOUpdate
    obs_dim = 15
    net = make_net(obs_dim, seed=3)
    twin = copy.deepcopy(net)
    upd = FusedPPOUpdate(net, lr=2e-4, max_norm_pi=0.5, max_norm_v=0.5, max_batch=64)
    buf = torch.zeros(int(_capi.load_library().auv_policy_param_floats(obs_dim)), device=DEV)
    upd.attach(types.SimpleNamespace(bf16=False, env=types.SimpleNamespace(obs_dim=obs_dim), params=buf))
    assert torch.equal(buf, expected_policy_buffer(net, obs_dim))
    n_pi = sum(p.numel() for p in net.pi.parameters())
    n_v = sum(p.numel() for p in net.v.parameters())
    torch.manual_seed(11)
    g = torch.randn(upd.theta.numel(), device=DEV)
    g[:n_pi] *= 5.0 / g[:n_pi].norm()                               # (with log_std: a little above 5 -> clipped at 0.5)
    g[n_pi:n_pi + n_v] *= 0.1 / g[n_pi:n_pi + n_v].norm()           # 0.1 < 0.5: not clipped
    tp = ordered(twin)
    opt = torch.optim.Adam(tp, lr=2e-4)
    pi_t, v_t = list(twin.pi.parameters()) + [twin.log_std], list(twin.v.parameters())
    for step in range(3):
        off = 0
        for p in tp:
            p.grad = g[off:off + p.numel()].view_as(p).clone()
            off += p.numel()
        norms_t = torch.stack([ppo.clip_grad_norm(pi_t, 0.5), ppo.clip_grad_norm(v_t, 0.5)])
        before = [p.detach().clone() for p in tp]
        opt.step()
        norms = upd.apply(g).clone()
        assert norms_t[0] > 0.5 > norms_t[1]
        assert torch.allclose(norms, norms_t, rtol=1e-6, atol=0), (norms, norms_t)
        assert_adam_step(upd, net, tp, opt, before, step)
        assert torch.equal(buf, expected_policy_buffer(net, obs_dim)), step
    # the updater's own forward copy follows too: a gradient after the steps is the gradient AT the updated weights
    data = make_data(net, obs_dim, seed=2)
    idx = torch.arange(64, device=DEV)
    upd.grad(*data, idx)
    g64, _ = autograd_reference(net, torch.float64, data, idx)
    g32, _ = autograd_reference(net, torch.float32, data, idx)
    for x, a, b in zip(split(upd.g.clone(), net), g32, g64):
        assert err(x, b) <= max(8 * err(a, b), 1e-5)


def test_non_finite_inputs_are_counted_exactly():
    """stats[5] = the number of non-finite values among the GATHERED rows of O, A, LP, ADV, RET: planted in several row tiles, in
    both action components, in rows inside and outside the minibatch."""
    net, data, upd = case(15)
    O, A, LP, ADV, RET = (x.clone() for x in data)
    idx = torch.arange(0, 200, 2, device=DEV)                        # rows 0, 2, .., 198: seven row tiles of 16
    nan, inf = float("nan"), float("inf")
    O[0, 0], O[0, 14], O[34, 7], O[198, 3] = nan, inf, -inf, nan     # 4, in the first, a middle and the last (ragged) tile
    A[2, 0], A[2, 1], A[66, 1] = nan, inf, nan                       # 3, both components of one row, the second alone
    LP[4], ADV[100], RET[130], RET[196] = inf, nan, -inf, nan        # 4
    O[1, 0], A[3, 1], LP[5], ADV[199], RET[4999] = nan, nan, nan, inf, nan      # odd rows, and rows past the minibatch: not gathered
    _, stats = upd.grad(O, A, LP, ADV, RET, idx)
    assert float(stats[5]) == 11.0, float(stats[5])
    _, stats = upd.grad(*data, idx)
    assert float(stats[5]) == 0.0


@pytest.mark.parametrize("dims", [(400, 600)])
def test_wide_observations_use_more_than_64_kib_of_lds_per_updater(dims):
    """obs_dim 400 and 600: the row pass' LDS tile is 73 and 86 KiB, above the 64 KiB a kernel gets without asking.  Two live
    updaters of different width, the narrower used AFTER the wider was created and used: each launch asks for its own size."""
    from gym_auv_amd.ppo_update import FusedPPOUpdate
    made = []
    for D in dims:
        net = make_net(D)
        made.append((net, make_data(net, D), FusedPPOUpdate(net, clip=CLIP, vf_coef=VF, ent_coef=ENT, max_batch=100)))
    idx = torch.arange(100, device=DEV) * 7
    for net, data, upd in reversed(made):
        g64, _ = autograd_reference(net, torch.float64, data, idx)
        g32, _ = autograd_reference(net, torch.float32, data, idx)
        g, _ = upd.grad(*data, idx)
        for x, a, b in zip(split(g.clone(), net), g32, g64):
            assert err(x, b) <= max(8 * err(a, b), 1e-5), (net.pi[0].in_features, err(x, b), err(a, b))


def test_arguments_are_refused_with_a_message():
    net, data, upd = case(6)
    with pytest.raises(RuntimeError, match="max_batch"):
        upd.grad(*data, torch.arange(4097, device=DEV) % N_ROWS)
    with pytest.raises(RuntimeError, match="16-byte"):
        upd.attach(types.SimpleNamespace(bf16=False, env=types.SimpleNamespace(obs_dim=6), params=torch.zeros(70000, device=DEV)[1:]))
    with pytest.raises(ValueError):
        upd.grad(data[0].double(), *data[1:])


def test_training_with_the_fused_update_moves_the_weights_and_keeps_the_policy_buffer_in_step(monkeypatch):
    import ppo
    from gym_auv_amd.ppo_update import FusedPPOUpdate
    keep = {}
    attach = FusedPPOUpdate.attach

    def recording_attach(self, fused=None):                          # (train() returns its history only: catch the objects it builds)
        keep.update(net=self.net, fused=fused, updater=self)
        return attach(self, fused)
    monkeypatch.setattr(FusedPPOUpdate, "attach", recording_attach)
    hist = ppo.train(task="pathfollow", envs=256, updates=3, rollout=16, minibatches=4, fused_update=True, log=lambda *_: None)
    assert len(hist) == 3
    w = [h["weight_l1"] for h in hist]
    assert all(abs(b - a) > 1e-3 for a, b in zip(w[:-1], w[1:])), w   # every update moves the weights (rounds 2-3 froze them silently)
    assert all(h["minibatch_steps_nonfinite"] == 0 and h["minibatch_steps"] == 16 for h in hist)
    assert all(math.isfinite(h["loss"]) and h["grad_norm_pi"] > 0 and h["grad_norm_v"] > 0 and h["max_ratio"] > 0 for h in hist)
    net, fused = keep["net"], keep["fused"]
    assert keep["updater"].n_steps == 48
    assert torch.equal(fused.params, expected_policy_buffer(net, fused.env.obs_dim))
