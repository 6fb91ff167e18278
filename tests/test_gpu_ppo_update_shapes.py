"""-m gpu: the fused PPO update at the batch sizes the trainer runs, in every split regime of the weight-gradient pass, on degenerate
minibatches, and clip + Adam + repack at every width and option.  Helpers, data and the parity rule are those of
test_gpu_ppo_update.py: e(fused) <= max(8 e(g32), 1e-5) per tensor against autograd on the torch modules of examples/ppo.py in fp64.

Split factors.  ppo_nsplit (csrc/k8_ppo_update.hip) = max(ceil(rt / 64), min(ceil(512 / blocks), ceil(rt / 4))) clamped to [1, 16] with
rt = ceil(B / 16) row tiles; blocks = 114 at obs_dim 15, 178 at obs_dim 186, so the middle term is at most 5 and 3.  Each B below is
meant to reach (the same at both widths; re-derive them if the formula changes):
    B = 16384  1024 tiles  split 16, not clamped; 16 tiles per wave (examples/ppo.py --fused-update in the documented shapes)
    B = 15361   961 tiles  the first size with split 16; the last tile holds one row
    B = 16400  1025 tiles  17 clamped to 16: the last split ends at the end of the partials' allocation; 17 tiles per wave, wave 60 of
                           64 gets 5 tiles, waves 61-63 none; the statistics loop of k8_reduce makes five trips
    B =  8200   513 tiles  split 9: 15 tiles per wave, wave 34 of 36 gets 3, wave 35 none
    B =  6000   375 tiles  split 6
The parametrisation of test_gradient_and_stats_match_autograd covers splits 1, 3, 4 and 5.

Per-column metric of the first layer (test_first_layer_gradient_is_right_in_every_input_column): measured on the MI355X, the worst
e_k(fused) / e_k(g32) over the 186 columns is 2.27 for pi.W1 and 1.73 for v.W1 (medians 0.67 and 0.58, no
outlier column); the factor in use is F = 8, the project's."""
import copy
import functools
import math
import os
import sys
import types

import pytest
import torch

import test_gpu_ppo_update as base
from test_gpu_ppo_update import CLIP, DEV, ENT, VF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

N_BIG, MAX_BIG = 20000, 16400
V_TENSORS = base.NAMES[8:16]


@functools.lru_cache(maxsize=None)
def big_case(obs_dim):
    """Shared by every test of the workload's sizes: the module, 20000 stored rows, an updater with max_batch 16400, and one
    permutation of the rows.  Nothing here is modified afterwards."""
    from gym_auv_amd.ppo_update import FusedPPOUpdate
    net = base.make_net(obs_dim)
    data = base.make_data(net, obs_dim, n_rows=N_BIG)
    upd = FusedPPOUpdate(net, clip=CLIP, vf_coef=VF, ent_coef=ENT, max_batch=MAX_BIG)
    torch.manual_seed(77)
    return net, data, upd, torch.randperm(N_BIG, device=DEV)


def new_updater(net, **kw):
    from gym_auv_amd.ppo_update import FusedPPOUpdate
    kw.setdefault("max_batch", 4096)
    return FusedPPOUpdate(net, clip=CLIP, vf_coef=VF, ent_coef=ENT, **kw)


# ------------------------------------------------------------------------------------------------- 1. sizes and split regimes
@pytest.mark.parametrize("B", [16384, 15361, 16400, 8200, 6000])
@pytest.mark.parametrize("obs_dim", [15, 186])
def test_gradient_and_stats_match_autograd_at_the_workloads_sizes(obs_dim, B):
    """Splits 16, 16 (first), 16 (clamped from 17), 9 and 6: see the module's docstring."""
    net, data, upd, perm = big_case(obs_dim)
    idx = perm[(B % 1000):(B % 1000) + B].contiguous()
    _, stats, _, _ = base.assert_parity(net, data, upd, idx, "obs_dim %3d B %5d" % (obs_dim, B))
    assert float(stats[5]) == 0.0 and float(stats[7]) == 0.0
    assert 0.0 < float(stats[6]) < 1.0


def test_two_calls_give_the_same_bits_with_the_clamped_split():
    net, data, upd, perm = big_case(186)
    idx = perm[:MAX_BIG].contiguous()
    g, s = upd.grad(*data, idx)
    g, s = g.clone(), s.clone()
    g2, s2 = upd.grad(*data, idx)
    assert torch.equal(g, g2) and torch.equal(s, s2)
    assert g.abs().max() > 0


def test_gather_is_bit_identical_to_contiguous_rows_with_the_clamped_split():
    net, data, upd, perm = big_case(186)
    idx = perm[N_BIG - MAX_BIG:].contiguous()
    g, s = upd.grad(*data, idx)
    g, s = g.clone(), s.clone()
    packed = tuple(x[idx].contiguous() for x in data)
    g2, s2 = upd.grad(*packed, None)
    assert torch.equal(g, g2) and torch.equal(s, s2)
    assert float(s[6]) > 0.0 and g.abs().max() > 0


# ------------------------------------------------------------------------------- 2. statistics across more than 256 row tiles
def gathered(idx, tile, r):
    """The stored row that lands in row r of row tile `tile`."""
    return int(idx[16 * tile + r])


def test_non_finite_inputs_are_counted_exactly_across_1025_row_tiles():
    """As test_non_finite_inputs_are_counted_exactly, on 16400 rows: planted in tiles 0, 255, 256 (the second trip of k8_reduce's
    statistics loop begins there), 700 and 1024 (the last tile, 16 rows), in observation columns on both sides of the gather loop's
    stride of 32, and in rows that are stored but not gathered."""
    net, data, upd, perm = big_case(186)
    idx = perm[:MAX_BIG].contiguous()
    O, A, LP, ADV, RET = (x.clone() for x in data)
    nan, inf = float("nan"), float("inf")
    n = 0
    for tile, r in ((0, 0), (255, 15), (256, 0), (700, 7), (1024, 15)):           # every tile x every column: 25
        for col, v in ((0, nan), (31, inf), (32, -inf), (100, nan), (185, inf)):
            O[gathered(idx, tile, r), col] = v
            n += 1
    A[gathered(idx, 256, 3), 0], A[gathered(idx, 256, 3), 1], A[gathered(idx, 1024, 0), 1], A[gathered(idx, 0, 9), 0] = nan, inf, nan, -inf
    LP[gathered(idx, 255, 1)], LP[gathered(idx, 1024, 8)] = inf, nan
    ADV[gathered(idx, 700, 2)], ADV[gathered(idx, 256, 15)] = nan, -inf
    RET[gathered(idx, 0, 5)], RET[gathered(idx, 1024, 15)], RET[gathered(idx, 511, 4)] = -inf, nan, inf
    n += 4 + 2 + 2 + 3
    rest = perm[MAX_BIG:]                                              # stored, not gathered
    for j, col in enumerate((0, 31, 32, 100, 185)):
        O[int(rest[j]), col] = nan
    A[int(rest[5]), 0], A[int(rest[5]), 1], LP[int(rest[6])], ADV[int(rest[7])], RET[int(rest[8])] = nan, inf, -inf, nan, inf
    _, stats = upd.grad(O, A, LP, ADV, RET, idx)
    assert float(stats[5]) == float(n) == 36.0, float(stats[5])
    _, stats = upd.grad(*data, idx)
    assert float(stats[5]) == 0.0


def test_maximum_advantage_and_ratio_are_found_past_256_row_tiles():
    net, data, upd, perm = big_case(186)
    idx = perm[:MAX_BIG].contiguous()
    O, A, LP, ADV, RET = (x.clone() for x in data)
    assert float(ADV[idx].abs().max()) < 37.5
    ADV[gathered(idx, 700, 3)] = 37.5
    _, stats = upd.grad(O, A, LP, ADV, RET, idx)
    assert float(stats[3]) == 37.5
    # one row of tile 300 at ratio 3.0; every other gathered row above 2.5 is moved to ratio 1, so that this row holds the maximum
    ADV = data[3].clone()
    n64 = copy.deepcopy(net).double()
    with torch.no_grad():
        lp64 = n64.log_prob(n64.pi(O[idx].double()), A[idx].double())
        r = (lp64 - LP[idx].double()).exp()
        high = r > 2.5
        high[16 * 300 + 5] = True
        target = torch.ones_like(r)
        target[16 * 300 + 5] = 3.0
        LP[idx[high]] = (lp64 - target.log())[high].float()
        r = (lp64 - LP[idx].double()).exp()
        assert int(r.argmax()) == 16 * 300 + 5 and abs(float(r.max()) - 3.0) < 1e-3 and float(r.topk(2).values[1]) <= 2.5
    d2 = (O, A, LP, ADV, RET)
    _, s64 = base.autograd_reference(net, torch.float64, d2, idx)
    _, s32 = base.autograd_reference(net, torch.float32, d2, idx)
    _, stats = upd.grad(*d2, idx)
    ef, e32 = abs(float(stats[4]) - float(s64[4])) / float(s64[4]), abs(float(s32[4] - s64[4])) / float(s64[4])
    print("max ratio %.9g fp64 %.9g e(fused) %.3e e(g32) %.3e" % (float(stats[4]), float(s64[4]), ef, e32))
    assert ef <= max(8 * e32, 1e-5) and float(stats[4]) >= 2.99


# --------------------------------------------------------------------------------------------------------- 3. stale scratch
@pytest.mark.parametrize("obs_dim,sizes", [(15, (4096, 17, 7)), (186, (1000, 33))])
def test_a_small_batch_after_a_large_one_reads_nothing_stale(obs_dim, sizes):
    """The scratch (tiles, split partials, tile statistics) still holds the large batch: the small batches' results equal, bit for
    bit, those of an updater that has only ever seen the small batch."""
    net, data, _ = base.case(obs_dim)
    used = new_updater(copy.deepcopy(net))
    used.grad(*data, torch.arange(sizes[0], device=DEV))
    for B in sizes[1:]:
        idx = (torch.arange(B, device=DEV) * 3 + 1).contiguous()
        g, s = used.grad(*data, idx)
        g, s = g.clone(), s.clone()
        g2, s2 = new_updater(copy.deepcopy(net)).grad(*data, idx)
        assert torch.equal(g, g2) and torch.equal(s, s2), B
        assert g.abs().max() > 0 and float(s[5]) == 0.0


# --------------------------------------------------------------------------------------------------- 4. degenerate minibatches
B_DEG = 200


def rows_at_ratios(net, ratio, adv, seed, scale=1.0, far=None):
    """B_DEG rows whose fp64 ratio is `ratio` (up to the rounding of LP to float32): actions sampled from the net, LP = the fp64
    log-probability - log(ratio), as make_data does for its near-boundary rows.  far: rows whose action is moved 20 sigma from the
    mean in both components and whose LP is 0.5, a plausible old log-probability."""
    torch.manual_seed(seed)
    with torch.no_grad():
        O = scale * torch.randn(B_DEG, 15, device=DEV)
        mu = net.pi(O)
        A = mu + net.log_std.exp() * torch.randn_like(mu)
        if far is not None:
            A[far] = mu[far] + 20.0 * net.log_std.exp()
        n64 = copy.deepcopy(net).double()
        LP = (n64.log_prob(n64.pi(O.double()), A.double()) - ratio.double().log()).float()
        if far is not None:
            LP[far] = 0.5
        RET = torch.randn(B_DEG, device=DEV)
    return O.contiguous(), A.contiguous(), LP.contiguous(), adv.clone().contiguous(), RET


def test_every_row_on_the_clipped_branch_gives_an_exactly_zero_policy_gradient():
    net, _, upd = base.case(15)
    half = B_DEG // 2
    ratio = torch.cat([torch.full((half,), 1.5), torch.full((half,), 0.5)]).to(DEV)
    adv = torch.cat([torch.ones(half), -torch.ones(half)]).to(DEV)
    data = rows_at_ratios(net, ratio, adv, seed=21)
    gf, stats, g64, _ = base.assert_parity(net, data, upd, None, "all clipped", names=V_TENSORS)
    for name, x, b in zip(base.NAMES[:8], gf, g64):
        assert bool((x == 0).all()) and bool((b == 0).all()), name
    want = float(torch.tensor(-ENT, dtype=torch.float32))
    assert gf[16].tolist() == [want, want], gf[16].tolist()
    assert float(stats[6]) == 1.0 and float(stats[5]) == 0.0


def test_no_row_clipped():
    net, _, upd = base.case(15)
    torch.manual_seed(22)
    ratio = (0.9 + 0.2 * torch.rand(B_DEG)).to(DEV)
    adv = torch.randn(B_DEG).to(DEV)
    adv[adv.abs() < 1e-3] = 1.0
    data = rows_at_ratios(net, ratio, adv, seed=23)
    _, stats, _, _ = base.assert_parity(net, data, upd, None, "none clipped")
    assert float(stats[6]) == 0.0 and float(stats[5]) == 0.0


def test_zero_advantages_and_ratios_that_underflow_to_zero():
    """A quarter of the rows with adv == 0 exactly (no branch of the minimum is active: no gradient), a quarter with actions 20 sigma
    from the mean: their ratio is exp(-400) = 0 in float32 and 1e-174 in float64, no gradient either, and nothing is non-finite."""
    net, _, upd = base.case(15)
    q = B_DEG // 4
    torch.manual_seed(24)
    ratio = torch.tensor([0.6, 0.95, 1.05, 1.4])[torch.randint(0, 4, (B_DEG,))].to(DEV)
    adv = torch.randn(B_DEG).to(DEV)
    adv[adv.abs() < 1e-3] = 1.0
    adv[:q] = 0.0
    far = torch.arange(q, 2 * q, device=DEV)
    data = rows_at_ratios(net, ratio, adv, seed=25, far=far)
    assert bool((data[3][:q] == 0.0).all())
    for dtype in (torch.float64, torch.float32):                      # on the CPU: what the reference itself sees
        n = copy.deepcopy(net).cpu().to(dtype)
        o, a, lp, ad, ret = (x.cpu().to(dtype) for x in data)
        loss, pg, vf, r = base.loss_terms(n, o, a, lp, ad, ret)
        loss.backward()
        assert all(bool(torch.isfinite(x).all()) for x in [loss, pg, vf, r] + [p.grad for p in base.ordered(n)]), dtype
        if dtype == torch.float64:
            assert bool(((r[q:2 * q] > 0.0) & (r[q:2 * q] < 1e-150)).all())
        else:
            assert bool((r[q:2 * q] == 0.0).all())
    gf, stats, _, _ = base.assert_parity(net, data, upd, None, "adv 0 / ratio 0")
    assert all(bool(torch.isfinite(x).all()) for x in gf) and bool(torch.isfinite(stats).all())
    assert float(stats[5]) == 0.0


def test_saturated_hidden_units():
    """Observations scaled by 50: most first-layer units sit at tanh = +-1, where 1 - y^2 is zero or a few ulp.  The rule's absolute
    floor of 1e-5 carries a layer whose fp64 gradient is ~0; both errors are printed for every tensor."""
    net, _, upd = base.case(15)
    torch.manual_seed(26)
    ratio = torch.tensor([0.6, 0.95, 1.05, 1.4])[torch.randint(0, 4, (B_DEG,))].to(DEV)
    adv = torch.randn(B_DEG).to(DEV)
    adv[adv.abs() < 1e-3] = 1.0
    data = rows_at_ratios(net, ratio, adv, seed=27, scale=50.0)
    gf, stats, _, _ = base.assert_parity(net, data, upd, None, "obs x 50")
    assert all(bool(torch.isfinite(x).all()) for x in gf) and bool(torch.isfinite(stats).all())
    assert float(stats[5]) == 0.0


# ------------------------------------------------------------------------------ 5. a per-column metric for the first layer
F_COLUMN = 8.0


def test_first_layer_gradient_is_right_in_every_input_column():
    """Observation column k scaled by 10 ** linspace(-3, 2, 186)[k], the first layers' weight columns by the inverse: the activations
    and clip fractions are make_data's, the columns of dW1 differ by five orders of magnitude, and a per-tensor maximum norm sees the
    largest only.  Per input column k of pi.W1 and v.W1: e_k(x) = max_n |x[n, k] - g64[n, k]| / max_n |g64[n, k]|, required
    e_k(fused) <= max(F_COLUMN e_k(g32), 1e-5)."""
    obs_dim, B = 186, 1000
    net = base.make_net(obs_dim, seed=5)
    O, A, LP, ADV, RET = base.make_data(net, obs_dim, seed=6, n_rows=B)
    scale = (10.0 ** torch.linspace(-3, 2, obs_dim, dtype=torch.float64)).to(DEV)
    with torch.no_grad():
        O = (O.double() * scale).float().contiguous()
        for seq in (net.pi, net.v):
            seq[0].weight.copy_((seq[0].weight.double() / scale).float())
        n64 = copy.deepcopy(net).double()
        r = (n64.log_prob(n64.pi(O.double()), A.double()) - LP.double()).exp()           # make_data's assertions, on what is used
        assert not (((r - (1 - CLIP)).abs() < 5e-5) | ((r - (1 + CLIP)).abs() < 5e-5)).any()
        assert (r < 1 - CLIP).float().mean() > 0.02 and (r > 1 + CLIP).float().mean() > 0.02
    data = (O, A, LP, ADV, RET)
    upd = new_updater(net, max_batch=B)
    gf, _, g64, g32 = base.assert_parity(net, data, upd, None, "scaled columns")
    failed = []
    for name, j in (("pi.W1", 0), ("v.W1", 8)):
        x, a, b = (t.reshape(256, obs_dim) for t in (gf[j], g32[j], g64[j]))
        den = b.abs().amax(0)
        assert float(den.min()) > 0
        ef, e32 = (x - b).abs().amax(0) / den, (a - b).abs().amax(0) / den
        ratio = ef / e32.clamp_min(1e-30)
        top = ratio.topk(5)
        print("%s worst e_k(fused) / e_k(g32): %s at columns %s; median %.2f; e_k(fused) max %.3e, e_k(g32) max %.3e"
              % (name, ["%.2f" % v for v in top.values.tolist()], top.indices.tolist(), float(ratio.median()), float(ef.max()), float(e32.max())))
        bad = ~(ef <= torch.maximum(F_COLUMN * e32, torch.full_like(e32, 1e-5)))
        failed += [(name, int(k), float(ef[k]), float(e32[k])) for k in bad.nonzero().reshape(-1)]
    assert not failed, failed


# ------------------------------------------------------------------------- 6. clip, Adam and repack at every width and option
# q_pi, q_v: with clipping on, the gradient of a group is (a random integer in [-8, 8]) * q; with it off, randn scaled to norm_pi, norm_v
OPTIONS = {
    "defaults": dict(kw=dict(lr=2e-4, max_norm_pi=0.5, max_norm_v=0.5), q_pi=2.0 ** -6, q_v=2.0 ** -12),
    "both_clipped": dict(kw=dict(lr=1e-3, betas=(0.8, 0.99), eps=1e-5, max_norm_pi=0.5, max_norm_v=0.5), q_pi=2.0 ** -6, q_v=2.0 ** -6),
    "clipping_off": dict(kw=dict(lr=2e-4, max_norm_pi=0.0, max_norm_v=0.0), norm_pi=5.0, norm_v=0.1),
}


def total_norm(params):
    """clip_grad_norm's norm (examples/ppo.py) without the clip."""
    sq = None
    for p in params:
        s = (p.grad * p.grad).sum()
        sq = s if sq is None else sq + s
    return torch.sqrt(sq)


@pytest.mark.parametrize("option", sorted(OPTIONS))
@pytest.mark.parametrize("obs_dim", [1, 15, 32, 33, 186])
def test_clip_adam_and_repack_at_every_width_and_option(obs_dim, option):
    """test_clip_and_adam_match_torch_and_repack_the_policy_buffer with its rules, for 25 steps with a fresh random gradient each, at
    widths 1, 15, 32 (no padding), 33 (one column into a second 32-k step) and 186.  Before every step the updater's theta, m and v
    are copied into the twin and its optimiser's state (step t - 1), so that every step is a one-step comparison at t = 1 .. 25 and
    the per-step bounds apply.  Options: the defaults (policy group clipped, value group not); both groups clipped with other betas,
    eps and lr; max_norm 0, which turns clipping off: the norms are still reported, the step is Adam's on the unscaled gradient.

    The twin sums the squares for its norm in float32, in torch's order; the updater in float64, in its own.  On arbitrary values the
    two norms agree to rtol 1e-6 and not to the bit, then the clip coefficients differ in their last bit, so does every scaled
    gradient element, and every rounding after it falls independently on the two sides: an element that the step carries across zero
    then differs by the accumulated rounding of the step itself, measured 2.1 to 3.9 ulp on the MI355X among 10^5 elements and 25
    steps (and m misses its RELATIVE bound wherever (1 - w) m and w g cancel).  That is the reference's summation error, not the
    updater's, so with clipping on the gradient lies on a grid: a random integer in [-8, 8] times a power of two per group.  Every
    square and every partial sum of at most 2^17 of them is then exact in float32 in any order (an integer below 2^24 times q^2),
    both norms and both coefficients are the same bits (max_norm 0.5 is a power of two: torch's reciprocal-then-multiply rounds once,
    as the updater's division), and the bounds apply as they stand.  Norms of arbitrary values at every width: with clipping off."""
    import ppo
    from gym_auv_amd import _capi
    from gym_auv_amd.ppo_update import FusedPPOUpdate
    opt_set = OPTIONS[option]
    kw = opt_set["kw"]
    net = base.make_net(obs_dim, seed=3)
    twin = copy.deepcopy(net)
    upd = FusedPPOUpdate(net, max_batch=64, **kw)
    buf = torch.zeros(int(_capi.load_library().auv_policy_param_floats(obs_dim)), device=DEV)
    upd.attach(types.SimpleNamespace(bf16=False, env=types.SimpleNamespace(obs_dim=obs_dim), params=buf))
    assert torch.equal(buf, base.expected_policy_buffer(net, obs_dim))
    n_pi = sum(p.numel() for p in net.pi.parameters())
    n_v = sum(p.numel() for p in net.v.parameters())
    assert n_pi + n_v + 2 == upd.theta.numel()
    tp = base.ordered(twin)
    adam_kw = {k: kw[k] for k in ("lr", "betas", "eps") if k in kw}
    opt = torch.optim.Adam(tp, **adam_kw)
    pi_t, v_t = list(twin.pi.parameters()) + [twin.log_std], list(twin.v.parameters())
    mx = kw["max_norm_pi"]
    torch.manual_seed(11 + obs_dim)
    worst, exact = 0.0, 0
    for t in range(1, 26):
        if mx > 0:
            g = torch.randint(-8, 9, (upd.theta.numel(),), device=DEV).float() * opt_set["q_pi"]
            g[n_pi:n_pi + n_v] *= opt_set["q_v"] / opt_set["q_pi"]
        else:
            g = torch.randn(upd.theta.numel(), device=DEV)
            g[:n_pi] *= opt_set["norm_pi"] / g[:n_pi].norm()          # (with log_std: a little above)
            g[n_pi:n_pi + n_v] *= opt_set["norm_v"] / g[n_pi:n_pi + n_v].norm()
        off = 0
        with torch.no_grad():
            for p in tp:
                sl = slice(off, off + p.numel())
                off += p.numel()
                p.copy_(upd.theta[sl].view_as(p))
                p.grad = g[sl].view_as(p).clone()
                opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": upd.m[sl].view_as(p).clone(),
                                "exp_avg_sq": upd.v[sl].view_as(p).clone()}
        if mx > 0:
            norms_t = torch.stack([ppo.clip_grad_norm(pi_t, mx), ppo.clip_grad_norm(v_t, kw["max_norm_v"])])
        else:
            norms_t = torch.stack([total_norm(pi_t), total_norm(v_t)])
        before = [p.detach().clone() for p in tp]
        opt.step()
        norms = upd.apply(g).clone()
        assert upd.t == t and float(opt.state[tp[0]]["step"]) == t
        if option == "both_clipped":
            assert norms_t[0] > 0.5 and norms_t[1] > 0.5
        else:
            assert norms_t[0] > 0.5 > norms_t[1]
        assert torch.allclose(norms, norms_t, rtol=1e-6, atol=0), (norms, norms_t)
        exact += int(torch.equal(norms, norms_t))
        worst = max(worst, base.assert_adam_step(upd, net, tp, opt, before, t, say=False))
        assert torch.equal(buf, base.expected_policy_buffer(net, obs_dim)), t
    print("obs_dim %3d %-12s 25 steps: largest difference of a parameter %.2f ulp; both norms the twin's bits in %d steps" % (obs_dim, option, worst, exact))
    assert mx == 0 or exact == 25                                     # (the grid does what the docstring says)
    if obs_dim in (33, 186):
        # the forward and the transposed copies follow: a gradient after the steps is the gradient AT the updated weights
        data = base.make_data(net, obs_dim, seed=2)
        base.assert_parity(net, data, upd, torch.arange(64, device=DEV), "obs_dim %3d after 25 steps" % obs_dim)


# ------------------------------------------------------------------------------------------------ 7. the wrapper's other paths
def attached(obs_dim, seed=4, **kw):
    from gym_auv_amd import _capi
    net = base.make_net(obs_dim, seed=seed)
    upd = new_updater(net, max_batch=64, **kw)
    buf = torch.zeros(int(_capi.load_library().auv_policy_param_floats(obs_dim)), device=DEV)
    fused = types.SimpleNamespace(bf16=False, env=types.SimpleNamespace(obs_dim=obs_dim), params=buf)
    upd.attach(fused)
    return net, upd, fused


def test_a_detached_policy_buffer_is_left_alone_and_is_current_after_attaching_again():
    obs_dim = 33
    net, upd, fused = attached(obs_dim)
    buf = fused.params
    assert torch.equal(buf, base.expected_policy_buffer(net, obs_dim))
    upd.attach(None)
    kept, theta0 = buf.clone(), upd.theta.clone()
    torch.manual_seed(12)
    g = torch.randn(upd.theta.numel(), device=DEV)
    upd.apply(g)
    assert float((upd.theta != theta0).float().mean()) > 0.99         # (Adam's first step moves every weight by about lr)
    assert torch.equal(buf, kept)
    assert not torch.equal(buf, base.expected_policy_buffer(net, obs_dim))
    upd.attach(fused)
    assert torch.equal(buf, base.expected_policy_buffer(net, obs_dim))


def test_load_after_an_outside_write_repacks_every_copy():
    obs_dim = 33
    net, upd, fused = attached(obs_dim)
    before = fused.params.clone()
    with torch.no_grad():
        upd.theta.mul_(1.01)
    assert torch.equal(fused.params, before)                          # (nothing has told the updater yet)
    upd.load()
    assert torch.equal(fused.params, base.expected_policy_buffer(net, obs_dim)) and not torch.equal(fused.params, before)
    data = base.make_data(net, obs_dim, seed=2)
    base.assert_parity(net, data, upd, torch.arange(64, device=DEV), "after load")


def test_step_is_grad_then_apply():
    net, data, _ = base.case(15)
    a, b = new_updater(copy.deepcopy(net), max_batch=256), new_updater(copy.deepcopy(net), max_batch=256)
    for k in range(3):
        idx = (torch.arange(200, device=DEV) * 7 + k).contiguous()
        row_a = a.step(*data, idx).clone()
        g, s = b.grad(*data, idx)
        s = s.clone()
        norms = b.apply().clone()
        row_b = b.log[k]
        assert torch.equal(row_b[:8], s) and torch.equal(row_b[8:], norms) and float(norms[0]) > 0 and float(norms[1]) > 0
        assert torch.equal(row_a, row_b) and torch.equal(a.log[k], row_b)
        assert torch.equal(a.theta, b.theta) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
        assert a.n_steps == b.n_steps == k + 1 and a.t == b.t == k + 1
    assert not torch.equal(a.theta, torch.cat([p.detach().reshape(-1) for p in base.ordered(net)]))
    assert float(a.log[3].abs().max()) == 0.0


def test_the_log_is_a_ring():
    net, data, _ = base.case(15)
    upd = new_updater(copy.deepcopy(net), max_batch=256)
    last = upd.LOG_ROWS - 1
    upd.n_steps = last
    idx = torch.arange(100, device=DEV)
    r0 = upd.step(*data, idx).clone()
    r1 = upd.step(*data, idx).clone()
    assert upd.n_steps == last + 2 and upd.t == 2
    assert torch.equal(upd.log[last], r0) and torch.equal(upd.log[0], r1)
    assert float(r0[8]) > 0 and float(r1[8]) > 0 and not torch.equal(r0, r1)
    assert float(upd.log[1:last].abs().max()) == 0.0
    assert math.isfinite(float(r1[0]))
