"""-m gpu: the fused PPO / clone update at the hidden widths of POL_ARCH_LIST other than the reference's (gym_auv_amd/ppo_update.py,
csrc/auv_ppo_pass.h, k13_ppo_update_arch.hip) against autograd on the torch modules of examples/ppo.py.  No environment handle except in
the last test: random tensors, 5000 stored rows.

Gradient parity by the rule of tests/test_gpu_ppo_update.py: per parameter tensor e(x) = max |x - g64| / max |g64| with
g64 = autograd in fp64, g32 the same in fp32; required e(fused) <= max(8 e(g32), 1e-5), and the same bound per statistic.  Every figure
is printed before it is asserted."""
import copy
import functools
import math
import os
import sys
import types

import pytest
import torch

import test_gpu_clone_update as tc
import test_gpu_ppo_update as tp
from test_gpu_ppo_update import CLIP, DEV, ENT, N_ROWS, VF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

REF = (256, 128, 64)
NEW = [(128, 128, 64), (128, 64, 64), (64, 64, 64)]
# make_data's perturbation of the policy that "collected" the rows: tests/test_gpu_ppo_update.py uses 0.15 for the reference's net.  A
# triple listed here would take another scale so that the ratios still spread over both clip boundaries (make_data's own conditions,
# asserted for every net in test_rows_meet_make_data_s_conditions).  None needs it: at 0.15 every new net has 5 - 18 % of its rows below
# 1 - clip and 11 - 30 % above 1 + clip.
PERTURB = {}


def make_net(obs_dim, hidden, seed=0, device=DEV):
    """tests/test_gpu_ppo_update.make_net with the hidden widths `hidden`."""
    import ppo
    torch.manual_seed(seed)
    net = ppo.ActorCritic(obs_dim, hidden=hidden).to(device)
    with torch.no_grad():
        net.log_std.copy_(torch.tensor([-0.5, -1.1]))
        for m in list(net.pi) + list(net.v):
            if isinstance(m, torch.nn.Linear):
                m.bias.uniform_(-0.3, 0.3)
    return net


def make_data(net, obs_dim, hidden, seed=1, device=DEV, n_rows=N_ROWS):
    """tests/test_gpu_ppo_update.make_data, line by line, with the perturbation scale of PERTURB: actions sampled from the net, LP from a
    perturbed copy, rows within 1e-4 of a clip boundary (in fp64) or with |adv| < 1e-6 replaced by rows at ratio 1.  Its conditions are
    asserted: no row within 1e-4 of a boundary, at least 2 % of the rows beyond each."""
    scale = PERTURB.get(tuple(hidden), 0.15)
    torch.manual_seed(seed)
    with torch.no_grad():
        O = torch.randn(n_rows, obs_dim, device=device)
        mu = net.pi(O)
        A = mu + net.log_std.exp() * torch.randn_like(mu)
        old = copy.deepcopy(net)
        for p in old.pi.parameters():
            p.add_(scale * torch.randn_like(p) * p.abs().max())
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
        lo, hi = float((r < 1 - CLIP).float().mean()), float((r > 1 + CLIP).float().mean())
        print("hidden %s obs_dim %d on %s: %.1f %% of the rows below 1 - clip, %.1f %% above 1 + clip, %d replaced"
              % (list(hidden), obs_dim, device, 100 * lo, 100 * hi, int(near.sum())))
        assert not (((r - (1 - CLIP)).abs() < 1e-4) | ((r - (1 + CLIP)).abs() < 1e-4) | (ADV.abs() < 1e-6)).any()
        assert lo > 0.02 and hi > 0.02, (lo, hi)
    return O, A, LP, ADV, RET


@functools.lru_cache(maxsize=None)
def case(hidden, obs_dim):
    """Shared by every test of one net: the module, the PPO rows, the clone rows, the updater (max_batch 4096).  Nothing here is modified
    afterwards."""
    from gym_auv_amd.ppo_update import FusedPPOUpdate
    net = make_net(obs_dim, hidden)
    data = make_data(net, obs_dim, hidden)
    upd = FusedPPOUpdate(net, clip=CLIP, vf_coef=VF, ent_coef=ENT, max_batch=4096)
    assert upd.hidden == tuple(hidden) and upd._arch is not None
    return net, data, tc.make_data(obs_dim), upd


@pytest.mark.parametrize("hidden,obs_dim", [(h, D) for h in NEW for D in (6, 15, 186)] + [((64, 64, 64), 600)])
def test_rows_meet_make_data_s_conditions(hidden, obs_dim):
    """On the CPU (no launch): make_data's own assertions for every net the tests below draw rows from."""
    make_data(make_net(obs_dim, hidden, device="cpu"), obs_dim, hidden, device="cpu")


@pytest.mark.parametrize("B", [1, 17, 33, 1000, 4096])
@pytest.mark.parametrize("obs_dim", [6, 186])
@pytest.mark.parametrize("hidden", NEW)
def test_gradient_and_stats_match_autograd(hidden, obs_dim, B):
    """obs_dim 6 / 186: K0p = 32 with one layer-0 k-group, 192 with three.  B = 1: one ragged tile; 17, 33: a one-row tile after one and
    two full ones; 1000: at [64, 64, 64] the split factor lies above the reference width's; 4096: the cap."""
    net, data, _, upd = case(hidden, obs_dim)
    torch.manual_seed(100 + B)
    perm = torch.randperm(N_ROWS, device=DEV)
    idx = perm[:B].contiguous()
    if B == 1:
        # (one row on the clipped branch has a policy gradient of exactly zero: nothing to compare.  The first row of the permutation
        # that is not clipped -- by the fp64 ratio, which make_data keeps 1e-4 away from the boundaries)
        O, A, LP, ADV, _ = data
        with torch.no_grad():
            n64 = copy.deepcopy(net).double()
            r = (n64.log_prob(n64.pi(O.double()), A.double()) - LP.double()).exp()[perm]
        clipped = ((ADV[perm] > 0) & (r > 1 + CLIP)) | ((ADV[perm] < 0) & (r < 1 - CLIP))
        idx = perm[(~clipped).nonzero()[:1, 0]].contiguous()
    _, stats, _, _ = tp.assert_parity(net, data, upd, idx, "%s obs_dim %3d B %4d" % (list(hidden), obs_dim, B))
    assert idx.numel() == B and float(stats[5]) == 0.0 and float(stats[7]) == 0.0         # no non-finite input; the spare slot
    if B >= 1000:
        assert 0.0 < float(stats[6]) < 1.0


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", ["nll", "mse"])
@pytest.mark.parametrize("B", [1, 17, 4095])
@pytest.mark.parametrize("obs_dim", [6, 186])
@pytest.mark.parametrize("hidden", NEW)
def test_clone_gradient_and_stats_match_autograd(hidden, obs_dim, B, kind, weighted):
    net, _, cdata, upd = case(hidden, obs_dim)
    torch.manual_seed(100 + B)
    idx = torch.randperm(N_ROWS, device=DEV)[:B].contiguous()
    if weighted and B == 1:
        idx = (cdata[3] > 0).nonzero()[:1, 0].contiguous()            # (one row of weight zero has no gradient to compare)
    _, stats = tc.assert_parity(net, cdata, upd, idx, kind, weighted, "%s obs_dim %3d B %4d %s w %d" % (list(hidden), obs_dim, B, kind, weighted))
    if not weighted:
        assert float(stats[4]) == float(B)


@pytest.mark.parametrize("hidden", NEW)
def test_gather_is_bit_identical_to_contiguous_rows(hidden):
    net, data, cdata, upd = case(hidden, 186)
    torch.manual_seed(5)
    idx = torch.randperm(N_ROWS, device=DEV)[:1000].contiguous()
    g, s = upd.grad(*data, idx)
    g, s = g.clone(), s.clone()
    g2, s2 = upd.grad(*(x[idx].contiguous() for x in data), None)
    assert torch.equal(g, g2) and torch.equal(s, s2)
    assert float(s[6]) > 0.0 and g.abs().max() > 0
    g, s = upd.clone_grad(*cdata, idx)
    g, s = g.clone(), s.clone()
    g2, s2 = upd.clone_grad(*(x[idx].contiguous() for x in cdata))
    assert torch.equal(g, g2) and torch.equal(s, s2)
    assert g.abs().max() > 0 and float(s[4]) > 0


@pytest.mark.parametrize("obs_dim,B", [(186, 4096), (6, 7)])
@pytest.mark.parametrize("hidden", NEW)
def test_two_calls_give_the_same_bits(hidden, obs_dim, B):
    net, data, cdata, upd = case(hidden, obs_dim)
    idx = torch.arange(B, device=DEV) * (N_ROWS // B)
    for fn in (lambda: upd.grad(*data, idx), lambda: upd.clone_grad(*cdata, idx, kind="nll")):
        g, s = fn()
        g, s = g.clone(), s.clone()
        g2, s2 = fn()
        assert torch.equal(g, g2) and torch.equal(s, s2)
        assert g.abs().max() > 0


def policy_namespace(obs_dim, hidden, params):
    """What FusedPPOUpdate.attach reads of a FusedActorCritic."""
    return types.SimpleNamespace(bf16=False, env=types.SimpleNamespace(obs_dim=obs_dim), params=params, hidden=tuple(hidden))


@pytest.mark.parametrize("hidden", NEW)
def test_clip_and_adam_match_torch_and_repack_the_policy_buffer(hidden):
    """tests/test_gpu_ppo_update.py's test of the same name at the other widths: three steps on a fixed random gradient (policy group
    clipped, value group not) against examples/ppo.clip_grad_norm + torch.optim.Adam on a twin, by assert_adam_step's rules (norms rtol
    1e-6, m and v rtol 2e-6, every parameter within 2 ulp).  The attached buffer is BITWISE pack_policy_params of the module, after load
    and after every step; a gradient after the steps is the gradient AT the updated weights (the forward and the transposed copy
    followed); a policy of another triple is refused."""
    import ppo
    from gym_auv_amd.policy import pack_policy_params, policy_param_floats
    from gym_auv_amd.ppo_update import FusedPPOUpdate
    obs_dim = 15
    net = make_net(obs_dim, hidden, seed=3)
    twin = copy.deepcopy(net)
    upd = FusedPPOUpdate(net, lr=2e-4, max_norm_pi=0.5, max_norm_v=0.5, max_batch=64)
    buf = torch.zeros(policy_param_floats(obs_dim, hidden), device=DEV)
    other = REF if hidden != REF else NEW[0]
    with pytest.raises(ValueError, match="hidden widths"):
        upd.attach(policy_namespace(obs_dim, other, torch.zeros(policy_param_floats(obs_dim, other), device=DEV)))
    upd.attach(policy_namespace(obs_dim, hidden, buf))
    assert torch.equal(buf, pack_policy_params(net, obs_dim, hidden=hidden))
    n_pi = sum(p.numel() for p in net.pi.parameters())
    n_v = sum(p.numel() for p in net.v.parameters())
    torch.manual_seed(11)
    g = torch.randn(upd.theta.numel(), device=DEV)
    g[:n_pi] *= 5.0 / g[:n_pi].norm()                               # (with log_std: a little above 5 -> clipped at 0.5)
    g[n_pi:n_pi + n_v] *= 0.1 / g[n_pi:n_pi + n_v].norm()           # 0.1 < 0.5: not clipped
    tw = tp.ordered(twin)
    opt = torch.optim.Adam(tw, lr=2e-4)
    pi_t, v_t = list(twin.pi.parameters()) + [twin.log_std], list(twin.v.parameters())
    for step in range(3):
        off = 0
        for p in tw:
            p.grad = g[off:off + p.numel()].view_as(p).clone()
            off += p.numel()
        norms_t = torch.stack([ppo.clip_grad_norm(pi_t, 0.5), ppo.clip_grad_norm(v_t, 0.5)])
        before = [p.detach().clone() for p in tw]
        opt.step()
        norms = upd.apply(g).clone()
        assert norms_t[0] > 0.5 > norms_t[1]
        print("step %d norms %s torch %s" % (step, norms.tolist(), norms_t.tolist()))
        assert torch.allclose(norms, norms_t, rtol=1e-6, atol=0), (norms, norms_t)
        tp.assert_adam_step(upd, net, tw, opt, before, step)
        assert torch.equal(buf, pack_policy_params(net, obs_dim, hidden=hidden)), step
    data = make_data(net, obs_dim, hidden, seed=2)
    tp.assert_parity(net, data, upd, torch.arange(64, device=DEV), "%s after three steps" % list(hidden))


def test_two_handles_of_different_widths_alternate():
    """One updater of [64, 64, 64] and one of [256, 128, 64], both live, used alternately twice each: every gradient is bitwise what the
    same updater gave alone (nothing of a launch belongs to the kernel or the process instead of the handle)."""
    from gym_auv_amd.ppo_update import FusedPPOUpdate
    obs_dim = 15
    torch.manual_seed(7)
    idx = torch.randperm(N_ROWS, device=DEV)[:1000].contiguous()
    made, alone = [], []
    for hidden in ((64, 64, 64), REF):
        net = make_net(obs_dim, hidden)
        data = make_data(net, obs_dim, hidden)
        upd = FusedPPOUpdate(net, clip=CLIP, vf_coef=VF, ent_coef=ENT, max_batch=1000)
        g, s = upd.grad(*data, idx)
        made.append((data, upd))
        alone.append((g.clone(), s.clone()))
        assert g.abs().max() > 0
    assert made[0][1].hidden == (64, 64, 64) and made[1][1].hidden == REF and made[0][1].theta.numel() < made[1][1].theta.numel()
    for _ in range(2):
        for (data, upd), (g0, s0) in zip(made, alone):
            g, s = upd.grad(*data, idx)
            assert torch.equal(g, g0) and torch.equal(s, s0), upd.hidden


def test_wide_observations_use_more_than_64_kib_of_lds():
    """[64, 64, 64] at obs_dim 600: the row pass' LDS tile (csrc/auv_ppo_pass.h, ppo_lds_floats_h) is 16 rows of X (608 + 8), Y1, 2 x Y2,
    2 x Y3 (72 each) and D4 (72) floats + 144 bytes = 67216 bytes, above the 64 KiB a kernel gets without asking (at obs_dim 400: 54928),
    so the launch must have asked for it on ITS instantiation."""
    from gym_auv_amd.ppo_update import FusedPPOUpdate
    hidden, D = (64, 64, 64), 600
    assert 16 * ((608 + 8) + 72 + 2 * 72 + 2 * 72 + 72) * 4 + 144 == 67216 > 64 * 1024 > 16 * ((416 + 8) + 6 * 72) * 4 + 144
    net = make_net(D, hidden)
    data = make_data(net, D, hidden)
    upd = FusedPPOUpdate(net, clip=CLIP, vf_coef=VF, ent_coef=ENT, max_batch=100)
    tp.assert_parity(net, data, upd, torch.arange(100, device=DEV) * 7, "%s obs_dim %d B 100" % (list(hidden), D))


def test_default_width_through_the_arch_entry_is_bitwise_the_plain_entry():
    """FusedPPOUpdate(net, arch_entry=True) at [256, 128, 64] dispatches to the very kernels of the plain constructor: the flat gradient,
    the statistics, the clone gradient, and theta, m, v after three steps are equal bit for bit."""
    from gym_auv_amd.ppo_update import FusedPPOUpdate
    obs_dim = 186
    net = tp.make_net(obs_dim)
    net2 = copy.deepcopy(net)
    data = tp.make_data(net, obs_dim)
    cdata = tc.make_data(obs_dim)
    plain = FusedPPOUpdate(net, clip=CLIP, vf_coef=VF, ent_coef=ENT, max_batch=4096)
    arch = FusedPPOUpdate(net2, clip=CLIP, vf_coef=VF, ent_coef=ENT, max_batch=4096, arch_entry=True)
    assert plain._arch is None and arch._arch is not None and plain.hidden == arch.hidden == REF
    torch.manual_seed(3)
    idx = torch.randperm(N_ROWS, device=DEV)[:4096].contiguous()
    g1, s1 = plain.grad(*data, idx)
    g2, s2 = arch.grad(*data, idx)
    assert torch.equal(g1, g2) and torch.equal(s1, s2) and g1.abs().max() > 0
    g1, s1 = plain.clone_grad(*cdata, idx)
    g2, s2 = arch.clone_grad(*cdata, idx)
    assert torch.equal(g1, g2) and torch.equal(s1, s2) and g1.abs().max() > 0
    before = plain.theta.clone()
    for k in range(3):
        r1 = plain.step(*data, idx[1000 * k:1000 * (k + 1)].contiguous()).clone()
        r2 = arch.step(*data, idx[1000 * k:1000 * (k + 1)].contiguous()).clone()
        assert torch.equal(r1, r2), k
    assert not torch.equal(before, plain.theta)
    assert torch.equal(plain.theta, arch.theta) and torch.equal(plain.m, arch.m) and torch.equal(plain.v, arch.v)


def test_training_a_narrow_net_with_the_fused_update(monkeypatch):
    """tests/test_gpu_ppo_update.py's training test at [64, 64, 64]: every update moves the weights, nothing is non-finite, and the
    rollout policy's packed buffer is bitwise the packing of the trained net."""
    import ppo
    from gym_auv_amd.policy import pack_policy_params
    from gym_auv_amd.ppo_update import FusedPPOUpdate
    hidden = (64, 64, 64)
    keep = {}
    attach = FusedPPOUpdate.attach

    def recording_attach(self, fused=None):                          # (train() returns its history only: catch the objects it builds)
        keep.update(net=self.net, fused=fused, updater=self)
        return attach(self, fused)
    monkeypatch.setattr(FusedPPOUpdate, "attach", recording_attach)
    hist = ppo.train(task="pathfollow", envs=256, updates=2, rollout=16, minibatches=4, fused_update=True, net_arch=hidden, log=lambda *_: None)
    assert len(hist) == 2
    w = [h["weight_l1"] for h in hist]
    assert all(abs(b - a) > 1e-3 for a, b in zip(w[:-1], w[1:])), w   # every update moves the weights
    assert all(h["minibatch_steps_nonfinite"] == 0 and h["minibatch_steps"] == 16 for h in hist)
    assert all(math.isfinite(h["loss"]) and h["grad_norm_pi"] > 0 and h["grad_norm_v"] > 0 and h["max_ratio"] > 0 for h in hist)
    net, fused, upd = keep["net"], keep["fused"], keep["updater"]
    assert upd.hidden == fused.hidden == hidden and upd.n_steps == 32
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
    assert torch.equal(fused.params, pack_policy_params(net, fused.env.obs_dim, hidden=hidden))
