"""CPU: the tanh-squashed policy without a device -- the torch statement of its loss (ppo_update.squash_loss_terms) against an independent
one and against the plain PPO loss, the analytic extra gradients the kernel adds, the NumPy mirror of the action map
(policy.squash_map_reference), the refusals, the recorded bounds of the GPU tests (tests/golden/squash_bounds.json, derived in
tests/squash_cases.py) and the resource numbers of the new kernels."""
import math
import os
import types

import numpy as np
import pytest
import torch

import squash_cases as cases
from kernel_resources import HIPCC, assert_policy_budget, kernel_resources

f32, f64 = np.float32, np.float64
C_LOG = 0.5 * math.log(2.0 * math.pi)


def _batch(B, hidden=(64, 64, 64), obs_dim=7):
    net = cases.make_net(obs_dim, hidden)
    O, A, LP, ADV, RET = (x[:B].double() for x in cases.make_rows(obs_dim, hidden))
    return net, O, A, LP, ADV, RET


def _plain_loss(net, o, a, lp, adv, ret, clip, vf_coef, ent_coef):
    """minibatch_step of examples/ppo.py."""
    mu = net.pi(o)
    ratio = (net.log_prob(mu, a) - lp).exp()
    pg = -torch.min(ratio * adv, ratio.clamp(1 - clip, 1 + clip) * adv).mean()
    vf = 0.5 * (net.v(o).squeeze(-1) - ret).pow(2).mean()
    return pg + vf_coef * vf - ent_coef * net.entropy()


# ------------------------------------------------------------------------------ the torch statement
@pytest.mark.parametrize("ent_coef", [0.0, 0.01, 1.0])
def test_loss_terms_against_an_independent_autograd_statement(ent_coef):
    from gym_auv_amd.ppo_update import squash_loss_terms
    net, o, a, lp, adv, ret = _batch(37)
    loss, pg, vf, ent = squash_loss_terms(net, o, a, lp, adv, ret, cases.CLIP, cases.VF_COEF, ent_coef)
    g = cases.flat_grad(net, loss)
    # independently: torch.distributions' Gaussian, tanh and log1p spelled out, the noise recovered and held
    mu, sigma = net.pi(o), net.log_std.exp()
    dist = torch.distributions.Normal(mu, sigma)
    ratio = (dist.log_prob(a).sum(-1) - lp).exp()
    pg2 = -torch.minimum(ratio * adv, torch.clamp(ratio, 1 - cases.CLIP, 1 + cases.CLIP) * adv).mean()
    vf2 = 0.5 * torch.mean((net.v(o)[:, 0] - ret) ** 2)
    eps = ((a - mu) / sigma).detach()
    u = mu + sigma * eps
    ent2 = (dist.entropy() + torch.log1p(-torch.tanh(u) ** 2)).sum(-1).mean()
    loss2 = pg2 + cases.VF_COEF * vf2 - ent_coef * ent2
    g2 = cases.flat_grad(net, loss2)
    assert float(u.detach().abs().max()) < 12.0                     # (where log1p(-tanh^2) still holds digits in fp64)
    for x, y in ((loss, loss2), (pg, pg2), (vf, vf2), (ent, ent2)):
        assert abs(float(x.detach()) - float(y.detach())) <= 1e-10 * max(1.0, abs(float(y.detach())))
    assert float((g - g2).abs().max()) <= 1e-10 * max(1.0, float(g2.abs().max()))
    g0 = cases.flat_grad(net, squash_loss_terms(net, o, a, lp, adv, ret, cases.CLIP, cases.VF_COEF, 0.0)[0])
    assert ent_coef == 0.0 or float((g - g0).abs().max()) > 1e-6           # (the entropy term does move the gradient)


def test_without_the_entropy_term_it_is_the_plain_ppo_loss():
    from gym_auv_amd.ppo_update import squash_loss_terms
    net, o, a, lp, adv, ret = _batch(37)
    loss, pg, vf, ent = squash_loss_terms(net, o, a, lp, adv, ret, cases.CLIP, cases.VF_COEF, 0.0)
    plain = _plain_loss(net, o, a, lp, adv, ret, cases.CLIP, cases.VF_COEF, 0.0)
    assert abs(float(loss) - float(plain)) <= 1e-13 * max(1.0, abs(float(plain)))
    g, gp = cases.flat_grad(net, loss), cases.flat_grad(net, plain)
    assert float((g - gp).abs().max()) <= 1e-13 * max(1.0, float(gp.abs().max()))
    # the entropy is the Gaussian's plus the mean log-Jacobian of tanh at the stored actions
    want = float(net.entropy()) + float(torch.log1p(-torch.tanh(a) ** 2).sum(-1).mean())
    assert abs(float(ent) - want) <= 1e-10 * max(1.0, abs(want))


@pytest.mark.parametrize("ent_coef", [0.01, 1.0])
def test_the_extra_gradients_the_kernel_adds_are_autograds(ent_coef):
    """d/d mu_ik += ent_coef 2 tanh(a_ik) / B;  d/d log_std_k = -ent_coef (1 - (1/B) sum_i 2 tanh(a_ik) (a_ik - mu_ik)), for B = 5."""
    B = 5
    net, o, a, lp, adv, ret = _batch(B)
    mu = net.pi(o).detach().requires_grad_(True)
    log_std = net.log_std.detach().clone().requires_grad_(True)
    sigma = log_std.exp()
    u = mu + sigma * ((a - mu) / sigma).detach()
    assert torch.allclose(u, a, rtol=0, atol=1e-14)
    au = u.abs()
    ent = (0.5 + C_LOG + log_std + 2.0 * (math.log(2.0) - au - torch.log1p(torch.exp(-2.0 * au)))).sum(-1).mean()
    g_mu, g_ls = torch.autograd.grad(-ent_coef * ent, (mu, log_std))
    want_mu = ent_coef * 2.0 * torch.tanh(a) / B
    want_ls = -ent_coef * (1.0 - (2.0 * torch.tanh(a) * (a - mu.detach())).sum(0) / B)
    assert float((g_mu - want_mu).abs().max()) <= 1e-12 and float((g_ls - want_ls).abs().max()) <= 1e-12
    assert float(want_mu.abs().min()) > 0.0


# ------------------------------------------------------------------------------ the NumPy mirror
def test_the_map_mirror_is_odd_monotone_bounded_and_saturates_exactly():
    from gym_auv_amd.policy import squash_map_reference
    u = np.array(cases.SPECIAL_U)
    assert list(u) == [0.0, 1e-8, 0.5, 9.0, 20.0, 88.0, 1e30]
    mid, half = np.array(cases.MAP_MID), np.array(cases.MAP_HALF)
    for dtype in (f32, f64):
        uu = np.stack([u, u], axis=1).astype(dtype)
        pos, neg = squash_map_reference(uu, mid, half, dtype), squash_map_reference(-uu, mid, half, dtype)
        assert pos.dtype == dtype and np.isfinite(pos).all() and np.isfinite(neg).all()
        m, h = mid.astype(f32).astype(dtype), half.astype(f32).astype(dtype)
        # odd: bit for bit with mid = 0, and about mid up to the roundings of mid + x otherwise
        p0, n0 = squash_map_reference(uu, 0 * mid, half, dtype), squash_map_reference(-uu, 0 * mid, half, dtype)
        assert np.array_equal(p0, -n0)
        assert np.abs((pos - m) + (neg - m)).max() <= 2 * np.spacing(dtype(1.0))
        # monotone over -1e30 .. 1e30, inside the box
        chain = np.concatenate([neg[::-1], pos])
        assert (np.diff(chain, axis=0) >= 0).all()
        assert (np.abs(chain - m) <= np.abs(h)).all()
        assert (np.diff(chain, axis=0) > 0).any(axis=0).all()
    # float32: exactly mid +- half from |u| = 20 on
    uu = np.stack([u, u], axis=1).astype(f32)
    pos, neg = squash_map_reference(uu, mid, half, f32), squash_map_reference(-uu, mid, half, f32)
    far = u >= 20.0
    assert far.sum() == 3
    assert np.array_equal(pos[far], np.broadcast_to(mid.astype(f32) + half.astype(f32), (3, 2)))
    assert np.array_equal(neg[far], np.broadcast_to(mid.astype(f32) - half.astype(f32), (3, 2)))
    assert np.array_equal(pos[0], mid.astype(f32)) and not np.array_equal(pos[2], pos[4])
    # and it is tanh
    grid = cases.map_inputs().astype(f64)
    assert np.abs(squash_map_reference(grid, (0, 0), (1, 1), f64) - np.tanh(grid)).max() <= 4e-16


# ------------------------------------------------------------------------------ refusals
def _mlp(i, out, hidden=(256, 128, 64)):
    import torch.nn as nn
    h1, h2, h3 = hidden
    return nn.Sequential(nn.Linear(i, h1), nn.Tanh(), nn.Linear(h1, h2), nn.Tanh(), nn.Linear(h2, h3), nn.Tanh(), nn.Linear(h3, out))


def test_squash_refuses_the_launches_that_have_no_squashed_variant():
    """Before the environment or the library is touched: a stand-in with nothing but obs_dim and a device is enough."""
    import torch.nn as nn
    from gym_auv_amd.normalize import RunningNorm
    from gym_auv_amd.policy import FusedActorCritic
    from gym_auv_amd.population import PolicyPopulation
    env = types.SimpleNamespace(obs_dim=26, device="cpu")
    net = nn.Module()
    net.pi, net.v, net.log_std = _mlp(26, 2), _mlp(26, 1), nn.Parameter(torch.zeros(2))
    with pytest.raises(ValueError, match="squash.*frames"):
        FusedActorCritic(net, env, rollout=4, squash=True, frames=2)
    with pytest.raises(ValueError, match="squash.*normalize"):
        FusedActorCritic(net, env, rollout=4, squash=True, normalize=RunningNorm(26, 0.99))
    with pytest.raises(ValueError, match="squash.*bf16"):
        FusedActorCritic(net, env, rollout=4, squash=True, bf16=True)
    with pytest.raises(ValueError, match="squash"):
        PolicyPopulation(env, members=4, squash=True)
    with pytest.raises(ValueError, match="squash"):
        PolicyPopulation.base_state_into(types.SimpleNamespace(obs_dim=26, hidden=(256, 128, 64)), types.SimpleNamespace(squash=True))


# ------------------------------------------------------------------------------ the recorded bounds
def test_recorded_bounds_are_what_the_float32_mirrors_give():
    rec = cases.recorded()
    # the action map is NumPy, one rounding per operation: the same numbers on every machine
    me = cases.map_errors()
    assert rec["actions"]["mirror_error"] == me
    for k in range(2):
        floor = 4 * cases.ulp32(cases.MAP_HALF[k])
        assert rec["actions"]["floor"][k] == floor and rec["actions"]["bound"][k] == max(8 * me[k], floor)
        assert 0.0 < me[k] <= 4 * cases.ulp32(cases.MAP_HALF[k])          # a float32 tanh of a few ulp, scaled by half
    # the update's float32 pass runs through the host's matrix products, whose summation order is the BLAS's: the recorded errors are
    # held to a re-measurement within a factor of two, the bounds to the recorded errors exactly
    now = cases.update_errors()
    assert sorted(now) == sorted(rec["update"]) and len(now) == 2 * len(cases.HIDDEN) * len(cases.ENT_COEFS)
    for key, (eg, es) in now.items():
        r = rec["update"][key]
        assert 0.5 * eg <= r["mirror_error_grad"] <= 2.0 * eg and 0.5 * es <= r["mirror_error_stats"] <= 2.0 * es, (key, r, eg, es)
        assert r["bound_grad"] == max(8 * r["mirror_error_grad"], cases.UPDATE_FLOOR)
        assert r["bound_stats"] == max(8 * r["mirror_error_stats"], cases.UPDATE_FLOOR)
        assert r["bound_grad"] <= 1e-3 and r["bound_stats"] <= 1e-3       # float32 on sums of a few hundred rows, and no worse


# ------------------------------------------------------------------------------ resources
def _occupancy(vgpr):
    """Waves per SIMD the register file allows: 512 VGPRs, allocated in blocks of 8."""
    return 512 // (8 * ((vgpr + 7) // 8))


def _by_arch(kernels, body):
    out = {}
    for h in cases.HIDDEN:
        tag = "PolArchILi%dELi%dELi%dEE" % h
        k = [x for x in kernels if body in x["name"] and tag in x["name"] and "EEELb1E" not in x["name"]]
        assert len(k) == 1, (body, h, [x["name"] for x in kernels])
        out[h] = k[0]
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_squash_forward_kernels_keep_the_occupancy_of_their_plain_siblings():
    new = kernel_resources("k17_policy_squash.hip")
    assert len([k for k in new if "k17_" in k["name"]]) == 2 * len(cases.HIDDEN), [k["name"] for k in new]
    for body, src, sibling in (("k17_squash_act", "k6_policy.hip", "k6_policy_act"), ("k17_squash_eval", "k9_policy_eval.hip", "k9_policy_eval")):
        mine, plain = _by_arch(new, body), _by_arch(kernel_resources(src), sibling)
        for h in cases.HIDDEN:
            assert_policy_budget(mine[h])                   # 128 VGPRs, nothing spilled, no private segment, no static LDS
            assert _occupancy(mine[h]["vgpr"]) >= _occupancy(plain[h]["vgpr"]), (h, mine[h]["vgpr"], plain[h]["vgpr"])
            assert mine[h]["static_lds"] == plain[h]["static_lds"] == 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_squash_row_passes_keep_the_occupancy_of_the_ppo_row_passes():
    k8 = kernel_resources("k8_ppo_update.hip")
    sq = [k for k in k8 if "k8_squash" in k["name"]]
    rows = [k for k in k8 if "k8_rows" in k["name"]]
    assert len(sq) == 1 and len(rows) == 1, [k["name"] for k in k8]
    pairs = [(sq[0], rows[0])]
    k13 = kernel_resources("k13_ppo_update_arch.hip")
    assert not any("k8_squash" in k["name"] for k in k13)
    for h in cases.HIDDEN[1:]:
        tag = "PolArchILi%dELi%dELi%dEE" % h
        s = [k for k in k13 if "k13_ppo_squash" in k["name"] and tag in k["name"]]
        r = [k for k in k13 if "k13_ppo_rows" in k["name"] and tag in k["name"]]
        assert len(s) == 1 and len(r) == 1, (h, [k["name"] for k in k13])
        pairs.append((s[0], r[0]))
    for s, r in pairs:
        assert_policy_budget(s)
        # (launch bounds of four workgroups of eight waves per CU: at most eight waves per SIMD are asked for)
        assert min(_occupancy(s["vgpr"]), 8) >= min(_occupancy(r["vgpr"]), 8), (s["name"], s["vgpr"], r["vgpr"])
        assert s["static_lds"] == r["static_lds"] == 0
