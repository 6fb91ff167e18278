"""CPU: the supervised (clone) row pass of the PPO updater (include/auv_hip.h, auv_ppo_grad_clone): the export is declared, bound and
present; the struct has the header's layout; bad arguments are refused before any device call; the head gradients the kernel
implements are the derivatives of ppo_update.clone_loss_terms; planning.DistillBuffer wraps and inverts as documented."""
import ctypes as C
import math
import os
import subprocess
import sys
import types

import pytest
import torch

from gym_auv_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))


def test_export_is_declared_bound_and_present_and_the_abi_version_stays():
    lib = _capi.load_library()
    hdr = open(os.path.join(ROOT, "include", "auv_hip.h")).read()
    assert "auv_ppo_grad_clone" in _capi.EXPORTED_SYMBOLS and "int auv_ppo_grad_clone(" in hdr
    assert lib.auv_ppo_grad_clone.argtypes is not None and lib.auv_ppo_grad_clone.restype is C.c_int
    assert _capi.ABI_VERSION == 5 and lib.auv_abi_version() == 5


def test_struct_layout_matches_the_header(tmp_path):
    names = [f[0] for f in _capi.AuvPpoCloneBatch._fields_]
    assert names == ["O", "A", "RET", "W", "idx", "B", "n_rows", "kind", "vf_coef", "ent_coef"]
    body = 'printf("%zu\\n", sizeof(auv_ppo_clone_batch_t));\n'
    body += "".join('printf("%%zu\\n", offsetof(auv_ppo_clone_batch_t, %s));\n' % f for f in names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){%sreturn 0;}\n' % (os.path.join(ROOT, "include", "auv_hip.h"), body))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert C.sizeof(_capi.AuvPpoCloneBatch) == out[0] == 5 * 8 + 5 * 4 + 4          # five pointers, five words, padded to 8
    for f, off in zip(names, out[1:]):
        assert getattr(_capi.AuvPpoCloneBatch, f).offset == off, f


def test_arguments_are_refused_before_any_device_call():
    """Every call below fails a check that comes before the first use of the updater: `one` is never dereferenced."""
    lib = _capi.load_library()
    one = C.c_void_p(16)
    B = _capi.AuvPpoCloneBatch

    def batch(O=16, A=16, RET=16, B_=4, kind=0):
        return B(O, A, RET, None, None, B_, 8, kind, 0.5, 0.0)
    calls = [("null argument", lambda: lib.auv_ppo_grad_clone(None, C.byref(batch()), one, one, None)),
             ("null argument", lambda: lib.auv_ppo_grad_clone(one, None, one, one, None)),
             ("null argument", lambda: lib.auv_ppo_grad_clone(one, C.byref(batch()), None, one, None)),
             ("null argument", lambda: lib.auv_ppo_grad_clone(one, C.byref(batch()), one, None, None)),
             ("null batch buffer", lambda: lib.auv_ppo_grad_clone(one, C.byref(batch(O=None)), one, one, None)),
             ("null batch buffer", lambda: lib.auv_ppo_grad_clone(one, C.byref(batch(A=None)), one, one, None)),
             ("null batch buffer", lambda: lib.auv_ppo_grad_clone(one, C.byref(batch(RET=None)), one, one, None)),
             ("kind = 2", lambda: lib.auv_ppo_grad_clone(one, C.byref(batch(kind=2)), one, one, None)),
             ("kind = -1", lambda: lib.auv_ppo_grad_clone(one, C.byref(batch(kind=-1)), one, one, None)),
             ("B = 0", lambda: lib.auv_ppo_grad_clone(one, C.byref(batch(B_=0)), one, one, None)),
             ("B = -3", lambda: lib.auv_ppo_grad_clone(one, C.byref(batch(B_=-3)), one, one, None))]
    for msg, call in calls:
        assert call() == -1, msg
        err = lib.auv_last_error().decode()
        assert "auv_ppo_grad_clone" in err and msg in err, (msg, err)


def test_clone_loss_terms_refuses_an_unknown_kind():
    from gym_auv_amd.ppo_update import clone_loss_terms
    with pytest.raises(ValueError, match="kind"):
        clone_loss_terms(None, None, None, None, kind="huber")


@pytest.mark.parametrize("kind", ["nll", "mse"])
def test_head_gradients_of_the_table_are_the_derivatives_of_clone_loss_terms(kind):
    """fp64, obs_dim 6, B 5, weights with a zero: d loss / d mu, d loss / d v and d loss / d log_std as the kernel's head forms them
    (the table of include/auv_hip.h and k8_ppo_update.hip) against autograd through clone_loss_terms, to 1e-12."""
    import ppo
    from gym_auv_amd.ppo_update import clone_loss_terms
    torch.manual_seed(0)
    B, D, vf_coef, ent_coef = 5, 6, 0.7, 0.03
    net = ppo.ActorCritic(D).double()
    with torch.no_grad():
        net.log_std.copy_(torch.tensor([-0.5, 0.3], dtype=torch.float64))
    o = torch.randn(B, D, dtype=torch.float64)
    a, ret = torch.randn(B, 2, dtype=torch.float64), torch.randn(B, dtype=torch.float64)
    w = torch.tensor([1.0, 0.0, 2.5, 0.25, 1.0], dtype=torch.float64)
    mu = net.pi(o).detach().requires_grad_(True)
    v = net.v(o).detach().requires_grad_(True)
    ls = net.log_std.detach().clone().requires_grad_(True)
    heads = types.SimpleNamespace(pi=lambda _: mu, v=lambda _: v, log_std=ls)
    loss, bc, vf = clone_loss_terms(heads, o, a, ret, w, kind, vf_coef, ent_coef)
    # the terms themselves, and that the module gives them too
    loss_m, bc_m, vf_m = clone_loss_terms(net, o, a, ret, w, kind, vf_coef, ent_coef)
    assert float((loss - loss_m).detach()) == 0.0 and float((bc - bc_m).detach()) == 0.0 and float((vf - vf_m).detach()) == 0.0
    sigma, c = ls.detach().exp(), 0.5 * math.log(2.0 * math.pi)
    e = a - mu.detach()
    z = e / sigma
    bc_hand = (w[:, None] * (0.5 * z * z + ls.detach() + c)).sum() / B if kind == "nll" else (w[:, None] * 0.5 * e * e).sum() / B
    vf_hand = (w * 0.5 * (v.detach().squeeze(-1) - ret) ** 2).sum() / B
    loss_hand = bc_hand + vf_coef * vf_hand - ent_coef * (0.5 + c + ls.detach()).sum()
    assert all(abs(float((x - y).detach())) <= 1e-12 for x, y in ((bc, bc_hand), (vf, vf_hand), (loss, loss_hand)))
    g_mu, g_v, g_ls = torch.autograd.grad(loss, [mu, v, ls])
    if kind == "nll":
        hand_mu = -w[:, None] * e / (sigma * sigma) / B
        hand_ls = (w[:, None] * (1.0 - z * z)).sum(0) / B - ent_coef
    else:
        hand_mu = -w[:, None] * e / B
        hand_ls = torch.full((2,), -ent_coef, dtype=torch.float64)
    hand_v = (vf_coef * w * (v.detach().squeeze(-1) - ret) / B)[:, None]
    for name, x, y in (("mu", g_mu, hand_mu), ("v", g_v, hand_v), ("log_std", g_ls, hand_ls)):
        assert float((x - y).abs().max()) <= 1e-12, (name, x, y)
    assert float(g_mu[1].abs().max()) == 0.0 and float(g_v[1].abs().max()) == 0.0      # the row of weight zero


def test_distill_buffer_ring_wraps():
    from gym_auv_amd.planning import DistillBuffer
    buf = DistillBuffer(8, 3, "cpu")

    def rows(lo, n):
        k = torch.arange(lo, lo + n, dtype=torch.float32)
        return k[:, None].expand(n, 3).contiguous(), torch.stack([k, -k], 1), 10.0 * k, 0.5 * k
    with pytest.raises(ValueError):
        buf.sample(4)
    buf.add(*rows(0, 5))
    assert (buf.size, buf.head) == (5, 5) and buf.RET[:5].tolist() == [0.0, 10.0, 20.0, 30.0, 40.0]
    g = torch.Generator().manual_seed(0)
    idx = buf.sample(64, g)
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (64,) and int(idx.min()) >= 0 and int(idx.max()) <= 4
    o, a, r, _ = rows(5, 6)
    buf.add(o, a, r)                                                 # rows 5 .. 10 at positions 5, 6, 7, 0, 1, 2; weights default to one
    assert (buf.size, buf.head) == (8, 3)
    assert buf.RET.tolist() == [80.0, 90.0, 100.0, 30.0, 40.0, 50.0, 60.0, 70.0]
    assert buf.O[:, 2].tolist() == [8.0, 9.0, 10.0, 3.0, 4.0, 5.0, 6.0, 7.0]
    assert buf.A[0].tolist() == [8.0, -8.0]
    assert buf.W.tolist() == [1.0, 1.0, 1.0, 1.5, 2.0, 1.0, 1.0, 1.0]
    assert int(buf.sample(256, g).max()) == 7
    buf.add(*rows(100, 19))                                          # longer than the ring: the last eight stay, the head moves by 19
    assert (buf.size, buf.head) == (8, (3 + 19) % 8)
    assert sorted(buf.RET.tolist()) == [10.0 * k for k in range(111, 119)]
    assert buf.RET[(buf.head - 1) % 8] == 1180.0 and buf.RET[buf.head] == 1110.0
    with pytest.raises(ValueError):
        buf.add(torch.zeros(2, 4), torch.zeros(2, 2), torch.zeros(2))


def test_targets_from_plan_inverts_the_action_map_and_the_value_scaling():
    from gym_auv_amd.planning import DistillBuffer
    prior = types.SimpleNamespace(action_map=((0.5, 0.0), (0.5, 0.25), (-1.0, -1.0), (1.0, 1.0)))
    planner = types.SimpleNamespace(prior=prior, value_scale=4.0, value_shift=-2.0)
    mu = torch.tensor([[-1.0, 1.0], [0.0, -0.5], [0.75, 0.125]])
    value = torch.tensor([3.0, -1.5, 0.25])
    actions = torch.tensor([0.5, 0.0]) + torch.tensor([0.5, 0.25]) * mu       # (powers of two: every step is exact)
    a, ret = DistillBuffer.targets_from_plan(planner, actions, value * 4.0 - 2.0)
    assert torch.equal(a, mu) and torch.equal(ret, value)
    # no prior, no scaling: the identity
    a, ret = DistillBuffer.targets_from_plan(types.SimpleNamespace(prior=None, value_scale=1.0, value_shift=0.0), actions, value)
    assert torch.equal(a, actions) and torch.equal(ret, value)
    prior.action_map = ((0.5, 0.0), (0.5, 0.0), (-1.0, -1.0), (1.0, 1.0))
    with pytest.raises(ValueError, match="zero"):
        DistillBuffer.targets_from_plan(planner, actions, value)
