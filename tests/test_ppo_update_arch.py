"""CPU: the fused PPO / clone update at the other hidden widths of POL_ARCH_LIST (csrc/auv_ppo_pass.h, k13_ppo_update_arch.hip) -- the C
ABI's two additions, the flat parameter count for every listed triple, what is refused before any device call, and the register
budget of every row-pass instantiation of the new translation unit (cross-compile only, read from the code object's metadata)."""
import ctypes as C
import os
import sys

import pytest
import torch

from gym_auv_amd import _capi
from gym_auv_amd.policy import HIDDEN, SUPPORTED_HIDDEN
from kernel_resources import HIPCC, assert_policy_budget, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
NEW = [h for h in SUPPORTED_HIDDEN if h != HIDDEN]
SYMBOLS = ["auv_ppo_param_floats_arch", "auv_ppo_create_arch"]


def _arch(h):
    return C.byref(_capi.AuvPolicyArch(*h))


def _net(obs_dim, hidden, pi_hidden=None):
    import ppo
    net = ppo.ActorCritic(obs_dim, hidden=hidden)
    if pi_hidden is not None:
        net.pi = ppo.ActorCritic(obs_dim, hidden=pi_hidden).pi
    return net


def test_new_symbols_are_declared_bound_and_exported():
    lib = _capi.load_library()
    hdr = open(os.path.join(ROOT, "include", "auv_hip.h")).read()
    for name in SYMBOLS:
        assert name + "(" in hdr, name
        assert name in _capi.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert lib.auv_abi_version() == _capi.ABI_VERSION == 5             # additions only


def test_the_list_is_the_forward_launches():
    from gym_auv_amd import ppo_update
    assert ppo_update.SUPPORTED_HIDDEN == SUPPORTED_HIDDEN and ppo_update.HIDDEN == HIDDEN == SUPPORTED_HIDDEN[0]
    assert len(NEW) == 3


@pytest.mark.parametrize("obs_dim", [6, 15, 186])
def test_param_floats_arch_is_the_module_s_parameter_count(obs_dim):
    lib = _capi.load_library()
    for h in SUPPORTED_HIDDEN:
        n = sum(p.numel() for p in _net(obs_dim, h).parameters())
        assert int(lib.auv_ppo_param_floats_arch(obs_dim, _arch(h))) == n, h
    assert int(lib.auv_ppo_param_floats_arch(obs_dim, _arch(HIDDEN))) == int(lib.auv_ppo_param_floats(obs_dim))
    assert int(lib.auv_ppo_param_floats_arch(obs_dim, _arch((64, 64, 32)))) == 0
    assert int(lib.auv_ppo_param_floats_arch(obs_dim, None)) == 0
    assert int(lib.auv_ppo_param_floats_arch(0, _arch((64, 64, 64)))) == 0
    assert int(lib.auv_ppo_param_floats_arch(-3, _arch(HIDDEN))) == 0


def test_create_arch_refuses_before_any_device_call():
    """No GPU here: a call that got as far as the device would fail with another code (AUV_EHIP) and another message."""
    lib = _capi.load_library()
    h = C.c_void_p()
    assert lib.auv_ppo_create_arch(0, 6, 64, _arch((64, 64, 32)), C.byref(h)) == -1 and not h.value
    assert b"(64, 64, 64)" in lib.auv_last_error()                     # the list is in the message
    assert lib.auv_ppo_create_arch(0, 6, 64, None, C.byref(h)) == -1 and not h.value
    assert b"null arch" in lib.auv_last_error()
    assert lib.auv_ppo_create_arch(0, 6, 64, _arch((64, 64, 64)), None) == -1
    assert b"null out" in lib.auv_last_error()


@pytest.mark.parametrize("kind", ["unlisted", "depth", "mixed"])
def test_fused_ppo_update_refuses_on_cpu_modules(kind):
    """The checks of the architecture come before the device check: CPU modules reach them."""
    from gym_auv_amd.ppo_update import FusedPPOUpdate
    if kind == "unlisted":
        net, match = _net(6, (64, 64, 32)), r"\(128, 64, 64\)"         # the list is in the message
    elif kind == "depth":
        net, match = _net(6, (64, 64)), "depth"
    else:
        net, match = _net(6, (64, 64, 64), pi_hidden=(128, 64, 64)), "same"
    with pytest.raises(ValueError, match=match):
        FusedPPOUpdate(net)


def test_a_listed_cpu_module_gets_as_far_as_the_device_check():
    from gym_auv_amd.ppo_update import FusedPPOUpdate
    with pytest.raises(ValueError, match="GPU"):
        FusedPPOUpdate(_net(6, (64, 64, 64)))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_every_row_pass_instantiation_fits_the_register_budget():
    """k13_ppo_update_arch.hip: exactly one PPO and one clone row pass per non-default triple (the default's stay in k8_ppo_update.hip,
    whose names these must not contain); each within the budget of the launch's shape -- 512 threads, four workgroups per CU at the
    narrow observation widths: 128 VGPRs, nothing spilled, no scratch, no static LDS in front of the dynamic tile -- and the clone pass,
    whose head does less, needs no more registers than the PPO pass of the same widths."""
    kernels = kernel_resources("k13_ppo_update_arch.hip")
    names = [k["name"] for k in kernels]
    assert not any("k8_rows" in n or "k8_clone" in n for n in names), names
    rows = [k for k in kernels if "k13_ppo_rows" in k["name"]]
    clone = [k for k in kernels if "k13_ppo_clone" in k["name"]]
    assert len(rows) == len(clone) == len(NEW), names
    assert not any("PolArchILi%dELi%dELi%dEE" % HIDDEN in n for n in names), names     # no second copy of the default's kernels
    for h in NEW:
        tag = "PolArchILi%dELi%dELi%dEE" % h
        r = [k for k in rows if tag in k["name"]]
        c = [k for k in clone if tag in k["name"]]
        assert len(r) == 1 and len(c) == 1, (h, names)
        assert_policy_budget(r[0])
        assert_policy_budget(c[0])
        assert c[0]["vgpr"] <= r[0]["vgpr"], (h, c[0]["vgpr"], r[0]["vgpr"])
