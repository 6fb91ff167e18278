"""CPU: hidden widths other than [256, 128, 64] in the fused forward launches (csrc/auv_policy_mfma.h: PolArch, POL_ARCH_LIST) -- the C
ABI's additions (auv_policy_arch_t, the *_arch entries), the packed layout for every listed triple, what is refused, and the register
budget of every instantiation of the three forward launches (cross-compile only, read from the code object's metadata)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from gym_auv_amd import _capi
from gym_auv_amd.policy import HIDDEN, SUPPORTED_HIDDEN, _pad16, pack_policy_params, policy_param_floats
from kernel_resources import HIPCC, assert_policy_budget, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
NEW = [(128, 128, 64), (128, 64, 64), (64, 64, 64)]
ARCH_SYMBOLS = ["auv_policy_param_floats_arch", "auv_policy_act_arch", "auv_policy_rollout_arch", "auv_policy_act_stacked_arch",
                "auv_policy_rollout_stacked_arch", "auv_policy_eval_arch"]


def _net(obs_dim, hidden, pi_hidden=None, seed=3):
    import ppo
    torch.manual_seed(seed)
    net = ppo.ActorCritic(obs_dim, hidden=hidden)
    if pi_hidden is not None:
        net.pi = ppo.ActorCritic(obs_dim, hidden=pi_hidden).pi
    with torch.no_grad():
        net.log_std.copy_(torch.tensor([-0.5, -1.1]))
        for m in net.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.uniform_(-0.3, 0.3)
    return net


def test_the_list_of_triples_and_its_default():
    assert SUPPORTED_HIDDEN == ((256, 128, 64),) + tuple(NEW) and SUPPORTED_HIDDEN[0] == HIDDEN
    # ... and it is the list of the header, in its order: one line per triple, the default first
    hdr = open(os.path.join(ROOT, "gym_auv_amd", "csrc", "auv_policy_mfma.h")).read()
    block = hdr[hdr.index("#define POL_ARCH_LIST(X)"):]
    block = block[:block.index("__host__")]
    listed = [tuple(int(x) for x in m) for m in re.findall(r"X\((\d+), (\d+), (\d+)\)", block)]
    assert tuple(listed) == SUPPORTED_HIDDEN and listed[0] == HIDDEN
    ref = tuple(int(re.search(r"#define POL_H%d (\d+)" % i, hdr).group(1)) for i in (1, 2, 3))      # what PolArchRef is made of
    assert ref == HIDDEN


def test_arch_struct_has_the_header_s_size(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu %%d\\n", '
                   'sizeof(auv_policy_arch_t), offsetof(auv_policy_arch_t, h2), offsetof(auv_policy_arch_t, h3), '
                   'sizeof(auv_policy_io_t), AUV_ABI_VERSION);return 0;}\n' % os.path.join(ROOT, "include", "auv_hip.h"))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    size, o2, o3, io_size, abi = map(int, subprocess.check_output([str(exe)]).split())
    assert C.sizeof(_capi.AuvPolicyArch) == size == 12
    assert _capi.AuvPolicyArch.h2.offset == o2 == 4 and _capi.AuvPolicyArch.h3.offset == o3 == 8
    assert C.sizeof(_capi.AuvPolicyIO) == io_size and abi == _capi.ABI_VERSION == 5      # additions only


def test_new_symbols_are_exported():
    lib = _capi.load_library()
    for name in ARCH_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _capi.EXPORTED_SYMBOLS, name


def _formula(h, obs_dim):
    """The layout comment of csrc/auv_policy_mfma.h: W1 [H1][K0p] b1 [H1] W2 [H2][H1] b2 [H2] W3 [H3][H2] b3 [H3] W4 [16][H3] b4 [16],
    two nets and four floats (log_std, padded)."""
    h1, h2, h3 = h
    k0p = (obs_dim + 31) // 32 * 32
    return 2 * (h1 * k0p + h1 + h2 * h1 + h2 + h3 * h2 + h3 + 16 * h3 + 16) + 4


@pytest.mark.parametrize("obs_dim", [6, 15, 186])
def test_param_floats_arch(obs_dim):
    lib = _capi.load_library()
    f = lambda h: int(lib.auv_policy_param_floats_arch(obs_dim, C.byref(_capi.AuvPolicyArch(*h))))   # noqa: E731
    assert f(HIDDEN) == int(lib.auv_policy_param_floats(obs_dim)) == _formula(HIDDEN, obs_dim)
    for h in NEW:
        assert f(h) == _formula(h, obs_dim) == policy_param_floats(obs_dim, h), h
    # outside the list: 0, never the size of a listed neighbour; NULL and obs_dim < 1 likewise
    for h in [(64, 64, 32), (256, 128, 128), (192, 128, 64), (64, 128, 64), (0, 0, 0), (-64, 64, 64), (128, 128, 128)]:
        assert f(h) == 0, h
    assert int(lib.auv_policy_param_floats_arch(obs_dim, None)) == 0
    assert int(lib.auv_policy_param_floats_arch(0, C.byref(_capi.AuvPolicyArch(64, 64, 64)))) == 0


def _unpack(frag, out_pad, in_pad):
    """pack_linear's inverse in NumPy: [n-tile][k-step J][half h][group g][row n][4] -> [out_pad][in_pad], lane 16 g + n of a wave holds
    k = 32 J + 8 g + 4 h + (0..3) of row n of the tile."""
    w = np.zeros((out_pad, in_pad), dtype=np.float32)
    f = frag.reshape(out_pad // 16, in_pad // 32, 2, 4, 16, 4)
    for t in range(out_pad // 16):
        for J in range(in_pad // 32):
            for h in range(2):
                for g in range(4):
                    k = 32 * J + 8 * g + 4 * h
                    w[16 * t:16 * t + 16, k:k + 4] = f[t, J, h, g]
    return w


@pytest.mark.parametrize("hidden", NEW)
@pytest.mark.parametrize("obs_dim", [6, 15])
def test_pack_round_trips_and_pads_with_zeros(hidden, obs_dim):
    net = _net(obs_dim, hidden)
    p = pack_policy_params(net, obs_dim, hidden=hidden).numpy()
    assert p.size == _formula(hidden, obs_dim)
    k0p = _pad16(obs_dim)
    off = 0
    for seq in (net.pi, net.v):
        lin = [m for m in seq if isinstance(m, torch.nn.Linear)]
        assert tuple(l.out_features for l in lin[:-1]) == hidden
        for j, l in enumerate(lin):
            out_p = l.out_features if j < 3 else 16
            in_p = k0p if j == 0 else l.in_features
            w = _unpack(p[off:off + out_p * in_p], out_p, in_p)
            off += out_p * in_p
            ref = l.weight.detach().numpy()
            assert np.array_equal(w[:ref.shape[0], :ref.shape[1]], ref), (hidden, j)
            w[:ref.shape[0], :ref.shape[1]] = 0.0
            assert not w.any(), (hidden, j)                                     # padding rows and columns
            b = p[off:off + out_p]
            off += out_p
            assert np.array_equal(b[:l.out_features], l.bias.detach().numpy()) and not b[l.out_features:].any()
    assert np.array_equal(p[off:off + 2], net.log_std.detach().numpy()) and not p[off + 2:].any() and off + 4 == p.size


def test_pack_refuses_what_is_not_listed():
    with pytest.raises(ValueError, match=r"\(64, 64, 64\)"):                    # the list is in the message
        pack_policy_params(_net(6, (64, 64, 32)), 6, hidden=(64, 64, 32))
    with pytest.raises(ValueError, match="depth"):
        pack_policy_params(_net(6, (64, 64)), 6, hidden=(64, 64))
    with pytest.raises(ValueError):                                             # the net is not what `hidden` says
        pack_policy_params(_net(6, (64, 64, 64)), 6, hidden=(128, 64, 64))
    with pytest.raises(ValueError):                                             # ... nor the default
        pack_policy_params(_net(6, (64, 64, 64)), 6)
    with pytest.raises(ValueError):                                             # a mixed pair
        pack_policy_params(_net(6, (64, 64, 64), pi_hidden=(128, 64, 64)), 6, hidden=(64, 64, 64))


class _Env:
    """What FusedActorCritic reads of an environment before it allocates anything."""
    obs_dim, device = 6, "cpu"


@pytest.mark.parametrize("kind", ["unlisted", "depth", "mixed", "bf16"])
def test_fused_actor_critic_refuses(kind):
    from gym_auv_amd.policy import FusedActorCritic
    kw = {}
    if kind == "unlisted":
        net, match = _net(6, (64, 64, 32)), r"\(128, 64, 64\)"
    elif kind == "depth":
        net, match = _net(6, (64, 64)), "depth"
    elif kind == "mixed":
        net, match = _net(6, (64, 64, 64), pi_hidden=(128, 64, 64)), "same"
    else:
        net, match, kw = _net(6, (128, 64, 64)), "bf16", dict(bf16=True)
    with pytest.raises(ValueError, match=match):
        FusedActorCritic(net, _Env(), rollout=3, **kw)


def test_fused_update_and_population_keep_refusing():
    from gym_auv_amd import population, ppo_update
    assert ppo_update.HIDDEN == population.HIDDEN == HIDDEN
    with pytest.raises(ValueError):
        population.pack_member(_net(6, (64, 64, 64)).pi, 6)


# ---- the register budget of every instantiation of the three forward launches (tests/kernel_resources.py) ----
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src,kernel", [("k6_policy.hip", "k6_policy_act"), ("k9_policy_eval.hip", "k9_policy_eval"),
                                        ("k12_policy_stacked.hip", "k12_stacked_act")])
def test_every_instantiation_fits_the_register_budget(src, kernel):
    blocks = [k for k in kernel_resources(src) if kernel in k["name"]]
    names = sorted(k["name"] for k in blocks)
    # one instantiation per listed triple: the template arguments are in the mangled name (k6: <triple, BF>, BF = true -- bf16 weights --
    # for the default triple only)
    f32 = [x for x in names if "EEELb1E" not in x]
    assert len(f32) == len(SUPPORTED_HIDDEN), names
    for h in SUPPORTED_HIDDEN:
        assert sum("PolArchILi%dELi%dELi%dEE" % h in x for x in f32) == 1, (h, names)
    bf = [x for x in names if "EEELb1E" in x]
    assert len(bf) == (1 if kernel == "k6_policy_act" else 0), names
    assert all("PolArchILi%dELi%dELi%dEEELb1E" % HIDDEN in x for x in bf), names
    for k in blocks:
        assert_policy_budget(k)
