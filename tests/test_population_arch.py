"""CPU: the population's contract at the other hidden widths of POL_ARCH_LIST (gym_auv_amd/population.py with hidden=; the
auv_population_*_arch entries; csrc/auv_population_pass.h, k14_population_arch.hip) -- the NumPy mirrors tests/test_gpu_population_arch.py
holds the kernels to, the member size on both sides of the C ABI, and what PolicyPopulation decides before it touches a device."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from gym_auv_amd import _capi
from gym_auv_amd import population as pop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = (256, 128, 64)
OTHERS = [(128, 128, 64), (128, 64, 64), (64, 64, 64)]
UNLISTED = [(64, 64, 128), (256, 128, 128), (256, 128), (32, 32, 32), (0, 0, 0)]
NEW_SYMBOLS = ("auv_population_member_floats_arch", "auv_population_act_arch", "auv_population_rollout_arch", "auv_population_perturb_arch",
               "auv_population_update_arch")


def _true_params(obs_dim, hidden):
    h1, h2, h3 = hidden
    return obs_dim * h1 + h1 + h1 * h2 + h2 + h2 * h3 + h3 + 2 * h3 + 2


def _sequential(obs_dim, hidden, fill=None):
    import torch
    import torch.nn as nn
    dims = (obs_dim,) + tuple(hidden)
    layers = []
    for a, b in zip(dims[:-1], dims[1:]):
        layers += [nn.Linear(a, b), nn.Tanh()]
    layers.append(nn.Linear(dims[-1], 2))
    net = nn.Sequential(*layers)
    if fill is not None:
        with torch.no_grad():
            for p in net.parameters():
                p.fill_(fill)
    return net


def test_the_list_is_the_policy_launches_list():
    assert _capi.POLICY_ARCHS[0] == DEFAULT == pop.HIDDEN and sorted(_capi.POLICY_ARCHS[1:]) == sorted(OTHERS)


@pytest.mark.parametrize("hidden", OTHERS + [DEFAULT])
@pytest.mark.parametrize("obs_dim", [6, 15, 186])
def test_padding_mask_leaves_exactly_the_nets_parameters(obs_dim, hidden):
    h1, h2, h3 = hidden
    mask = pop.padding_mask(obs_dim, hidden)
    assert mask.dtype == bool and mask.shape == (pop.member_floats(obs_dim, hidden),)
    assert int((~mask).sum()) == _true_params(obs_dim, hidden)
    # b1 (behind W1) has no padding; b4 (the last 16 floats) keeps its first two entries
    k0p = (obs_dim + 31) & ~31
    assert not mask[h1 * k0p:h1 * k0p + h1].any()
    assert not mask[-16:-14].any() and mask[-14:].all()
    # ... and is what packing all-ones weights through pack_member leaves at zero
    block = pop.pack_member(_sequential(obs_dim, hidden, fill=1.0), obs_dim, hidden=hidden).numpy()
    assert block.shape == mask.shape and np.array_equal(block == 0.0, mask) and np.array_equal(block[~mask], np.ones(int((~mask).sum()), np.float32))
    if hidden == DEFAULT:
        assert np.array_equal(mask, pop.padding_mask(obs_dim))
        assert np.array_equal(block, pop.pack_member(_sequential(obs_dim, hidden, fill=1.0), obs_dim).numpy())


@pytest.mark.parametrize("hidden", OTHERS + [DEFAULT])
def test_member_floats_is_the_policy_half_of_the_packed_buffer(hidden):
    from gym_auv_amd.policy import policy_param_floats
    lib = _capi.load_library()
    arch = _capi.AuvPolicyArch(*hidden)
    h1, h2, h3 = hidden
    for obs_dim in (1, 6, 15, 32, 33, 186):
        nf = pop.member_floats(obs_dim, hidden)
        k0p = (obs_dim + 31) & ~31
        assert nf % 4 == 0 and nf == (h1 * k0p + h1 + h2 * h1 + h2 + h3 * h2 + h3 + 16 * h3 + 16 + 3) // 4 * 4
        half = (policy_param_floats(obs_dim, hidden) - 4) // 2
        assert nf == (half + 3) // 4 * 4
        assert int(lib.auv_population_member_floats_arch(obs_dim, C.byref(arch))) == nf
        if hidden == DEFAULT:
            assert nf == pop.member_floats(obs_dim) == int(lib.auv_population_member_floats(obs_dim))
    assert int(lib.auv_population_member_floats_arch(0, C.byref(arch))) == 0
    assert int(lib.auv_population_member_floats_arch(-3, C.byref(arch))) == 0
    assert int(lib.auv_population_member_floats_arch(6, None)) == 0


@pytest.mark.parametrize("hidden", UNLISTED)
def test_an_unlisted_triple_has_no_member_size(hidden):
    lib = _capi.load_library()
    if len(hidden) == 3:
        assert int(lib.auv_population_member_floats_arch(6, C.byref(_capi.AuvPolicyArch(*hidden)))) == 0      # never rounded to a listed one
    for fn in (lambda: pop.member_floats(6, hidden), lambda: pop.padding_mask(6, hidden),
               lambda: pop.perturb_reference(np.zeros(4, np.float32), 2, 6, 0.1, 1, 0, hidden=hidden),
               lambda: pop.es_update_reference(np.zeros(4, np.float32), np.zeros(2, np.float32), 6, 0.1, 0.1, 1, 0, hidden=hidden)):
        with pytest.raises(ValueError):
            fn()


@pytest.mark.parametrize("hidden", OTHERS)
@pytest.mark.parametrize("obs_dim", [6, 15])
def test_perturb_reference_mirrors_pairs_and_spares_padding(obs_dim, hidden):
    nf = pop.member_floats(obs_dim, hidden)
    assert nf < pop.member_floats(obs_dim)
    rs = np.random.RandomState(obs_dim)
    mask = pop.padding_mask(obs_dim, hidden)
    theta = np.where(mask, 0.0, rs.randn(nf)).astype(np.float32)
    m = pop.perturb_reference(theta, 6, obs_dim, 0.02, seed=9, generation=4, stride=nf + 8, hidden=hidden)
    assert m.shape == (6, nf + 8) and m.dtype == np.float32 and not m[:, nf:].any()
    for j in range(3):
        up, dn = m[2 * j, :nf].astype(np.float64) - theta, m[2 * j + 1, :nf].astype(np.float64) - theta
        d = (np.float32(0.02) * pop.es_noise(9, 4, j, np.arange(nf))).astype(np.float64)
        # theta + d and theta - d, each rounded once: within half an ulp of the sum of the exact +-d
        big = np.maximum(np.abs(theta), np.maximum(np.abs(m[2 * j, :nf]), np.abs(m[2 * j + 1, :nf])))
        ulp = np.spacing(big.astype(np.float32)).astype(np.float64)
        assert (np.abs(up - d)[~mask] <= 0.5 * ulp[~mask]).all() and (np.abs(dn + d)[~mask] <= 0.5 * ulp[~mask]).all()
        assert np.array_equal(m[2 * j, :nf][mask], theta[mask]) and np.array_equal(m[2 * j + 1, :nf][mask], theta[mask])
        assert (up[~mask] != 0).mean() > 0.99
    # around theta = 0 the pair is exactly opposite
    z = pop.perturb_reference(np.zeros(nf, np.float32), 2, obs_dim, 0.02, seed=9, generation=4, hidden=hidden)
    assert np.array_equal(z[0], -z[1]) and not z[0][mask].any()
    assert not np.array_equal(m[0], m[2])
    assert not np.array_equal(m[0, :nf], pop.perturb_reference(theta, 2, obs_dim, 0.02, 9, 5, hidden=hidden)[0])
    # a block of the default's size is refused: the widths decide the block
    with pytest.raises(AssertionError):
        pop.perturb_reference(np.zeros(pop.member_floats(obs_dim), np.float32), 2, obs_dim, 0.02, 9, 4, hidden=hidden)


@pytest.mark.parametrize("hidden", OTHERS)
@pytest.mark.parametrize("obs_dim", [6, 15])
def test_es_update_reference_spares_padding_and_is_zero_for_equal_weights(obs_dim, hidden):
    nf = pop.member_floats(obs_dim, hidden)
    mask = pop.padding_mask(obs_dim, hidden)
    theta = np.linspace(-1, 1, nf).astype(np.float32)
    grad, new = pop.es_update_reference(theta, np.full(8, 0.37, np.float32), obs_dim, 0.05, 0.1, seed=2, generation=11, hidden=hidden)
    assert grad.dtype == np.float32 and grad.shape == (nf,) and not grad.view(np.uint32).any()
    assert np.array_equal(new.view(np.uint32), theta.view(np.uint32))
    w = np.random.RandomState(1).randn(8).astype(np.float32)
    grad, new = pop.es_update_reference(theta, w, obs_dim, 0.05, 0.1, seed=2, generation=11, hidden=hidden)
    assert not grad[mask].view(np.uint32).any() and np.array_equal(new[mask].view(np.uint32), theta[mask].view(np.uint32))
    assert (grad[~mask] != 0).mean() > 0.99 and (new[~mask] != theta[~mask]).mean() > 0.9
    # the estimate of a live element is the same number whatever the widths: the noise is keyed by the element's index alone
    acc = np.zeros(nf, np.float32)
    for pair in range(4):
        acc = acc + np.float32(w[2 * pair] - w[2 * pair + 1]) * pop.es_noise(2, 11, pair, np.arange(nf))
    assert np.array_equal(grad[~mask], (acc * np.float32(1.0 / (8 * float(np.float32(0.05)))))[~mask])


@pytest.mark.parametrize("hidden", OTHERS + [DEFAULT])
def test_the_constructor_reads_the_triple_off_the_module(hidden):
    net = _sequential(6, hidden)
    assert pop.net_hidden(net) == hidden
    assert pop.PolicyPopulation.resolve_hidden(net) == hidden
    assert pop.PolicyPopulation.resolve_hidden(SimpleNamespace(pi=net)) == hidden
    assert pop.PolicyPopulation.resolve_hidden(None, hidden) == hidden and pop.PolicyPopulation.resolve_hidden(None, list(hidden)) == hidden
    assert pop.PolicyPopulation.resolve_hidden(net, hidden) == hidden
    assert pop.PolicyPopulation.resolve_hidden() == DEFAULT
    other = OTHERS[0] if hidden != OTHERS[0] else OTHERS[1]
    with pytest.raises(ValueError):
        pop.PolicyPopulation.resolve_hidden(net, other)          # hidden= contradicts the net
    with pytest.raises(ValueError):
        pop.pack_member(net, 6, hidden=other)
    if hidden != DEFAULT:
        with pytest.raises(ValueError):
            pop.pack_member(net, 6)                              # the keyword-less call still means the reference's widths


def test_the_constructor_refuses_an_unlisted_triple_before_it_touches_a_device():
    env = SimpleNamespace(n_envs=96, obs_dim=6)                  # (no device, no handle: anything past the checks would raise AttributeError)
    for hidden in UNLISTED:
        with pytest.raises(ValueError):
            pop.PolicyPopulation(env, 3, 32, hidden=hidden)
        if len(hidden) == 3 and min(hidden) > 0:
            with pytest.raises(ValueError):
                pop.PolicyPopulation(env, 3, 32, net=_sequential(6, hidden))
    with pytest.raises(ValueError):
        pop.PolicyPopulation(env, 3, 32, net=_sequential(6, (64, 64, 64)), hidden=(128, 64, 64))
    with pytest.raises(ValueError):
        pop.PolicyPopulation(env, 5, None, hidden=(64, 64, 64))  # the geometry is still checked first
    # a listed triple passes the checks and goes on to the device it does not have here
    with pytest.raises(AttributeError):
        pop.PolicyPopulation(env, 3, 32, hidden=(64, 64, 64))


def test_base_state_into_refuses_other_hidden_widths():
    p = pop.PolicyPopulation.__new__(pop.PolicyPopulation)
    p.obs_dim, p.hidden, p.nf = 6, (64, 64, 64), pop.member_floats(6, (64, 64, 64))
    with pytest.raises(ValueError):
        p.base_state_into(SimpleNamespace(env=SimpleNamespace(obs_dim=6), hidden=(256, 128, 64)))
    with pytest.raises(ValueError):
        p.base_state_into(SimpleNamespace(env=SimpleNamespace(obs_dim=7), hidden=(64, 64, 64)))


def test_new_symbols_are_in_the_header_and_the_binding(tmp_path):
    header = open(os.path.join(ROOT, "include", "auv_hip.h")).read()
    lib = _capi.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert "evaluate (256, 128, 64) only" not in header
    assert lib.auv_abi_version() == _capi.ABI_VERSION == 5
    # the structs the new entries take are the ones the plain entries take: sizes unchanged
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "%s"\nint main(){printf("%%zu %%zu\\n", sizeof(auv_population_io_t), sizeof(auv_policy_arch_t));'
                   'return 0;}\n' % os.path.join(ROOT, "include", "auv_hip.h"))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    io_size, arch_size = map(int, subprocess.check_output([str(exe)]).split())
    assert C.sizeof(_capi.AuvPopulationIO) == io_size == 136 and C.sizeof(_capi.AuvPolicyArch) == arch_size == 12
