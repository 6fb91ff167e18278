"""CPU: the contract of the population kernels (gym_auv_amd/population.py) -- the NumPy mirrors that csrc/k11_population.hip is held
to bit for bit in tests/test_gpu_population.py -- and the argument checks of PolicyPopulation that need no device."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from gym_auv_amd import population as pop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = [(0, 0, 0), (1, 5, 3), (12345, 7, 127)]


def _true_params(obs_dim):
    return obs_dim * 256 + 256 + 256 * 128 + 128 + 128 * 64 + 64 + 64 * 2 + 2


@pytest.mark.parametrize("obs_dim", [6, 15, 186])
def test_padding_mask_leaves_exactly_the_nets_parameters(obs_dim):
    mask = pop.padding_mask(obs_dim)
    assert mask.dtype == bool and mask.shape == (pop.member_floats(obs_dim),)
    assert int((~mask).sum()) == _true_params(obs_dim)
    # b1 (behind W1) has no padding; b4 (the last 16 floats) keeps its first two entries
    k0p = (obs_dim + 31) & ~31
    assert not mask[256 * k0p:256 * k0p + 256].any()
    assert not mask[-16:-14].any() and mask[-14:].all()


def test_member_floats_is_the_policy_half_of_the_packed_buffer():
    from gym_auv_amd import _capi
    lib = _capi.load_library()
    for obs_dim in (1, 6, 15, 32, 33, 186):
        assert int(lib.auv_population_member_floats(obs_dim)) == pop.member_floats(obs_dim)
        assert 2 * pop.member_floats(obs_dim) + 4 == int(lib.auv_policy_param_floats(obs_dim))
    assert int(lib.auv_population_member_floats(0)) == 0


@pytest.mark.parametrize("seed,gen,pair", KEYS)
def test_es_noise_moments_and_bound(seed, gen, pair):
    eps = pop.es_noise(seed, gen, pair, np.arange(1 << 20))
    assert eps.dtype == np.float32 and eps.shape == (1 << 20,)
    e = eps.astype(np.float64)
    print("key %s: mean %.3e var %.5f max |eps| %.5f" % ((seed, gen, pair), e.mean(), e.var(), np.abs(e).max()))
    assert abs(e.mean()) < 5e-3                      # five standard errors of 2^-10
    assert abs(e.var() - 1.0) < 1e-2                 # the standard error is ~1.3e-3
    assert np.abs(e).max() <= 3.4642
    # another pair of the same key is another stream
    other = pop.es_noise(seed, gen, pair + 1, np.arange(100000)).astype(np.float64)
    c = np.corrcoef(e[:100000], other)[0, 1]
    print("  correlation with pair + 1: %.4f" % c)
    assert abs(c) < 0.02


def test_es_noise_is_one_rounded_product_of_an_integer():
    i = np.arange(1000)
    eps = pop.es_noise(3, 2, 1, i)
    S = np.rint(eps.astype(np.float64) / float(pop.EPS_SCALE)).astype(np.int64)
    assert (np.abs(S) <= 131070).all()
    assert np.array_equal((S.astype(np.float32) * pop.EPS_SCALE).view(np.uint32), eps.view(np.uint32))
    assert float(np.float32(131070) * pop.EPS_SCALE) <= 3.4642
    # the key is (seed, generation, pair, index): each part matters, and pair / index broadcast
    assert not np.array_equal(eps, pop.es_noise(4, 2, 1, i)) and not np.array_equal(eps, pop.es_noise(3, 3, 1, i))
    both = pop.es_noise(3, 2, np.array([[1], [2]]), i[None, :])
    assert both.shape == (2, 1000) and np.array_equal(both[0], eps) and np.array_equal(both[1], pop.es_noise(3, 2, 2, i))


@pytest.mark.parametrize("obs_dim", [6, 15])
def test_perturb_reference_mirrors_pairs_and_spares_padding(obs_dim):
    nf = pop.member_floats(obs_dim)
    rs = np.random.RandomState(obs_dim)
    mask = pop.padding_mask(obs_dim)
    theta = np.where(mask, 0.0, rs.randn(nf)).astype(np.float32)
    m = pop.perturb_reference(theta, 6, obs_dim, 0.02, seed=9, generation=4, stride=nf + 8)
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
    z = pop.perturb_reference(np.zeros(nf, np.float32), 2, obs_dim, 0.02, seed=9, generation=4)
    assert np.array_equal(z[0], -z[1]) and not z[0][mask].any()
    assert not np.array_equal(m[0], m[2]) and not np.array_equal(m[0, :nf], pop.perturb_reference(theta, 2, obs_dim, 0.02, 9, 5)[0])


def test_es_update_reference_with_equal_weights_is_exactly_zero():
    nf = pop.member_floats(6)
    theta = np.linspace(-1, 1, nf).astype(np.float32)
    grad, new = pop.es_update_reference(theta, np.full(8, 0.37, np.float32), 6, 0.05, 0.1, seed=2, generation=11)
    assert grad.dtype == np.float32 and not grad.view(np.uint32).any()
    assert np.array_equal(new.view(np.uint32), theta.view(np.uint32))


def test_mirrors_descend_a_quadratic():
    """f(theta) = -|theta - target|^2 over the live elements, obs_dim 6, P = 32: 50 generations of perturb -> centred ranks -> update
    move theta towards the target (sign and scale of the estimate).  32 members see 32 directions of ~42 000: with rank weights the
    estimate is mostly noise of size ~1 per element, its component along the true gradient ~ |d| / (6 sigma) -- the step that gains
    most is lr ~ 1e-3, and it gains ~0.1 per generation on |d|^2 ~ 430; a step ten times that would walk away."""
    obs_dim, P, sigma, lr = 6, 32, 0.05, 1e-3
    nf = pop.member_floats(obs_dim)
    live = ~pop.padding_mask(obs_dim)
    rs = np.random.RandomState(0)
    target = np.where(live, rs.randn(nf) * 0.1, 0.0).astype(np.float32)
    theta = np.zeros(nf, dtype=np.float32)
    d0 = float(np.linalg.norm((theta - target)[live]))
    for g in range(50):
        members = pop.perturb_reference(theta, P, obs_dim, sigma, seed=5, generation=g)
        f = -((members[:, :nf] - target)[:, live].astype(np.float64) ** 2).sum(axis=1)
        ranks = np.empty(P, dtype=np.float32)
        ranks[np.argsort(f)] = np.arange(P, dtype=np.float32)
        w = (ranks / (P - 1) - 0.5).astype(np.float32)
        grad, theta = pop.es_update_reference(theta, w, obs_dim, sigma, lr, seed=5, generation=g)
        assert not grad[~live].any() and not theta[~live].any()
    d1 = float(np.linalg.norm((theta - target)[live]))
    print("distance to the target: %.4f -> %.4f" % (d0, d1))
    assert d1 < d0


def test_population_geometry_and_constructor_refusals():
    assert pop.population_geometry(4096, 256) == (256, 16)
    assert pop.population_geometry(4096, 64) == (64, 64)
    assert pop.population_geometry(96, 3, 32) == (3, 32)
    env = SimpleNamespace(n_envs=96, obs_dim=6)
    for members, rows in ((0, None), (-2, None), (5, None), (8, None), (3, 16), (3, 24), (2, 32), (3, 0)):
        with pytest.raises(ValueError):
            pop.PolicyPopulation(env, members, rows)           # (refused before anything touches a device)
    import gym_auv_amd
    assert gym_auv_amd.PolicyPopulation is pop.PolicyPopulation


def test_population_io_struct_matches_the_header(tmp_path):
    from gym_auv_amd import _capi
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu\\n", '
                   'sizeof(auv_population_io_t), offsetof(auv_population_io_t, stride), offsetof(auv_population_io_t, accumulate), '
                   'offsetof(auv_population_io_t, clip_hi));return 0;}\n' % os.path.join(ROOT, "include", "auv_hip.h"))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    size, o_stride, o_acc, o_hi = map(int, subprocess.check_output([str(exe)]).split())
    assert C.sizeof(_capi.AuvPopulationIO) == size
    assert (_capi.AuvPopulationIO.stride.offset, _capi.AuvPopulationIO.accumulate.offset, _capi.AuvPopulationIO.clip_hi.offset) == (o_stride, o_acc, o_hi)
