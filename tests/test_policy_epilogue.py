"""CPU: the NumPy mirrors of the act launch's sampling epilogue and of the advantage kernel (gym_auv_amd/policy.py: policy_noise,
logp_reference, action_map_reference, gae_reference; kernels: csrc/auv_policy_forward.h, k6_gae in csrc/k6_policy.hip), the bounds
tests/test_gpu_policy_epilogue.py holds the kernels to (tests/golden/policy_epilogue_bounds.json, derived in
tests/policy_epilogue_cases.py from the float32 restatement's distance to the float64 one, never from a kernel's output) -- and that
those bounds are not vacuous: nine one-line mistakes in the float32 restatement each leave them."""
import json
import os

import numpy as np
import pytest

from gym_auv_amd import policy as P
from gym_auv_amd.population import _mix

import policy_epilogue_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
M64 = (1 << 64) - 1


def _mix_int(z):
    z = (z + 0x9e3779b97f4a7c15) & M64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def test_the_hash_is_splitmix64_and_the_draw_is_keyed_as_the_kernel_keys_it():
    assert _mix_int(0) == 0xE220A8397B1DCDAF                    # splitmix64's first output from state 0
    zs = [0, 1, M64, 0x9e3779b97f4a7c15, 1 << 63, 0x0123456789abcdef] + [int(x) for x in np.random.RandomState(0).randint(0, 1 << 62, 50)]
    got = _mix(np.array(zs, dtype=np.uint64))
    assert [int(x) for x in got] == [_mix_int(z) for z in zs]
    # the whole key, in plain integers: mix(mix(seed ^ step * c) ^ (env << 1 | comp))
    for seed, step, env, comp in ((0, 0, 0, 0), (P.chain_seed(5, 1), 7, 39, 1), (M64, (1 << 40) + 3, (1 << 32) - 1, 1)):
        want = _mix_int(_mix_int(seed ^ ((step * 0xd1342543de82ef95) & M64)) ^ ((env << 1) | comp))
        assert int(P.policy_noise_hash(seed, step, env, comp)) == want, (seed, step, env, comp)
    # chain_seed is the expression the constructor has always used
    for seed, i in ((0, 0), (0, 3), (5, 1), (12345678901234567890, 2), (-1, 0)):
        assert P.chain_seed(seed, i) == (int(seed) * 0x9E3779B97F4A7C15 + i) & 0xFFFFFFFFFFFFFFFF


def test_the_fields_at_their_ends_stay_inside_the_unit_interval_and_the_draw_is_bounded():
    top = 0xFFFFFF
    # |eps| <= sqrt(-2 ln 2^-25), in the draw's own precision: the logarithm and the root each round once (half an ulp each, |cos| <= 1)
    rmax = {dt: np.sqrt(-2.0 * np.log(2.0 ** -25)) * (1.0 + 2.0 * float(np.finfo(dt).eps)) for dt in (f32, f64)}
    for a in (0, 1, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, top - 1, top):
        for b in (0, 1, 1 << 22, 1 << 23, top):
            h = np.uint64((a << 40) | (b << 8) | 0xA5)             # (the low byte is not part of the draw)
            u1, u2 = P.hash_fields(h)
            assert u1.dtype == f32 and u2.dtype == f32
            assert 0.0 < float(u1[0]) < 1.0, (a, float(u1[0]))
            assert 0.0 <= float(u2[0]) < 1.0 and float(u2[0]) == b / 16777216.0, b
            if a < (1 << 23):
                assert float(u1[0]) == (a + 0.5) / 16777216.0      # exact below 2^23
            else:
                assert abs(float(u1[0]) - (a + 0.5) / 16777216.0) <= 0.5 / 16777216.0   # a tie, rounded to even (the top one held below 1)
            for dt in (f32, f64):
                e = P.box_muller(u1, u2, dt)
                assert e.dtype == dt and np.isfinite(e).all() and abs(float(e[0])) <= rmax[dt], (a, b, dt)
    assert float(P.hash_fields(np.uint64(0))[0][0]) == 2.0 ** -25
    assert float(P.hash_fields(np.uint64(top << 40))[0][0]) == 1.0 - 2.0 ** -24
    # and over a million hashes
    u1, u2 = P.policy_noise_fields(3, np.arange(500)[:, None, None], np.arange(1000)[None, :, None], np.arange(2)[None, None, :])
    assert u1.shape == (500, 1000, 2) and float(u1.min()) > 0.0 and float(u1.max()) < 1.0 and float(u2.min()) >= 0.0 and float(u2.max()) < 1.0
    assert float(np.abs(P.box_muller(u1, u2, f32)).max()) <= rmax[f32]


def test_the_mirror_draws_a_standard_normal():
    e = P.policy_noise(P.chain_seed(0, 0), np.arange(200)[:, None, None], np.arange(1024)[None, :, None], np.arange(2)[None, None, :])
    assert e.dtype == f64 and e.shape == (200, 1024, 2)        # 409 600 draws
    print("mean %.5f var %.5f kurtosis %.4f" % (e.mean(), e.var(), (e ** 4).mean()))
    assert abs(e.mean()) < 0.01 and abs(e.var() - 1.0) < 0.02 and abs((e ** 4).mean() - 3.0) < 0.1
    assert abs((e[..., 0] * e[..., 1]).mean()) < 0.01          # the two components
    assert abs((e[1:] * e[:-1]).mean()) < 0.01                 # consecutive steps of one environment
    assert abs((e[:, 1:] * e[:, :-1]).mean()) < 0.01           # neighbouring environments
    assert np.unique(e).size > 0.95 * e.size
    # float32 is the same draw within the distance the bounds start from
    e32 = P.policy_noise(P.chain_seed(0, 0), np.arange(200)[:, None, None], np.arange(1024)[None, :, None], np.arange(2)[None, None, :], f32)
    assert e32.dtype == f32 and float(np.abs(e32 - e).max()) < 4e-6


def test_the_draw_changes_with_every_part_of_its_key():
    env, comp = np.arange(24)[:, None], np.arange(2)[None, :]
    base = P.policy_noise(P.chain_seed(5, 0), 3, env, comp)
    others = {"seed": P.policy_noise(P.chain_seed(6, 0), 3, env, comp), "chain": P.policy_noise(P.chain_seed(5, 1), 3, env, comp),
              "step": P.policy_noise(P.chain_seed(5, 0), 4, env, comp), "environment": P.policy_noise(P.chain_seed(5, 0), 3, env + 24, comp),
              "component": base[:, ::-1]}
    for name, other in others.items():
        assert other.shape == base.shape and (other != base).all(), name
    assert np.array_equal(base, P.policy_noise(P.chain_seed(5, 0), 3, env, comp))
    # scalars and arrays give the same draw
    assert float(P.policy_noise(P.chain_seed(5, 0), 3, 7, 1)) == base[7, 1]


def test_the_small_mirrors_by_hand():
    a = np.array([[0.75, -2.0], [-1.0, 0.125]], dtype=f32)
    got = P.action_map_reference(a, (0.25, -0.125), (0.5, 0.25), (-0.25, -0.5), (0.25, 0.5))
    assert got.dtype == f32 and got.tolist() == [[0.375, -0.25], [0.125, -0.09375]]
    # log pi: z = (1, -2) at sigma = (1, 1/2)... with log_std = 0 both: -0.5 (1 + 4) - 2 log sqrt(2 pi)
    lp = P.logp_reference(np.array([[1.5, -1.0]]), np.array([[0.5, 1.0]]), np.array([0.0, 0.0]))
    assert lp.shape == (1,) and abs(lp[0] - (-2.5 - np.log(2.0 * np.pi))) < 1e-15
    ls = np.array([0.5, -1.0])
    lp = P.logp_reference(np.array([0.5, 1.0]), np.array([0.5, 1.0]), ls)                    # at the mean: - sum ls - log 2 pi
    assert abs(float(lp) - (0.5 - np.log(2.0 * np.pi))) < 1e-15
    assert P.logp_reference(np.zeros((3, 2), f32), np.zeros((3, 2), f32), ls.astype(f32), f32).dtype == f32
    s = P.sample_reference(np.array([[1.0, 2.0]]), np.array([0.0, np.log(2.0)]), np.array([[0.5, -0.25]]))
    np.testing.assert_allclose(s, [[1.5, 1.5]], rtol=0, atol=1e-15)


def test_gae_reference_by_hand():
    """T = 3, N = 3, gamma = lam = 0.5 on dyadic numbers: environment 0 never done, 1 done at t = 0, 2 done at t = T - 1."""
    R = np.array([[1.0] * 3, [2.0] * 3, [4.0] * 3])
    V = np.array([[0.5] * 3, [1.0] * 3, [2.0] * 3])
    Dn = np.array([[0, 1, 0], [0, 0, 0], [0, 0, 1]], dtype=f64)
    last_v = np.array([8.0, 8.0, 8.0])
    for dt in (f64, f32):
        adv, ret = P.gae_reference(R, V, Dn, last_v, 0.5, 0.5, dt)
        assert adv.dtype == dt and ret.dtype == dt
        assert adv.tolist() == [[1.875, 0.5, 1.625], [3.5, 3.5, 2.5], [6.0, 6.0, 2.0]]
        assert ret.tolist() == [[2.375, 1.0, 2.125], [4.5, 4.5, 3.5], [8.0, 8.0, 4.0]]
    # gamma and lam are rounded to float32 before anything else
    a = P.gae_reference(R, V, Dn, last_v, 0.999, 0.98)[0]
    b = P.gae_reference(R, V, Dn, last_v, float(f32(0.999)), float(f32(0.98)))[0]
    assert np.array_equal(a, b) and not np.array_equal(a, P.gae_reference(R, V, Dn, last_v, 0.5, 0.5)[0])
    assert a[2, 0] == 4.0 + float(f32(0.999)) * 8.0 - 2.0


def test_recorded_bounds_are_what_the_restatements_give():
    rec = json.load(open(cases.BOUNDS_PATH))
    now = cases.computed_bounds()
    assert rec["seed"] == now["seed"] == cases.SEED and rec["cases_seed"] == cases.CASES_SEED and rec["rule"] == now["rule"] == cases.RULE
    # the search the GPU test relies on: chain 0's smallest u1 below 2^16 steps lies below 2^-20
    assert rec["searched_step"] == now["searched_step"] and rec["searched_u1"] == now["searched_u1"] < 2.0 ** -20
    eps32 = float(np.finfo(f32).eps)
    for what in ("eps", "A", "LP"):
        pairs = [(rec[what], now[what])] if what == "eps" else [(rec[what][k], now[what][k]) for k in now[what]]
        assert what == "eps" or list(rec[what]) == list(now[what]) == ["-0.5,-1.1", "0.5,0"]
        for r, n in pairs:
            print(what, r, n)
            np.testing.assert_allclose(r, n, rtol=1e-6, atol=0)
            assert 4.0 * eps32 <= r < 2e-5                         # a few float32 roundings of values of order one
    assert [(c["T"], c["N"], c["gamma"], c["lam"], c["dones"]) for c in rec["gae"]] == cases.gae_cases() and len(rec["gae"]) == 72
    for c, d in zip(rec["gae"], now["gae"]):
        np.testing.assert_allclose(c["bound"], d["bound"], rtol=1e-6, atol=0)
        assert c["bound"] == cases.recorded_gae_bound(c["T"], c["N"], c["gamma"], c["lam"], c["dones"])
        # float32 error grows with the number of accumulated steps, and no faster
        assert c["bound"] <= 8.0 * eps32 * c["T"] * 40.0, c
    print("gae bounds: %.3g .. %.3g" % (min(c["bound"] for c in rec["gae"]), max(c["bound"] for c in rec["gae"])))
    assert cases.recorded_bound("eps") == rec["eps"] and cases.recorded_bound("LP", (0.5, 0.0)) == rec["LP"]["0.5,0"]


# ------------------------------------------------------------------------------ the bounds are not vacuous
def _dist(mut32, ref64):
    return float(np.abs(np.asarray(mut32).astype(f64) - ref64).max())


@pytest.mark.parametrize("mutation", ["row_keyed", "step_reset", "swap", "one_comp"])
def test_a_wrong_keying_of_the_draw_leaves_the_bound(mutation):
    bound = cases.recorded_bound("eps")
    ref = cases.noise_inputs(f64)[0]
    good = cases.noise_inputs(f32)[0]
    assert _dist(good, ref) <= bound / 8.0 + 1e-12
    if mutation == "step_reset":
        # the generator's step restarts with t at begin_rollout: the second rollout repeats the first one's steps
        bad = np.stack([cases.launch_noise(cases.SEED, g % (cases.T + 1), f32) for g in cases.SAMPLE_STEPS])
        assert np.array_equal(bad[:cases.T], good[:cases.T])
    else:
        bad = cases.noise_inputs(f32, **{mutation: True})[0]
    d = _dist(bad, ref)
    print(mutation, d, bound)
    assert d > bound
    if mutation == "row_keyed":
        lo = cases.SLICES[1][0]                                    # the first slice's rows are their own environments
        assert np.array_equal(bad[:, :lo], good[:, :lo]) and _dist(bad[:, lo:], ref[:, lo:]) > bound
    if mutation == "one_comp":
        assert np.array_equal(bad[..., 0], good[..., 0]) and np.array_equal(bad[..., 0], bad[..., 1])


@pytest.mark.parametrize("mutation", ["no_ls", "constant"])
@pytest.mark.parametrize("log_std", cases.LOG_STDS)
def test_a_wrong_log_probability_leaves_the_bound(mutation, log_std):
    bound = cases.recorded_bound("LP", log_std)
    mu, eps, ls = cases.sample_inputs(log_std)
    a = P.sample_reference(mu, ls, eps, f32)
    ref = P.logp_reference(a, mu, ls, f64)
    assert _dist(P.logp_reference(a, mu, ls, f32), ref) <= bound / 8.0 + 1e-12
    z = (a - mu) / np.exp(ls.astype(f64)).astype(f32)
    if mutation == "no_ls":
        lp = f32(-0.5) * z * z - f32(0.9189385332046727)
    else:
        lp = f32(-0.5) * z * z - ls - f32(0.9199385332046727)      # log sqrt(2 pi) off in the fourth digit
    bad = lp[..., 0] + lp[..., 1]
    assert bad.dtype == f32
    d = _dist(bad, ref)
    print(mutation, log_std, d, bound)
    assert d > bound


def _gae32(R, V, Dn, last_v, gamma, lam, mutation):
    g, l = f32(gamma), f32(lam)
    Tn = R.shape[0]
    nv, gae, adv = last_v.copy(), np.zeros(R.shape[1], dtype=f32), np.empty_like(R)
    for t in range(Tn - 1, -1, -1):
        nd = f32(1.0) - Dn[t]
        nd_boot, nd_rec = nd, nd
        if mutation == "next_done":                                 # the mask of step t + 1 (none behind the last step)
            nd_boot = nd_rec = (f32(1.0) - Dn[t + 1]) if t + 1 < Tn else np.ones_like(nd)
        if mutation == "last_v_unmasked" and t == Tn - 1:
            nd_boot = np.ones_like(nd)
        delta = R[t] + g * nv * nd_boot - V[t]
        gae = (l * delta if mutation == "lam_on_delta" else delta) + g * l * nd_rec * gae
        adv[t] = gae
        nv = V[t]
    return adv


@pytest.mark.parametrize("mutation", ["next_done", "last_v_unmasked", "lam_on_delta"])
def test_a_wrong_advantage_recursion_leaves_the_bound(mutation):
    gamma, lam = cases.GAE_PARAMS[0]
    for Tn, Nn in cases.GAE_SHAPES:
        if Nn < 3:
            continue                                                # (no environment 1 and 2: no forced dones)
        bound = cases.recorded_gae_bound(Tn, Nn, gamma, lam, "random")
        R, V, Dn, last_v = cases.gae_inputs(Tn, Nn, "random")
        assert Dn[Tn - 1, 1] == 1.0 and Dn[0, 2] == 1.0
        ref = P.gae_reference(R, V, Dn, last_v, gamma, lam, f64)[0]
        good = _gae32(R, V, Dn, last_v, gamma, lam, None)
        assert np.array_equal(good, P.gae_reference(R, V, Dn, last_v, gamma, lam, f32)[0]) and _dist(good, ref) <= bound / 8.0 + 1e-12
        bad = _gae32(R, V, Dn, last_v, gamma, lam, mutation)
        d = _dist(bad, ref)
        print(mutation, Tn, Nn, d, bound)
        assert d > bound, (Tn, Nn)
        if mutation == "last_v_unmasked":                           # seen in the last step's forced done, at the very least
            assert abs(float(bad[Tn - 1, 1]) - ref[Tn - 1, 1]) > bound
