"""CPU: what the planner's device sampler and refit (csrc/k15_plan.hip; auv_plan_sample, auv_plan_refit) promise without a device --
the exports are declared and bound and the ABI version stays, the kernels compile for gfx950 without scratch memory, the NumPy
mirrors give hand-computed values, the planner's option checks, and the recorded MPPI bound is what its derivation gives."""
import json
import os
import re

import numpy as np
import pytest

from gym_auv_amd import _capi, planning
from gym_auv_amd.population import es_noise

from kernel_resources import HIPCC, describe, kernel_resources
import plan_device_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f = np.float32


def test_new_exports_are_declared_bound_and_the_abi_version_stays():
    text = open(os.path.join(ROOT, "include", "auv_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _capi.load_library()
    for name, nargs in (("auv_plan_sample", 16), ("auv_plan_refit", 18)):
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
        assert "%s(" % name in open(os.path.join(ROOT, "gym_auv_amd", "csrc", "auv_capi_aux.hip")).read()
    assert _capi.ABI_VERSION == 5 and lib.auv_abi_version() == 5 and "#define AUV_ABI_VERSION 5" in text
    for name, val in (("AUV_PLAN_CEM", _capi.AUV_PLAN_CEM), ("AUV_PLAN_MPPI", _capi.AUV_PLAN_MPPI), ("AUV_PLAN_MAX_GROUP", _capi.AUV_PLAN_MAX_GROUP)):
        assert "#define %s %d\n" % (name, val) in text
    assert planning.PLAN_METHODS == {"cem": _capi.AUV_PLAN_CEM, "mppi": _capi.AUV_PLAN_MPPI}
    assert planning.PLAN_MAX_CANDIDATES == _capi.AUV_PLAN_MAX_GROUP
    assert "k15_plan.hip" in open(os.path.join(ROOT, "gym_auv_amd", "csrc", "Makefile")).read()
    # a null handle is refused, not dereferenced
    assert lib.auv_plan_sample(None, None, None, None, None, None, 1, 1, 1, 0, None, None, 0, 0, None, None) == -1
    assert lib.auv_plan_refit(None, None, None, None, 1, 1, 1, 0, 1, 0.0, 1.0, None, None, None, None, None, None, None) == -1


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_plan_kernels_compile_for_gfx950_without_scratch_or_spills():
    kernels = {n: [k for k in kernel_resources("k15_plan.hip") if n in k["name"]] for n in ("k15_plan_sample", "k15_plan_refit")}
    for name, ks in kernels.items():
        assert len(ks) == 1, name
        print(describe(ks[0]))
        assert ks[0]["private"] == 0 and ks[0]["vgpr_spill"] == 0 and ks[0]["sgpr_spill"] == 0, describe(ks[0])
    assert kernels["k15_plan_sample"][0]["static_lds"] == 0
    assert kernels["k15_plan_refit"][0]["static_lds"] <= 9 * 1024 + 64          # scores, elite list, elite flags of 1024 candidates


def test_one_definition_of_the_candidate_order_and_of_the_noise():
    csrc = os.path.join(ROOT, "gym_auv_amd", "csrc")
    for fn in os.listdir(csrc):
        if fn.endswith((".hip", ".h", ".inc")):
            txt = open(os.path.join(csrc, fn)).read()
            assert ("bool plan_beats(" in txt) == (fn == "auv_plan.h"), fn
            assert ("float pop_eps(" in txt) == (fn == "auv_noise.h"), fn
            assert ("long long pop_key(" in txt) == (fn == "auv_noise.h"), fn
    for fn in ("k7_snapshot.hip", "k15_plan.hip"):
        assert '#include "auv_plan.h"' in open(os.path.join(csrc, fn)).read()
    for fn in ("auv_population_pass.h", "k15_plan.hip"):
        assert '#include "auv_noise.h"' in open(os.path.join(csrc, fn)).read()


def test_sampler_mirror_gives_the_hand_computed_values():
    """K = 3, T = 2, one group: candidate 0 is the clipped mean, the others mean + sigma * eps with eps at (pair = k, idx = 2 t + j),
    clipped; a shift of 1 repeats the last row; a masked group reads mean0 / sigma0 unshifted."""
    lo, hi = np.array(cases.LO, dtype=f), np.array(cases.HI, dtype=f)
    mean = np.array([[[0.5, 0.2]], [[-2.0, 0.1]]], dtype=f)                  # [T = 2, B = 1, 2]: 0.2 > hi[1], -2 < lo[0]
    sigma = np.array([[[0.25, 0.05]], [[0.5, 0.0]]], dtype=f)
    seed, draw = 7, 3
    ring = planning.reference_plan_sample(mean, sigma, 3, lo, hi, seed, draw)
    assert ring.shape == (2, 3, 2) and ring.dtype == f
    np.testing.assert_array_equal(ring[:, 0, :], np.array([[0.5, 0.15], [-1.0, 0.1]], dtype=f))
    for t in range(2):
        for k in (1, 2):
            for j in range(2):
                eps = es_noise(seed, draw, k, 2 * t + j)[0]
                want = f(mean[t, 0, j] + f(sigma[t, 0, j] * eps))
                want = min(max(want, lo[j]), hi[j])
                assert ring[t, k, j] == want, (t, k, j)
    assert ring[1, 1, 1] == f(0.1) and ring[1, 2, 1] == f(0.1)              # sigma = 0: the mean itself
    assert not np.array_equal(ring, planning.reference_plan_sample(mean, sigma, 3, lo, hi, seed, draw + 1))
    # shift = 1: both rows read row 1, the noise still that of (t, j)
    sh = planning.reference_plan_sample(mean, sigma, 3, lo, hi, seed, draw, shift=1)
    np.testing.assert_array_equal(sh[1], ring[1])
    np.testing.assert_array_equal(sh[0, 0], np.array([-1.0, 0.1], dtype=f))
    assert sh[0, 1, 0] == min(max(f(f(-2.0) + f(f(0.5) * es_noise(seed, draw, 1, 0)[0])), lo[0]), hi[0])
    # two groups, the second masked: it reads mean0 / sigma0 at row t, the first is shifted
    mean2, sigma2 = np.concatenate([mean, mean], axis=1), np.concatenate([sigma, sigma], axis=1)
    mean0 = np.array([[[0.0, 0.0]] * 2, [[0.25, -0.05]] * 2], dtype=f)
    sigma0 = np.full((2, 2, 2), 0.125, dtype=f)
    two = planning.reference_plan_sample(mean2, sigma2, 3, lo, hi, seed, draw, shift=1, reset=np.array([0, 1], np.uint8), mean0=mean0, sigma0=sigma0)
    np.testing.assert_array_equal(two[:, :3], sh)
    np.testing.assert_array_equal(two[:, 3], mean0[:, 1])
    assert two[1, 5, 0] == f(f(0.25) + f(f(0.125) * es_noise(seed, draw, 5, 2)[0]))     # pair = e = 1 * 3 + 2, idx = 2 * 1 + 0


def test_refit_mirror_gives_the_hand_computed_values():
    """K = 3, T = 2: the elite of (1, NaN, 1) with E = 2 is {0, 2}; with E = 1 the lower index of the tie; all NaN: candidates 0 .. E - 1."""
    nan = float("nan")
    ring = np.zeros((2, 3, 2), dtype=f)
    ring[0] = [[0.5, 0.1], [9.0, 9.0], [-0.25, 0.05]]
    ring[1] = [[0.1, 0.15], [9.0, 9.0], [0.1, -0.15]]
    mean, sigma, chosen, predicted = planning.reference_plan_refit(ring, [1.0, nan, 1.0], [2], 3, "cem", n_elite=2, sigma_min=1e-3)
    assert mean.dtype == f and sigma.dtype == f and mean.shape == (2, 1, 2)
    np.testing.assert_array_equal(mean[:, 0], np.array([[0.125, f(f(f(0.1) + f(0.05)) / f(2))], [f(f(f(0.1) + f(0.1)) / f(2)), 0.0]], dtype=f))
    assert sigma[0, 0, 0] == f(0.375)                                        # ((0.375)^2 + (-0.375)^2) / 2 = 0.375^2, exact
    d0, d1 = f(f(0.15) - f(0.0)), f(f(-0.15) - f(0.0))
    assert sigma[1, 0, 1] == np.sqrt(f(f(f(d0 * d0) + f(d1 * d1)) / f(2)))
    assert sigma[1, 0, 0] == f(1e-3)                                         # identical elite: sigma_min
    np.testing.assert_array_equal(chosen[:, 0], ring[:, 2])
    assert predicted.tolist() == [1.0]
    m1 = planning.reference_plan_refit(ring, [1.0, nan, 1.0], [0], 3, "cem", n_elite=1, sigma_min=0.5)
    np.testing.assert_array_equal(m1[0][:, 0], ring[:, 0])
    assert (m1[1] == f(0.5)).all()
    m_nan = planning.reference_plan_refit(ring, [nan, nan, nan], [0], 3, "cem", n_elite=2)[0]
    np.testing.assert_array_equal(m_nan[0, 0], np.array([f(f(f(0.5) + f(9.0)) / f(2)), f(f(f(0.1) + f(9.0)) / f(2))], dtype=f))
    m_inf = planning.reference_plan_refit(ring, [-np.inf, nan, np.inf], [0], 3, "cem", n_elite=2)[0]      # -inf is valid and beats the NaN
    np.testing.assert_array_equal(m_inf, mean)
    assert planning._rank_order(np.array([0.0, nan, 2.0, -0.0, 2.0, nan, -np.inf], dtype=f)).tolist() == [2, 4, 0, 3, 6, 1, 5]
    # ---- MPPI, float64 ----
    mean_in, sigma_in = np.full((2, 1, 2), 0.01, dtype=f), np.full((2, 1, 2), 0.3, dtype=f)
    m, s, _, _ = planning.reference_plan_refit(ring, [0.0, nan, -1.0], [0], 3, "mppi", lam=1.0, mean_in=mean_in, sigma_in=sigma_in)
    assert m.dtype == np.float64
    w = np.exp(-1.0)
    np.testing.assert_allclose(m[:, 0], (ring[:, 0].astype(np.float64) + w * ring[:, 2]) / (1.0 + w), rtol=0, atol=1e-15)
    np.testing.assert_array_equal(s, sigma_in)
    m = planning.reference_plan_refit(ring, [nan, nan, nan], [0], 3, "mppi", lam=1.0, mean_in=mean_in, sigma_in=sigma_in)[0]
    np.testing.assert_array_equal(m, mean_in.astype(np.float64))
    # lambda so small that every other weight underflows: the mean of the tied maxima; -inf scores weigh 0, all -inf: all 1
    m = planning.reference_plan_refit(ring, [2.0, 1.0, 2.0], [0], 3, "mppi", lam=1e-30, mean_in=mean_in, sigma_in=sigma_in, mppi_dtype=f)[0]
    np.testing.assert_array_equal(m, mean)
    assert planning.mppi_weights([-np.inf, 0.0, nan], 1.0).tolist() == [0.0, 1.0, 0.0]
    assert planning.mppi_weights([-np.inf, -np.inf, nan], 1.0).tolist() == [1.0, 1.0, 0.0]
    assert planning.mppi_weights([np.inf, 5.0, np.inf], 1.0).tolist() == [1.0, 0.0, 1.0]
    assert planning.mppi_weights([nan, nan], 1.0) is None
    with pytest.raises(ValueError):
        planning.reference_plan_refit(ring, [1.0, 1.0, 1.0], [0], 3, "cem", n_elite=4)
    with pytest.raises(ValueError):
        planning.reference_plan_refit(ring, [1.0, 1.0, 1.0], [0], 2, "cem", n_elite=1)


def test_composed_mirror_runs_the_iterations_in_order():
    """Two records: three rings (draws d, d + 1, d + 2), each sampled around the refit of the one before."""
    lo, hi = np.array(cases.LO, dtype=f), np.array(cases.HI, dtype=f)
    T, B, K = 2, 2, 4
    mean0, sigma0 = np.zeros((T, B, 2), dtype=f), np.full((T, B, 2), 0.1, dtype=f)
    rs = np.random.RandomState(0)
    records = [(rs.normal(size=(T, B * K)).astype(f), np.zeros((T, B * K), np.uint8)) for _ in range(2)]
    rings, mean, sigma = planning.reference_plan_iterations(mean0, sigma0, K, lo, hi, 5, 10, records, 0.9, "cem", 2, 1e-3)
    assert len(rings) == 3
    np.testing.assert_array_equal(rings[0], planning.reference_plan_sample(mean0, sigma0, K, lo, hi, 5, 10))
    sc, be = planning.reference_plan_score(*records[0], K, 0.9)
    m1, s1, _, _ = planning.reference_plan_refit(rings[0], sc, be, K, "cem", 2, 1e-3)
    np.testing.assert_array_equal(rings[1], planning.reference_plan_sample(m1, s1, K, lo, hi, 5, 11))
    sc, be = planning.reference_plan_score(*records[1], K, 0.9)
    m2, s2, _, _ = planning.reference_plan_refit(rings[1], sc, be, K, "cem", 2, 1e-3)
    np.testing.assert_array_equal(mean, m2)
    np.testing.assert_array_equal(rings[2], planning.reference_plan_sample(m2, s2, K, lo, hi, 5, 12))


def test_planner_option_checks_need_no_device():
    planning.check_planner_options(64)
    planning.check_planner_options(1024, "device", "mppi", 0.5, True)
    planning.check_planner_options(4096, "torch")                           # the torch sampler has no such limit
    for args, what in (((64, "torch", "mppi"), "need sampler"), ((64, "torch", "cem", 1.0, True), "need sampler"),
                       ((1025, "device"), "at most 1024"), ((64, "hip"), "sampler must be"), ((64, "device", "pi2"), "method must be"),
                       ((64, "device", "mppi", 0.0), "mppi_lambda"), ((64, "device", "mppi", float("inf")), "mppi_lambda"),
                       ((64, "device", "mppi", float("nan")), "mppi_lambda")):
        with pytest.raises(ValueError, match=what):
            planning.check_planner_options(*args)
    # the constructor runs them before it looks at the environment
    with pytest.raises(ValueError, match="need sampler"):
        planning.ShootingPlanner(None, method="mppi")
    with pytest.raises(ValueError, match="at most 1024"):
        planning.ShootingPlanner(None, candidates=1025, sampler="device")


def test_recorded_mppi_bound_is_what_the_restatements_give():
    """tests/golden/plan_refit_bounds.json: per (K, lambda) of the GPU test and per action component, 8 x the distance of the plain
    float32 restatement from the float64 one on the GPU test's own inputs (seeded), at least 4 float32 eps x (hi - lo)."""
    rec = json.load(open(cases.BOUNDS_PATH))
    now = cases.computed_bounds()
    assert rec["seed"] == now["seed"] == cases.MPPI_SEED
    assert [(c["K"], c["lambda"]) for c in rec["cases"]] == cases.MPPI_CASES
    floor = 4.0 * float(np.finfo(f).eps) * (np.array(cases.HI) - np.array(cases.LO))
    for c, d in zip(rec["cases"], now["cases"]):
        print(c["K"], c["lambda"], c["bound"], d["bound"])
        np.testing.assert_allclose(c["bound"], d["bound"], rtol=1e-6, atol=0)
        assert (np.array(c["bound"]) >= floor).all() and (np.array(c["bound"]) < 1e-5).all()
        np.testing.assert_array_equal(cases.recorded_bound(c["K"], c["lambda"]), np.array(c["bound"]))
