"""CPU: the crafted rows of tests/devgen_rows.py really visit what they were crafted for (so that the GPU comparison of
tests/test_gpu_devgen_edges.py cannot silently miss a branch of k5_generate.hip), and the host mirror the device is compared
with -- path.Path -- agrees with SciPy's PchipInterpolator, the reference's own interpolant, on those degenerate curves."""
import warnings

import numpy as np
import pytest

import devgen_rows as R
from gym_auv_amd import devgen
from gym_auv_amd.obstacles import SIMPLIFY_TOLERANCE, circle_ring, douglas_peucker_keep
from gym_auv_amd.path import N_RESAMPLE, Path
from gym_auv_amd.world import build_world

NM, NS = 3, 16
GOLDEN_ATOL = 1e-11          # tests/test_path.py: the tolerance of the comparison with the reference's golden paths


@pytest.fixture(scope="module")
def built():
    """{case: (row, BuiltWorld)} of every crafted row; building must not warn"""
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for name, row in R.all_rows(NM, NS):
            out[name] = (row, build_world(devgen.world_from_draws(row, NM, NS)))
    return out


def _names(fam):
    return [n for n, _ in R.family(fam, NM, NS)]


# ---- the slope rule's predicates, restated: which branch a knot takes ---------------------------------------------------------
def _chords(wp):
    return np.concatenate([[0.0], np.cumsum(np.hypot(*np.diff(wp, axis=1)))])


def _interior_branch(mm, mp):
    if mm == 0.0 and mp == 0.0:
        return "zero,zero"
    if mm == 0.0:
        return "zero,nonzero"
    if mp == 0.0:
        return "nonzero,zero"
    return "sign" if (mm > 0) != (mp > 0) else "mean"


def _edge_exit(h0, h1, m0, m1):
    d = ((2.0 * h0 + h1) * m0 - h0 * m1) / (h0 + h1)
    if np.sign(d) != np.sign(m0):
        return "zero:m0=0" if m0 == 0.0 else "zero"
    if np.sign(m0) != np.sign(m1) and abs(d) > 3.0 * abs(m0):
        return "clamp"
    return "plain:d=0" if d == 0.0 else "plain"


def _branches(wp):
    s, y = _chords(wp), wp[1]
    h = np.diff(s)
    m = np.diff(y) / h
    inner = [_interior_branch(m[i - 1], m[i]) for i in range(1, len(s) - 1)]
    return inner, _edge_exit(h[0], h[1], m[0], m[1]), _edge_exit(h[-1], h[-2], m[-1], m[-2])


def test_slopes_rows_take_every_branch(built):
    inner, first, last = set(), set(), set()
    for n in _names("slopes"):
        row, hw = built[n]
        assert row[1] == 0.5 and np.all(hw.spec.waypoints[1, [0, -1]] == 0.0)        # sin(theta0) is exactly 0
        i, f, l = _branches(hw.spec.waypoints)
        inner |= set(i)
        first.add(f)
        last.add(l)
    assert inner == {"zero,zero", "zero,nonzero", "nonzero,zero", "sign", "mean"}
    # both special exits of the end rule (0: with a zero and with a non-zero first secant; the 3 * m0 clamp) and the plain one
    for seen in (first, last):
        assert seen >= {"zero", "zero:m0=0", "clamp", "plain", "plain:d=0"}


def test_collinear_rows_have_signed_zero_secants(built):
    """y == 0 everywhere; the end point is -start, so its y is -0.0 and the last secant of y is -0.0 next to +0.0 ones: a slope
    rule without its zero-secant test would divide by them into inf - inf."""
    for n in _names("collinear"):
        wp = built[n][1].spec.waypoints
        assert np.all(wp[1] == 0.0)
        m = np.diff(wp[1]) / np.diff(_chords(wp))
        assert np.all(m == 0.0) and np.signbit(m[-1]) and not np.signbit(m[-2])
        assert np.all(built[n][1].path.points[:, 1] == 0.0) and np.all(built[n][1].path.cy == 0.0)


def test_count_rows_give_5_7_and_9_points(built):
    """5 and 7 raw waypoints on either side of row[0] = 1/2 -- and 9 for the largest double below 1, where 4 * row[0] + 2 rounds
    to 6: the reference's RandomCurveThroughOrigin builds that curve, so the host mirror and the device must too."""
    n_pts = [built[n][1].spec.waypoints.shape[1] for n in _names("count")]
    # the count as the generator computes it, rounding of 4 * row[0] + 2 included (0.5 - 2^-54 already gives 7 points)
    for n, k in zip(_names("count"), n_pts):
        assert k == 2 * (int(np.floor(4 * built[n][0][0] + 2)) // 2) + 3
    assert n_pts == [5, 5, 5, 7, 7, 7, 7, 9]
    assert all(0.0 <= built[n][0][0] < 1.0 for n in _names("count"))


def test_lengths_are_away_from_whole_decimetres(built):
    """P = int(10 L); the device sums L in another order (~1e-13 relative), so P is only well defined away from integers."""
    for n, (row, hw) in built.items():
        t = 10.0 * hw.path.length
        if n.startswith("collinear"):
            assert abs(t - 8000.0) < 1e-8
        else:
            assert abs(t - np.round(t)) >= 1e-6, (n, hw.path.length)
    assert len(built["slopes%d" % R.LONGEST_SLOPES][1].path.points) == max(len(hw.path.points) for _, hw in built.values())


def test_cut_rows_start_on_the_cut(built):
    """y == 0 along the first half of the path: the direction at s = 0 is atan2(+-0, -1) = +-pi, and the heading draws
    0, 1/2, 1 - 2^-53 put the start heading at 0 (through the wrap), at -pi exactly, and within an ulp of 2 pi of 0 (after
    a turn of 2 pi (1/2 - 2^-53) and the wrap)."""
    h = [built[n][1].scalar[5] for n in _names("cut")]
    p = built["cut1"][1].path
    assert abs(p.get_direction(0.0)) == np.pi
    assert h[1] == -np.pi
    assert h[0] == 0.0 and abs(h[2]) < 1e-15


def test_first_candidate_kept_except_in_pool_rows(built):
    for n, (row, hw) in built.items():
        k = int(n[4:]) if n.startswith("pool") else 0
        col = 11
        for j in range(NM):
            z, u, pois = R.candidate(j, k if j == 0 else 0, R.MOVER_POISSON[j % 3] if n.startswith("radii") else 10, R.SIGMA_MOVER)
            assert hw.mv_param[j, 0] == max(1.0, pois) and hw.mv_param[j, 0] < 100
            col += 3 * R.CAND + 2
        for i in range(NS):
            pois = R.CIRCLE_POISSON[i] if n.startswith("radii") else 30
            z, u, pois = R.candidate(i, k if i == 0 else 0, pois, R.SIGMA_CIRCLE)
            assert hw.obs_cull[i, 2] == max(1.0, pois)
        if k:
            assert hw.mv_param[0, 0] == 10 + k and hw.obs_cull[0, 2] == 30 + k
            # ... and the candidates behind k differ from it, so another index would show
            assert len({tuple(row[11 + 3 * c: 14 + 3 * c]) for c in range(k, R.CAND)}) == R.CAND - k


# ---- the host mirror against SciPy -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["slopes", "collinear", "count"])
def test_three_passes_against_scipy(built, fam):
    """Path's three re-parameterisations (knots, coefficient rows) and its dense polyline against the same construction on
    scipy.interpolate.PchipInterpolator (what the reference's Path is built from), at the tolerance of the golden comparison."""
    interp = pytest.importorskip("scipy.interpolate")
    for n in _names(fam):
        p = built[n][1].path
        wp = p.init_waypoints
        for k in range(3):
            s = _chords(wp)
            fx, fy = interp.PchipInterpolator(s, wp[0]), interp.PchipInterpolator(s, wp[1])
            # the host's own pass k, rebuilt from the same points
            q = np.linspace(s[0], s[-1], N_RESAMPLE)
            wp = np.vstack([fx(q), fy(q)])
        np.testing.assert_allclose(p.knot_s, s, rtol=0, atol=GOLDEN_ATOL, err_msg=n)
        np.testing.assert_allclose(p.cx, fx.c, rtol=0, atol=GOLDEN_ATOL, err_msg=n)
        np.testing.assert_allclose(p.cy, fy.c, rtol=0, atol=GOLDEN_ATOL, err_msg=n)
        np.testing.assert_allclose(p._waypoints, wp, rtol=0, atol=GOLDEN_ATOL, err_msg=n)
        S = np.linspace(0, s[-1], int(10 * s[-1]))
        assert len(p.points) == len(S), n
        np.testing.assert_allclose(p.points, np.stack([fx(S), fy(S)], axis=1), rtol=0, atol=GOLDEN_ATOL, err_msg=n)
        assert np.all(np.isfinite(p.cx)) and np.all(np.isfinite(p.cy))


def test_first_pass_slopes_against_scipy(built):
    """the raw waypoints are where the crafted branches are: the first pass's coefficient rows on their own"""
    interp = pytest.importorskip("scipy.interpolate")
    from gym_auv_amd.path import hermite_coefs, pchip_slopes
    for fam in ("slopes", "collinear", "count", "cut"):
        for n in _names(fam):
            wp = built[n][1].spec.waypoints
            s = _chords(wp)
            for a in range(2):
                ref = interp.PchipInterpolator(s, wp[a])
                np.testing.assert_allclose(hermite_coefs(s, wp[a], pchip_slopes(s, wp[a])), ref.c, rtol=0, atol=GOLDEN_ATOL, err_msg=n)


# ---- rings ---------------------------------------------------------------------------------------------------------------
def test_radii_rows_have_the_table_segment_counts(built):
    _, nseg = devgen.ring_tables()
    assert [int(nseg[r]) for r in (1, 2, 3, 4, 15, 16, 62, 63, devgen.R_TABLE - 1)] == [4, 8, 8, 16, 16, 32, 32, 64, 64]
    for n in _names("radii"):
        hw = built[n][1]
        radii = hw.obs_cull[:NS, 2]
        np.testing.assert_array_equal(radii, np.maximum(1, R.CIRCLE_POISSON))
        # the device's lookup: index int(radius), clamped to the table's last entry
        want = [int(nseg[min(int(r), devgen.R_TABLE - 1)]) for r in radii]
        np.testing.assert_array_equal(hw.obs_meta[:NS, 2], want)
        assert sorted(set(want)) == [4, 8, 16, 32, 64]


def test_radii_beyond_the_table_keep_the_full_ring():
    """Finding, recorded: for every radius >= 63 Douglas-Peucker at the 0.1 m tolerance keeps all 64 segments of the buffer
    ring (the sagitta of a 64-gon's edge over two is r (1 - cos(pi / 32)) = 0.0048 r >= 0.3 m), so the table's last entry is
    what the host builds for any radius past it: the clamp in k5_generate is exact, not an approximation."""
    _, nseg = devgen.ring_tables()
    last = int(nseg[devgen.R_TABLE - 1])
    assert last == 64
    for r in (devgen.R_TABLE - 1, devgen.R_TABLE, devgen.R_TABLE + 1, 300, 1000, 6000):
        assert len(douglas_peucker_keep(circle_ring(0.0, 0.0, float(r)), SIMPLIFY_TOLERANCE)) - 1 == last, r
