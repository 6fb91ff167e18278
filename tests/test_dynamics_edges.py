"""The edge rows of tests/dynamics_edge_rows.py on the CPU: the oracle's one-step dynamics (plain float64, libm sin / cos at every
evaluation) against the 50-digit reference of that file, its largest error per row group, step size and state component as recorded
in tests/golden/k1_edge_bounds.json (what tests/test_gpu_dynamics_edges.py derives the kernel's bound from: 8 times the recorded
figure, at least 4 ulp), the coverage the rows are for -- counted on the reference alone -- and the two branches of the kernel's
stage_sincos against each other and against the true sine / cosine.

The six `_state_dot` evaluations of a step are numbered 1..6; the first is taken at the start heading itself (increment 0, always
the series branch), so the classes "all at or under 0.125", "all above" and "mixed" are formed over evaluations 2..6."""
import ctypes
import ctypes.util
import json

import numpy as np

import dynamics_edge_rows as R

ULP = R.EPS                           # "ulp" of a sine / cosine: that of the scale max(1, |value|) = 1, as in the bounds' floor
MIN_COUNT = 4


def test_the_set_is_a_few_hundred_rows_and_few_fall_under_a_special_rule():
    t, ex = R.table(), R.expectations()
    n_poisoned = sum(len(b["poisoned"]) for b in R.neighbour_batches())
    total = len(t["dt"]) + n_poisoned
    special = int(ex["near_pi"].sum()) + n_poisoned
    assert 200 <= total <= 500, total
    assert np.isfinite(t["state"]).all()
    assert int(ex["near_pi"].sum()) >= 4 and n_poisoned == 2 * len(R.NEIGHBOUR_SIZES) - 1
    assert special <= 0.10 * total, (special, total)
    for b in R.neighbour_batches():
        assert b["n"] - 1 in b["poisoned"]                          # the environment idle lane groups clamp to
        bad = ~np.isfinite(b["state"]).all(axis=1)
        assert np.array_equal(np.flatnonzero(bad), b["poisoned"])
    kinds = np.concatenate([b["state"][b["poisoned"]] for b in R.neighbour_batches()])
    assert np.isnan(kinds).any(axis=0).sum() >= 4 and np.isinf(kinds).any(axis=0).sum() >= 4       # in most of the six components


def test_oracle_error_is_what_the_bounds_file_records():
    """The oracle's error against the reference, per bounds entry and component: finite, far below the suite's standing 1e-9, and
    the recorded figures (numbers only) are these -- not stale, not padded."""
    now = R.group_max(R.errors(R.oracle_table()))
    with open(R.BOUNDS_FILE) as f:
        rec = json.load(f)
    assert set(rec) == set(now) == set(R.table()["bounds"].tolist())
    for g, row in rec.items():
        assert set(row) == set(R.COMPONENTS)
        for c, v in row.items():
            assert isinstance(v, float) and np.isfinite(v) and 0.0 <= v < 1e-9, (g, c, v)
            assert now[g][c] <= v * (1 + 1e-9) + 1e-30, (g, c, now[g][c], v)
            assert v <= 4.0 * max(now[g][c], R.EPS), (g, c, now[g][c], v)
    large = [g for g in rec if g.startswith("wrap_large/")]
    assert len(large) == len(R.DTS)                                  # |psi_0| >= 1e3 has entries of its own ...
    t = R.table()
    assert (np.abs(t["state"][t["group"] == "wrap_large", 2]) >= R.LARGE_HEADING).all()
    assert (np.abs(t["state"][t["group"] != "wrap_large", 2]) < R.LARGE_HEADING).all()
    tol = R.tolerances()
    assert all((v >= R.BOUND_FLOOR_ULPS * R.EPS).all() and (v < 1e-8).all() for v in tol.values())


def test_the_rows_reach_what_they_are_for():
    t, ex = R.table(), R.expectations()
    inc = np.abs(ex["incs"][:, 1:])
    under, above = (inc <= R.STAGE_LIMIT).all(axis=1), (inc > R.STAGE_LIMIT).all(axis=1)
    counts = {"a: all at or under 0.125": int(under.sum()), "b: all above": int(above.sum()), "c: mixed": int((~under & ~above).sum())}
    first = np.abs(ex["incs"][:, 1])
    counts["d: first increment within 2 ulp below or at the limit"] = int(((first <= 0.125) & (first >= 0.125 - 2 * 2.0 ** -56)).sum())
    counts["d: first increment within 2 ulp above the limit"] = int(((first > 0.125) & (first <= 0.125 + 2 * 2.0 ** -55)).sum())
    final = np.array([R.princip_branch(float(w)) for w in ex["raw"]])
    start = np.array([R.princip_branch(float(p)) for p in t["state"][:, 2]])
    names = ("no wrap", "one period down", "one period up", "fmod")
    for k, name in enumerate(names):
        counts["e: final wrap, " + name] = int((final == k).sum())
        counts["f: start heading, " + name] = int((start == k).sum())
    a = t["action"]
    ok = ~np.isnan(a).any(axis=1)                                   # (a NaN makes the whole action zero: no clip side taken)
    counts["g: thrust below 0"] = int((ok & (a[:, 0] < 0.0)).sum())
    counts["g: thrust above 1"] = int((ok & (a[:, 0] > 1.0)).sum())
    counts["g: rudder below -1"] = int((ok & (a[:, 1] < -1.0)).sum())
    counts["g: rudder above 1"] = int((ok & (a[:, 1] > 1.0)).sum())
    print(json.dumps(counts, indent=1))
    assert all(v >= MIN_COUNT for v in counts.values()), counts
    assert int((~ok).sum()) >= 3
    # a step that wraps twice (the new heading two periods away), exact limits of the clip, -0.0, float32's own values
    assert (np.abs(ex["raw"][t["group"] == "wrap"]) > 3 * R.PI).any()
    for v in (0.0, 1.0, np.nextafter(1.0, 2.0), np.nextafter(0.0, -1.0), np.inf, -np.inf):
        assert (a[:, 0] == v).any(), v
    for v in (1.0, -1.0, np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0), np.inf, -np.inf):
        assert (a[:, 1] == v).any(), v
    assert (np.signbit(a[:, 0]) & (a[:, 0] == 0.0)).any()
    with np.errstate(over="ignore"):
        widened = a.astype(np.float32).astype(np.float64)
    assert ((widened != a) & ~np.isnan(a)).any(axis=1).sum() >= MIN_COUNT      # rows whose float32 action is another number


# ------------------------------------------------------------------------------------------------ stage_sincos, both branches
_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3
_fma = np.frompyfunc(lambda a, b, c: _libm.fma(float(a), float(b), float(c)), 3, 1)


def fma(a, b, c):
    return _fma(a, b, c).astype(np.float64)


def princip64(a):
    """auv_princip in float64 (gym_auv_amd/csrc/auv_device.h:322-338; its short cuts are bit-identical to the fmod they replace)."""
    m = np.fmod(a + R.PI, R.TWO_PI)
    return np.where(m < 0.0, m + R.TWO_PI, m) - R.PI


def heading0(psi):
    """heading0 (k1_dynamics.hip:44-49), with libm's sin / cos where the device calls its sincos."""
    p = princip64(psi)
    return np.sin(p), np.cos(p)


def series_branch(h0s, h0c, dl):
    """A TRANSCRIPTION of the first branch of stage_sincos, gym_auv_amd/csrc/k1_dynamics.hip:54-64, operation for operation (fused
    multiply-adds where the kernel writes fma, single roundings elsewhere) -- the only place in the tests where the kernel's own
    formula is mirrored."""
    z = dl * dl
    ps = fma(z, 1.0 / 6227020800.0, -1.0 / 39916800.0)
    for k in (1.0 / 362880.0, -1.0 / 5040.0, 1.0 / 120.0, -1.0 / 6.0):
        ps = fma(z, ps, k)
    sd = fma(dl * z, ps, dl)
    pc = fma(z, -1.0 / 87178291200.0, 1.0 / 479001600.0)
    for k in (-1.0 / 3628800.0, 1.0 / 40320.0, -1.0 / 720.0, 1.0 / 24.0, -0.5):
        pc = fma(z, pc, k)
    cd = fma(z, pc, 1.0)
    return fma(h0s, cd, h0c * sd), fma(h0c, cd, -(h0s * sd))


def full_branch(psi):
    """The second branch, k1_dynamics.hip:66: sincos(auv_princip(psi)), libm standing in for the device's sincos."""
    p = princip64(psi)
    return np.sin(p), np.cos(p)


def _truth(psi):
    s = np.array([float(R._mp.sin(R._mp.mpf(float(p)))) for p in psi])
    c = np.array([float(R._mp.cos(R._mp.mpf(float(p)))) for p in psi])
    return s, c


def _both(psi0, psi):
    """(largest error of the series branch, of the full branch, largest difference between them) in ulp, over sine and cosine, for
    stage headings `psi` of steps that start at `psi0`; the truth is the sine / cosine of the float64 stage heading."""
    h0s, h0c = heading0(psi0)
    ts, tc = _truth(psi)
    s1, c1 = series_branch(h0s, h0c, psi - psi0)
    s2, c2 = full_branch(psi)
    e1 = max(np.abs(s1 - ts).max(), np.abs(c1 - tc).max()) / ULP
    e2 = max(np.abs(s2 - ts).max(), np.abs(c2 - tc).max()) / ULP
    return e1, e2, max(np.abs(s1 - s2).max(), np.abs(c1 - c2).max()) / ULP


def test_the_two_branches_of_stage_sincos_agree_to_rounding():
    """What the kernel's comment claims (k1_dynamics.hip:34-39: truncation < 1e-19, rounding ~2 ulp): on 10 000 increments spread
    over [-0.125, 0.125] from start headings 0, 0.7, -2.9 and 3.1, and on the rows placed at the limit, either branch is within 4
    ulp of the true sine / cosine of the float64 stage heading; at the limit -- those rows, and increments of +-0.125 and one unit
    in the last place inside from the four start headings -- the two are within 4 ulp of each other.  ulp: 2^-52, that of the scale
    max(1, |value|) = 1, the unit the bounds' floor is counted in.  Both branches inherit the rounding of `princip` itself
    ((a + pi) - pi in float64, up to 2^-51 in the argument), which the reference has as well: the truth here is taken without it, so
    the figures include it.  Away from the limit the two branches round `princip` at different arguments and differ by more (5.2 ulp
    measured over the sweep, printed below); only the agreement at the limit is the kernel's claim."""
    starts = (0.0, 0.7, -2.9, 3.1)
    sweep = [0.0, 0.0, 0.0]
    for psi0 in starts:
        psi = psi0 + np.linspace(-0.125, 0.125, 2500)
        keep = np.abs(psi - psi0) <= 0.125
        sweep = [max(a, b) for a, b in zip(sweep, _both(np.full(int(keep.sum()), psi0), psi[keep]))]
    inside = np.nextafter(0.125, 0.0)
    p0 = np.repeat(starts, 4)
    psi = p0 + np.tile([0.125, -0.125, inside, -inside], len(starts))
    keep = np.abs(psi - p0) <= 0.125
    assert keep.sum() >= 2 * MIN_COUNT
    edge = _both(p0[keep], psi[keep])
    t, ex = R.table(), R.expectations()
    first = np.abs(ex["incs"][:, 1])
    at = (first >= 0.125 - 2 * 2.0 ** -56) & (first <= 0.125 + 2 * 2.0 ** -55)
    assert at.sum() >= 2 * MIN_COUNT
    psi0 = t["state"][at, 2]
    rows = _both(psi0, psi0 + t["dt"][at] * t["state"][at, 5] / 4.0)   # the stage heading as every body forms it: y + h * s1 / 4.0
    print("ulp (series branch, full branch, between them): over the sweep %.2f, %.2f, %.2f; at +-0.125 %.2f, %.2f, %.2f; on the rows "
          "at the limit %.2f, %.2f, %.2f" % (tuple(sweep) + edge + rows))
    assert max(sweep[0], edge[0], rows[0]) <= 4.0 and max(sweep[1], edge[1], rows[1]) <= 4.0
    assert max(edge[2], rows[2]) <= 4.0
