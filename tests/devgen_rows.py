"""Crafted rows of draws for the on-device world generator (k5_generate.hip) and its host mirror
(devgen.world_from_draws): the places random draws never visit -- exact-zero and sign-changing secants, both
special exits of the PCHIP end-slope rule, the boundaries of the waypoint count, headings on the +-pi cut, the edges
of the ring table, a pool whose k-th candidate is the first accepted one, a path of a whole number of decimetres.

Row layout (devgen.n_draws / world_from_draws): row[0] waypoint count, row[1] theta0, row[2..7] jitters
(row[2 + 2k] moves raw waypoint 1 + k, row[3 + 2k] waypoint n - 2 - k; a jitter moves x and y alike), row[8..10]
the pose, then 3 * CAND + 2 columns per mover and 3 * CAND per circle.  Unless a family says otherwise the first
candidate of every obstacle sits well clear of start and goal (u = 0.5, |z| = (radius + 100) / sigma) and is the
one kept; candidate c >= 1 differs from every other in place and radius.

The jitters of SLOPES are the winners of a grid search over {0.5, 0.5 +- 2^-7, 0.1, 0.9} for rows whose y series
(row[1] = 0.5: sin(theta0) is exactly 0, so y is the jitters alone) takes, in the first of the three passes, every
branch of the interior slope rule and every exit of the end rule at both ends; tests/test_devgen_edges.py
re-derives the branches from the waypoints and fails if one is no longer visited.

Also here: the table comparison shared by tests/test_gpu_devgen.py and tests/test_gpu_devgen_edges.py."""
import numpy as np

from gym_auv_amd import devgen

CAND = devgen.CAND
E = 2.0 ** -7
SIGMA_MOVER, SIGMA_CIRCLE = 500.0, 250.0
REJECTED_RADIUS = 6000.0                  # larger than any world: such a candidate always covers the vessel

COUNT_VALUES = (0.0, 0.25 - 2.0 ** -54, 0.25, 0.5 - 2.0 ** -54, 0.5, 0.75 - 2.0 ** -54, 0.75, 1.0 - 2.0 ** -53)
ORDINARY_JITTERS = (0.31, 0.77, 0.62, 0.18, 0.44, 0.85)
ORDINARY_THETA = 0.137
ORDINARY_POSE = (0.3, 0.8, 0.65)

# (row[0], row[2..7]) -> branches of the y series in pass 1 (interior knots in order | first end, last end):
SLOPES = (
    (0.5, (0.5, 0.5, 0.5, 0.5 + E, 0.5, 0.5)),           # zero,zero  zero,zero  zero,+  sign  -,zero | d = 0, m0 = 0
    (0.0, (0.5 + E, 0.5 - E, 0.5, 0.5, 0.5, 0.5)),       # sign  mean  sign                      | plain, plain
    (0.0, (0.1, 0.5, 0.5, 0.5, 0.5, 0.5)),               # sign  -,zero  zero,zero               | 3 * m0 clamp, d = 0
    (0.5, (0.5, 0.5 + E, 0.5 + E, 0.1, 0.5, 0.5)),       # zero,+  sign  mean  sign  sign        | m0 = 0, 3 * m0 clamp
    (0.5, (0.5 + E, 0.5 + E, 0.9, 0.9, 0.5, 0.5)),       # mean  sign  sign  sign  mean          | sign(d) != sign(m0) at both
    (0.5, (0.1, 0.9, 0.9, 0.1, 0.5, 0.5)),               # the longest curve of the grid (L = 1509.3, P = 15093)
)
LONGEST_SLOPES = 5

CIRCLE_POISSON = (0, 1, 2, 3, 4, 5, 15, 16, 17, 62, 63, 64, 254, 255, 256, 300)
MOVER_POISSON = (0, 1, 2)

FAMILIES = ("count", "slopes", "collinear", "cut", "radii", "pool_k")


def candidate(index, c, pois, sigma):
    """(z, u, poisson) of candidate c of obstacle `index`: c = 0 at mid-path, radius + 100 m to one side; the others
    further along and further out, on the other side, each with a radius of its own."""
    side = 1.0 if index % 2 == 0 else -1.0
    if c == 0:
        return side * (max(1.0, pois) + 100.0) / sigma, 0.5, float(pois)
    p = float(pois + c)
    return -side * (max(1.0, p) + 100.0 + 20.0 * c) / sigma, 0.3 + 0.05 * c, p


def make_row(n_moving, n_static, count, theta, jitters, pose=(0.5, 0.5, 0.5), mover_pois=(10,), circle_pois=(30,),
             spread_circles=False, reject_first=0):
    """One row of draws.  `reject_first` = k: candidates 0 .. k - 1 of mover 0 and of circle 0 carry REJECTED_RADIUS, so
    candidate k is the first accepted.  `spread_circles`: circle c's first candidate at u = c / n_static, not at 0.5
    (the small rings near the start, where the LiDAR of a rollout reaches them)."""
    row = np.zeros(devgen.n_draws(n_moving, n_static), dtype=np.float64)
    row[0], row[1] = count, theta
    row[2:8] = jitters
    row[8:11] = pose
    col = 11
    for j in range(n_moving):
        for c in range(CAND):
            row[col + 3 * c: col + 3 * c + 3] = candidate(j, c, mover_pois[j % len(mover_pois)], SIGMA_MOVER)
            if j == 0 and c < reject_first:
                row[col + 3 * c + 2] = REJECTED_RADIUS
        row[col + 3 * CAND] = (0.13 + 0.29 * j) % 1.0          # direction
        row[col + 3 * CAND + 1] = (0.71 + 0.37 * j) % 1.0      # speed
        col += 3 * CAND + 2
    for i in range(n_static):
        for c in range(CAND):
            row[col + 3 * c: col + 3 * c + 3] = candidate(i, c, circle_pois[i % len(circle_pois)], SIGMA_CIRCLE)
            if i == 0 and c < reject_first:
                row[col + 3 * c + 2] = REJECTED_RADIUS
        if spread_circles:
            row[col + 1] = i / float(n_static)
        col += 3 * CAND
    assert col == len(row)
    return row


def family(name, n_moving, n_static):
    """[(case name, row)] of one family for worlds of n_moving movers and n_static circles."""
    mk = lambda *a, **kw: make_row(n_moving, n_static, *a, **kw)
    if name == "count":
        return [("count%d" % i, mk(v, ORDINARY_THETA, ORDINARY_JITTERS, ORDINARY_POSE)) for i, v in enumerate(COUNT_VALUES)]
    if name == "slopes":
        return [("slopes%d" % i, mk(c, 0.5, j)) for i, (c, j) in enumerate(SLOPES)]
    if name == "collinear":
        return [("collinear%d" % n, mk(c, 0.5, (0.5,) * 6)) for n, c in ((5, 0.0), (7, 0.5))]
    if name == "cut":
        # y = 0 up to the middle of the path, so the start heading is atan2(+-0, -1); 10 L = 8000.39
        return [("cut%d" % i, mk(0.0, 0.5, (0.5, 0.5 + E, 0.5, 0.5, 0.5, 0.5), (0.5, 0.5, h)))
                for i, h in enumerate((0.0, 0.5, 1.0 - 2.0 ** -53))]
    if name == "radii":
        return [("radii%d" % n, mk(c, ORDINARY_THETA, ORDINARY_JITTERS, ORDINARY_POSE, mover_pois=MOVER_POISSON,
                                   circle_pois=CIRCLE_POISSON, spread_circles=True)) for n, c in ((5, 0.0), (7, 0.5))]
    if name == "pool_k":
        return [("pool%d" % k, mk(0.5, ORDINARY_THETA, ORDINARY_JITTERS, ORDINARY_POSE, reject_first=k)) for k in range(1, CAND)]
    raise KeyError(name)


def all_rows(n_moving, n_static, families=FAMILIES):
    out = []
    for f in families:
        out += family(f, n_moving, n_static)
    return out


def princip(a):
    return ((np.asarray(a) + np.pi) % (2 * np.pi)) - np.pi


# ---- the device-built bank against the host builder -------------------------------------------------------------------------
BANK_TABLES = ("POLY_CNT", "POLY_XY", "POLY_CUM", "KNOT_S", "KNOT_COEF", "WORLD_SCALAR", "OBS_META", "OBS_CULL", "SEG",
               "MV_PARAM", "MV_INIT", "MV_VTAB", "CHUNK_BOUND")


def read_tables(env):
    return {k: env.read_bank(k).detach().cpu().numpy() for k in BANK_TABLES}


def assert_obstacle_tables(t, w, hw, nm, ns):
    """OBS_META / OBS_CULL / SEG / MV_* of world slot w against the host-built world hw (atol 1e-9; counts exact)."""
    meta, cull, seg = t["OBS_META"], t["OBS_CULL"], t["SEG"]
    K = nm + ns
    if K:
        hm = hw.obs_meta
        np.testing.assert_array_equal(meta[w, :K, 0], hm[:, 0])
        np.testing.assert_array_equal(meta[w, :K, 2], hm[:, 2])
        # movers: index within the world; circles: -3 = simple clockwise ring (back-face flag set on the device)
        np.testing.assert_array_equal(meta[w, :K, 3], np.where(hm[:, 0] == 0, -3, hm[:, 3]))
        np.testing.assert_allclose(cull[w, :K], hw.obs_cull, rtol=0, atol=1e-9)
        for k in range(ns):
            so = meta[w, k, 1] - w * seg.shape[1]          # absolute slot offset -> world-relative
            assert so == 64 * k
            np.testing.assert_allclose(seg[w, so:so + hm[k, 2]], hw.seg[hm[k, 1]:hm[k, 1] + hm[k, 2]], rtol=0, atol=1e-9)
    if nm:
        np.testing.assert_allclose(t["MV_PARAM"][w], hw.mv_param, rtol=0, atol=1e-9)
        np.testing.assert_allclose(t["MV_INIT"][w], hw.mv_init, rtol=0, atol=1e-9)
        np.testing.assert_allclose(t["MV_VTAB"][w], np.concatenate(hw.mv_vtab), rtol=0, atol=1e-9)


def assert_chunks_bound(t, w, points):
    """every chunk circle of slot w really bounds its vertices"""
    cb = t["CHUNK_BOUND"]
    P = len(points)
    for c in range((P - 1 + 63) // 64):
        v = points[c * 64:min(c * 64 + 64, P - 1) + 1]
        assert np.all(np.hypot(v[:, 0] - cb[w, c, 0], v[:, 1] - cb[w, c, 1]) <= cb[w, c, 2])


def assert_world_tables(t, w, hw, nm, ns, wrap_heading=False):
    """Every table of world slot w of the device-built bank `t` (read_tables) against the host-built world hw: P and the
    segment counts exactly, everything else at atol 1e-9 (coefficient rows: rtol 1e-6 as well).  `wrap_heading`: the start
    heading WORLD_SCALAR[5] is compared as an angle, |princip(device - host)| <= 1e-9 -- +pi and -pi are one heading."""
    p = hw.path
    P = len(p.points)
    assert t["POLY_CNT"][w] == P
    np.testing.assert_allclose(t["KNOT_S"][w], p.knot_s, rtol=0, atol=1e-9)
    np.testing.assert_allclose(t["KNOT_COEF"][w, :-1, 0:4], p.cx.T, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(t["KNOT_COEF"][w, :-1, 4:8], p.cy.T, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(t["POLY_XY"][w, :P], p.points, rtol=0, atol=1e-9)
    np.testing.assert_allclose(t["POLY_CUM"][w, :P], p._cum, rtol=0, atol=1e-9)
    sc = t["WORLD_SCALAR"][w]
    if wrap_heading:
        keep = np.arange(8) != 5
        np.testing.assert_allclose(sc[keep], hw.scalar[keep], rtol=0, atol=1e-9)
        assert abs(princip(sc[5] - hw.scalar[5])) <= 1e-9, (sc[5], hw.scalar[5])
    else:
        np.testing.assert_allclose(sc, hw.scalar, rtol=0, atol=1e-9)
    assert_chunks_bound(t, w, p.points)
    assert_obstacle_tables(t, w, hw, nm, ns)
