"""One-step cases for the vessel dynamics (K1) placed where the kernel's shortcuts switch, shared by tests/test_dynamics_edges.py
(CPU) and tests/test_gpu_dynamics_edges.py (GPU), and the high-precision reference both compare with.

A row is (state[6] = x, y, psi, u, v, r; action[2] = thrust, rudder; dt).  `groups()` returns the named groups, each with the
branch it aims at; `table()` the whole set as arrays; `neighbour_batches()` the batches of the group-packing tests.

`reference_step` is one Vessel.step in mpmath at 50 digits, written from the reference's formulas -- the constants and M, D,
N(nu) of utils/constants.py (M_inv is the inverse of M formed here, in mpmath), `_state_dot` (vessel.py:561-570), the `q`
combination of odesolver.py:2-47, `princip` of utils/geomutils.py:4-5 with the reference's pi (the float64 np.pi, taken exactly),
the clips of vessel.py:572-578 and the NaN-to-zero rule of environment.py:314-315.  It takes the float64 inputs exactly and knows
nothing of the kernel's constant division, its Taylor branch or the order of its sums.
"""
import functools
import json
import os

import mpmath
import numpy as np

PI = float(np.pi)
TWO_PI = 2.0 * PI
DTS = (0.5, 1.0, 8.0)
THRUST_MAX, MOMENT_MAX = 2.0, 0.15                 # Config().vessel.thrust_max_auv / moment_max_auv (reference config.py:39-40)
COMPONENTS = ("x", "y", "psi", "u", "v", "r")
STAGE_LIMIT = 0.125                                # |psi_stage - psi_0| at which stage_sincos changes branch
LARGE_HEADING = 1e3                                # groups with |psi_0| >= this have their own bounds entry
NEAR_PI = 1e-8                                     # a reference heading this close to +-pi is compared modulo 2 pi
BOUNDS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k1_edge_bounds.json")
BOUND_FACTOR = 8.0                                 # the GPU bound: this times the oracle's measured error ...
BOUND_FLOOR_ULPS = 4.0                             # ... and at least this many units in the last place of the scale
EPS = 2.0 ** -52
NEIGHBOUR_SIZES = (1, 7, 8, 9, 63, 64, 65)
NEIGHBOUR_DT = 0.5

_mp = mpmath.mp.clone()
_mp.dps = 50


# ------------------------------------------------------------------------------------------------ the reference
def _constants():
    f = _mp.mpf
    m, x_g, I_z = f(23.8), f(0.046), f(1.760)                  # the float64 values the reference holds, exactly
    X_udot, Y_vdot, Y_rdot, N_rdot, N_vdot = f(-2.0), f(-10.0), f(0.0), f(-1.0), f(0.0)
    X_u, Y_v, Y_r, N_v, N_r = f(-2.0), f(-7.0), f(-0.1), f(-0.1), f(-0.5)
    M = _mp.matrix([[m - X_udot, 0, 0], [0, m - Y_vdot, m * x_g - Y_rdot], [0, m * x_g - N_vdot, I_z - N_rdot]])
    D = _mp.matrix([[f(2.0), 0, 0], [0, f(7.0), f(-2.5425)], [0, f(-2.5425), f(1.422)]])
    return dict(m=m, x_g=x_g, X_u=X_u, Y_v=Y_v, Y_r=Y_r, N_v=N_v, N_r=N_r, M_inv=M ** -1, D=D)


_C = None


def _princip(a):
    """((a + pi) % (2 pi)) - pi with Python's sign convention and the reference's float64 pi, in exact arithmetic."""
    pi = _mp.mpf(PI)
    x = a + pi
    return x - 2 * pi * _mp.floor(x / (2 * pi)) - pi


def princip_branch(a):
    """Which of the four ranges of x = a + pi an exact evaluation of `princip` falls into:
    0: [0, 2 pi) no wrap   1: [2 pi, 4 pi) one period down   2: (-2 pi, 0) one period up   3: anything else (fmod)."""
    pi = _mp.mpf(PI)
    x = _mp.mpf(a) + pi
    if 0 <= x < 2 * pi:
        return 0
    if 2 * pi <= x < 4 * pi:
        return 1
    if -2 * pi < x < 0:
        return 2
    return 3


def reference_step(state, action, dt):
    """(new state as six mpf, the headings of the six _state_dot evaluations minus the start heading as mpf, the unwrapped new
    heading) of one Vessel.step from finite float64 inputs."""
    global _C
    if _C is None:
        _C = _constants()
    K = _C
    f = _mp.mpf
    a0, a1 = float(action[0]), float(action[1])
    if np.isnan(a0) or np.isnan(a1):                            # environment.py:314-315
        a0 = a1 = 0.0
    tau = _mp.matrix([f(min(max(a0, 0.0), 1.0)) * f(THRUST_MAX), 0, f(min(max(a1, -1.0), 1.0)) * f(MOMENT_MAX)])
    y = _mp.matrix([f(float(s)) for s in state])
    h = f(float(dt))
    incs = []

    def sdot(s):
        incs.append(s[2] - y[2])
        psi = _princip(s[2])
        c, sn = _mp.cos(psi), _mp.sin(psi)
        nu = _mp.matrix([s[3], s[4], s[5]])
        u = nu[0]
        eta = _mp.matrix([c * nu[0] - sn * nu[1], sn * nu[0] + c * nu[1], nu[2]])
        N = _mp.matrix([[-K["X_u"], 0, 0], [0, -K["Y_v"], K["m"] * u - K["Y_r"]], [0, -K["N_v"], K["m"] * K["x_g"] * u - K["N_r"]]])
        nud = K["M_inv"] * (tau - K["D"] * nu - N * nu)
        return _mp.matrix([eta[0], eta[1], eta[2], nud[0], nud[1], nud[2]])

    s1 = sdot(y)
    s2 = sdot(y + h * s1 / 4)
    s3 = sdot(y + 3 * h * s1 / 32 + 9 * h * s2 / 32)
    s4 = sdot(y + 1932 * h * s1 / 2197 - 7200 * h * s2 / 2197 + 7296 * h * s3 / 2197)
    s5 = sdot(y + 439 * h * s1 / 216 - 8 * h * s2 + 3680 * h * s3 / 513 - 845 * h * s4 / 4104)
    s6 = sdot(y - 8 * h * s1 / 27 + 2 * h * s2 - 3544 * h * s3 / 2565 + 1859 * h * s4 / 4104 - 11 * h * s5 / 40)
    q = y + h * (16 * s1 / 135 + 6656 * s3 / 12825 + 28561 * s4 / 56430 - 9 * s5 / 50 + 2 * s6 / 55)
    raw = q[2]
    out = [q[i] for i in range(6)]
    out[2] = _princip(raw)
    return out, incs, raw


# ------------------------------------------------------------------------------------------------ the rows
def _row(x=0.0, y=0.0, psi=0.0, u=0.0, v=0.0, r=0.0, a0=0.0, a1=0.0, dt=0.5):
    return (np.array([x, y, psi, u, v, r], dtype=np.float64), np.array([a0, a1], dtype=np.float64), float(dt))


def _yaw_change(u, v, r, a0, a1, dt):
    """The change of heading over one step (it does not depend on x, y, psi), to float64: places a row's new heading."""
    _, _, raw = reference_step([0.0, 0.0, 0.0, u, v, r], [a0, a1], dt)
    return float(raw)


def _ordinary(rs, k, dt):
    """k rows drawn as the K1 goldens are (oracle/ref_harness/make_golden.py:119-134)."""
    out = []
    for _ in range(k):
        out.append(_row(rs.uniform(-1500, 1500), rs.uniform(-1500, 1500), rs.uniform(-PI, PI), rs.uniform(-0.5, 2.0),
                        rs.uniform(-0.5, 0.5), rs.uniform(-0.6, 0.6), rs.uniform(-1.5, 1.5), rs.uniform(-1.5, 1.5), dt))
    return out


@functools.lru_cache(maxsize=None)
def groups():
    """name -> list of rows.  Deterministic (seeded)."""
    g = {}
    # ---- stage_limit: the heading of the second _state_dot evaluation is psi_0 + dt r / 4; r makes that increment 0.125 exactly
    # and one unit in the last place to either side, where stage_sincos goes from its Taylor branch to the full sincos.  With
    # psi_0 = 0 the kernel's difference psi_stage - psi_0 is the increment itself; with psi_0 = 0.7 and -2.9 the rounding of the
    # sum decides the side.
    rows = []
    for dt in DTS:
        r0 = 0.5 / dt                                           # dt r0 / 4 = 0.125 exactly (powers of two throughout)
        for sign in (1.0, -1.0):
            for r in (r0, np.nextafter(r0, 0.0), np.nextafter(r0, 2.0 * r0)):
                for psi in (0.0, 0.7, -2.9):
                    rows.append(_row(3.0, -4.0, psi, 1.0, 0.1 * sign, sign * r, 0.6, 0.3 * sign, dt))
    g["stage_limit"] = rows
    # ---- stage_mixed: steps whose six evaluations use both branches, or the second branch throughout -- dt = 8 with full rudder
    # from rest, dt = 8 with r = +-0.6, dt = 1 with r = +-2 and +-5 (unphysical, but a written state may hold them)
    rows = []
    for s in (1.0, -1.0):
        rows.append(_row(0.0, 0.0, 0.3, 0.0, 0.0, 0.0, 1.0, s, 8.0))
        rows.append(_row(10.0, -20.0, -1.1, 1.2, 0.0, 0.0, 0.5, s, 8.0))
        rows.append(_row(1.0, 2.0, 2.5, 1.0, 0.05, 0.6 * s, 0.7, -0.4 * s, 8.0))
        rows.append(_row(-7.0, 5.0, 0.2, 1.5, -0.1, 2.0 * s, 0.8, 0.2, 1.0))
        rows.append(_row(2.0, 9.0, -2.0, 0.8, 0.2, 5.0 * s, 0.3, -0.9, 1.0))
        rows.append(_row(0.0, 0.0, 1.0, 1.0, 0.0, 1.2 * s, 1.0, 1.0, 0.5))
    g["stage_mixed"] = rows
    # ---- wrap: auv_princip's branches, in heading0 (the start heading as written: outside [-pi, pi), on the limits of the
    # branches to a unit in the last place) and in the final wrap (a new heading just inside +-pi, past it, two periods away)
    rows = []
    starts = [-PI, np.nextafter(PI, 0.0), np.nextafter(-PI, -4.0), PI, 3.0 * PI - 1e-9, -3.0 * PI + 1e-9, 10.0, -10.0,
              np.nextafter(-PI, 0.0), 3.0 * PI, np.nextafter(3.0 * PI, 0.0), -3.0 * PI, np.nextafter(-3.0 * PI, 0.0), 4.0, -4.0, 7.5, -7.5]
    for i, psi in enumerate(starts):
        for dt in (0.5, 1.0):
            s = 1.0 if i % 2 == 0 else -1.0
            rows.append(_row(5.0, 6.0, psi, 1.3, 0.1 * s, 0.3 * s, 0.7, 0.5 * s, dt))
    for psi in (PI, -PI, 10.0, -10.0):
        rows.append(_row(5.0, 6.0, psi, 1.0, 0.0, 0.1, 0.5, 0.2, 8.0))
    for dt, s, gap in ((0.5, 1.0, 5e-13), (1.0, 1.0, 1e-13), (8.0, 1.0, 2e-15), (0.5, -1.0, 5e-13), (1.0, -1.0, 1e-13), (8.0, -1.0, 2e-15)):
        u, v, r, a0, a1 = 1.1, 0.05 * s, 0.25 * s, 0.6, 0.4 * s       # the new heading lands `gap` inside +-pi
        rows.append(_row(-3.0, 8.0, s * (PI - gap) - _yaw_change(u, v, r, a0, a1, dt), u, v, r, a0, a1, dt))
    rows.append(_row(0.0, 0.0, 3.0, 1.0, 0.0, 1.0, 1.0, 1.0, 8.0))     # wraps twice in one step
    rows.append(_row(0.0, 0.0, -3.0, 1.0, 0.0, -1.0, 1.0, -1.0, 8.0))
    g["wrap"] = rows
    # ---- wrap_large: start headings of 1e3 and 1e6 (the fmod branch): reducing them costs absolute accuracy in any float64 code
    rows = []
    for psi in (1e3, -1e3, 1e6, -1e6):
        for dt in DTS:
            rows.append(_row(5.0, 6.0, psi, 1.3, 0.1, 0.3, 0.7, 0.5, dt))
    g["wrap_large"] = rows
    # ---- action: the clip at its limits and a unit in the last place beyond, infinities, a NaN in either component (the whole
    # action then counts as zero), -0.0, values float32 does not hold
    rows = []
    a0s = [-0.0, 0.0, np.nextafter(0.0, -1.0), 1.0, np.nextafter(1.0, 2.0), np.inf, -np.inf, 1e300, -1e300, 0.1, 0.7, -1.5, 1.5,
           np.nextafter(1.0, 0.0)]
    a1s = [1.0, -1.0, np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0), np.inf, -np.inf, 0.1, -0.0, 1.5, -1.5, 1e300, -1e300,
           np.nextafter(1.0, 0.0), 1e-40]
    for i, a0 in enumerate(a0s):
        rows.append(_row(1.0, -2.0, 0.4, 0.9, 0.02, 0.05, a0, (0.3, -0.6, 0.1)[i % 3], (0.5, 1.0)[i % 2]))
    for i, a1 in enumerate(a1s):
        rows.append(_row(1.0, -2.0, -0.4, 0.9, -0.02, -0.05, (0.4, 0.1, 0.9)[i % 3], a1, (0.5, 1.0)[i % 2]))
    for a in ((np.nan, np.inf), (np.inf, np.nan), (np.nan, np.nan), (np.nan, 0.5), (0.5, np.nan), (-np.inf, np.nan)):
        rows.append(_row(1.0, -2.0, 0.4, 0.9, 0.02, 0.05, a[0], a[1], 0.5))
    rows.append(_row(0.0, 0.0, 0.0, -0.0, 0.0, 0.0, -0.0, -0.0, 0.5))
    rows.append(_row(0.0, 0.0, 0.0, 1.0, 0.0, 0.0, np.inf, -np.inf, 8.0))
    g["action"] = rows
    # ---- magnitude: positions of 1e6, speeds no episode reaches, the state at rest, a denormal yaw rate
    rows = []
    for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        rows.append(_row(sx * 1e6, sy * 1e6, 0.8 * sx, 1.5, 0.1 * sy, 0.2, 0.5, 0.3, 0.5 if sx > 0 else 1.0))
    for v in (20.0, -20.0):
        for dt in (0.5, 1.0):
            rows.append(_row(0.0, 0.0, 0.5, 50.0, v, 0.1, 1.0, 0.0, dt))
    for dt in DTS:
        rows.append(_row(dt=dt))
    for r in (5e-324, -5e-324, 1e-310):
        rows.append(_row(0.0, 0.0, 0.0, 1.0, 0.0, r, 0.5, 0.0, 1.0))
    g["magnitude"] = rows
    # ---- ordinary: states drawn as the goldens are -- the rows beside the poisoned ones in neighbour_batches(), and every
    # evaluation on the Taylor branch
    rs = np.random.RandomState(20261)
    g["ordinary"] = _ordinary(rs, sum(NEIGHBOUR_SIZES), NEIGHBOUR_DT) + _ordinary(rs, 12, 1.0) + _ordinary(rs, 12, 8.0)
    return g


@functools.lru_cache(maxsize=None)
def table():
    """The whole set: state [N, 6], action [N, 2], dt [N], group [N] (names), bounds [N] (the row's entry in BOUNDS_FILE: the
    error of any float64 code grows with the step size, so each group has one entry per dt)."""
    st, ac, dt, gr = [], [], [], []
    for name, rows in groups().items():
        for s, a, h in rows:
            st.append(s), ac.append(a), dt.append(h), gr.append(name)
    t = dict(state=np.array(st), action=np.array(ac), dt=np.array(dt), group=np.array(gr),
             bounds=np.array(["%s/dt%g" % (n, h) for n, h in zip(gr, dt)]))     # a bounds entry per group and step size
    for v in t.values():
        v.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def neighbour_batches():
    """Batches of n = 1 ... 65 environments at dt = 0.5: ordinary rows, of which one holds a NaN and one an inf in a state
    component -- in the first, a middle or the last position, the last always among them (it is the environment that the idle
    lane groups of the last wave clamp to).  Each: dict(n, clean_state [n, 6], state [n, 6], action [n, 2], poisoned [k])."""
    rows = [r for r in groups()["ordinary"] if r[2] == NEIGHBOUR_DT]
    out, at = [], 0
    for k, n in enumerate(NEIGHBOUR_SIZES):
        clean = np.array([r[0] for r in rows[at:at + n]])
        action = np.array([r[1] for r in rows[at:at + n]])
        at += n
        state = clean.copy()
        other = 0 if k % 2 else n // 2                          # n = 7, 9, 64: a middle position; 8, 63, 65: the first
        inf = np.inf if k % 4 < 2 else -np.inf
        nan_at, inf_at = (n - 1, other) if k % 2 else (other, n - 1)      # the NaN and the inf take turns in the last position
        state[inf_at, (5 * k + 2) % 6] = inf                    # components 2, 1, 0, 5, 4, 3, 2
        poisoned = [n - 1]
        if n > 1:
            state[nan_at, k % 6] = np.nan                       # components 0, 1, 2, 3, 4, 5, 0
            poisoned.append(other)
        out.append(dict(n=n, clean_state=clean, state=state, action=action, poisoned=np.array(sorted(poisoned))))
    return out


def poisoned_rows():
    """(state [k, 6], action [k, 2]) of the environments neighbour_batches() poisons, at NEIGHBOUR_DT."""
    st = np.concatenate([b["state"][b["poisoned"]] for b in neighbour_batches()])
    ac = np.concatenate([b["action"][b["poisoned"]] for b in neighbour_batches()])
    return st, ac


def poisoned_clean_states():
    """[k, 6]: the rows of poisoned_rows() as they were before the NaN or the inf went in."""
    return np.concatenate([b["clean_state"][b["poisoned"]] for b in neighbour_batches()])


# ------------------------------------------------------------------------------------------------ expectations and errors
@functools.lru_cache(maxsize=None)
def expectations():
    """The reference on every row of table(): dict(mp = list of six-mpf lists, f64 [N, 6] (each rounded to nearest), incs [N, 6]
    (heading of each evaluation minus the start heading, float64), raw [N] (the new heading before the wrap, float64), near_pi
    [N] (the new heading within NEAR_PI of +-pi: compared modulo 2 pi))."""
    t = table()
    mp, f64, incs, raw = [], [], [], []
    for s, a, h in zip(t["state"], t["action"], t["dt"]):
        o, i, w = reference_step(s, a, h)
        mp.append(o), f64.append([float(v) for v in o]), incs.append([float(v) for v in i]), raw.append(float(w))
    f64 = np.array(f64)
    out = dict(mp=mp, f64=f64, incs=np.array(incs), raw=np.array(raw), near_pi=PI - np.abs(f64[:, 2]) <= NEAR_PI)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def errors(got, rows=None):
    """|got - reference| / scale per row and component [k, 6] for `got` [k, 6] on the rows `rows` (indices into table(); None:
    all).  scale = max(1, |reference|) for x, y, u, v, r and 1 for psi; psi modulo 2 pi where expectations()["near_pi"]."""
    ex = expectations()
    rows = np.arange(len(ex["mp"])) if rows is None else np.asarray(rows)
    got = np.asarray(got, dtype=np.float64)
    out = np.empty((len(rows), 6))
    two_pi = _mp.mpf(PI) * 2
    for k, i in enumerate(rows):
        for c in range(6):
            if not np.isfinite(got[k, c]):
                out[k, c] = np.inf
                continue
            d = abs(_mp.mpf(float(got[k, c])) - ex["mp"][i][c])
            if c == 2:
                if ex["near_pi"][i]:
                    d = min(d, abs(two_pi - d))
            else:
                d = d / max(_mp.mpf(1), abs(ex["mp"][i][c]))
            out[k, c] = float(d)
    return out


def group_max(err, rows=None):
    """{bounds entry: {component: largest error}} of errors() output."""
    names = table()["bounds"] if rows is None else table()["bounds"][np.asarray(rows)]
    return {str(g): {c: float(err[names == g, k].max()) for k, c in enumerate(COMPONENTS)} for g in dict.fromkeys(names.tolist())}


def oracle_step(state, action, dt):
    """One `Oracle.step_dynamics` on rows of one dt: the new states [k, 6]."""
    from gym_auv_amd._capi import make_config
    from gym_auv_amd.config import effective_reference_config
    from gym_auv_amd.scenarios import moving_obstacles_world
    from gym_auv_amd.world import build_world, pack_bank
    from oracle.pyoracle import Oracle
    cfg = effective_reference_config()
    cfg.simulation.t_step_size = float(dt)
    ora = Oracle(make_config(cfg, auto_reset=False), len(state), pack_bank([build_world(moving_obstacles_world(0, 0, 0))]))
    ora.reset()
    ora.write("STATE", np.ascontiguousarray(np.asarray(state, dtype=np.float64).T))
    ora.step_dynamics(np.asarray(action, dtype=np.float64))
    out = ora.read("STATE").T.copy()
    ora.close()
    return out


@functools.lru_cache(maxsize=None)
def oracle_table():
    """The oracle's new state on every row of table() [N, 6]."""
    t = table()
    out = np.empty_like(t["state"])
    for dt in DTS:
        sel = t["dt"] == dt
        out[sel] = oracle_step(t["state"][sel], t["action"][sel], dt)
    out.setflags(write=False)
    return out


def load_bounds():
    with open(BOUNDS_FILE) as f:
        return json.load(f)


def tolerances():
    """{bounds entry: [6]} -- the GPU bound: BOUND_FACTOR times the oracle's recorded error, at least BOUND_FLOOR_ULPS units in the last
    place of the scale (errors() is relative to the scale, so that floor is a multiple of 2^-52)."""
    return {g: np.array([max(BOUND_FACTOR * v[c], BOUND_FLOOR_ULPS * EPS) for c in COMPONENTS]) for g, v in load_bounds().items()}


if __name__ == "__main__":                                      # python tests/dynamics_edge_rows.py: measure and record the oracle's error
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    rec = group_max(errors(oracle_table()))                     # {group: {component: number}}: the file holds numbers only
    with open(BOUNDS_FILE, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, indent=1))
