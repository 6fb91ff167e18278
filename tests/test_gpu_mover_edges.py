"""-m gpu: the moving obstacles' update (k2_movers, phase A of the LiDAR sweep) where it can go wrong unnoticed -- the restart
`idx >= n_vel - 1`, the clamp of constant tables, per-mover table offsets that are not zero, headings on the axes and at the cut
of atan2, an obstacle rewound onto the vessel between two refreshes of the nearby list, 70 movers in one world -- on the worlds
of tests/mover_edge_banks.py, in every step shape.

The expected values are the oracle's (oracle/auv_oracle.c: update_movers), which tests/test_mover_edges.py holds bit for bit to
`world.advance_mover` on the very same worlds and which asserts there that the worlds present what they are for.  Both are
transcriptions of the reference's VesselObstacle._update (objects/obstacles.py:195-215); the reference itself cannot be run
where these tests run (it needs shapely), so nothing here is compared with it directly.

Position and counter are compared bit for bit: one product, one sum, one floor, FMA contraction off.  The heading is not libm's
atan2 on the device: where the oracle's heading is +-0.0 the bits must agree, sign included; elsewhere the sign must agree (+pi is
not -pi) and the difference stay within HEADING_ATOL.  Measured on the MI355X over all cases of this file: the largest absolute
difference is 4.441e-16 = 2^-51 (MEASURED_HEADING_DIFF, one unit in the last place of pi, the same in every run); the bound
is four times that, rounded up to a power of two: HEADING_ATOL = 2^-49 = 1.776e-15.
"""
import functools
import warnings

import numpy as np
import pytest
import torch

import mover_edge_banks as mb
from helpers import shape_run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEASURED_HEADING_DIFF = 2.0 ** -51   # 4.441e-16, one unit in the last place of pi: in every run of this file
HEADING_ATOL = 2.0 ** -49            # 1.776e-15 = 4 * MEASURED_HEADING_DIFF, a power of two as it stands (far below the 1e-12 cap)
ATOL = 1e-9                          # the suite's standing fp64 bound (tests/test_gpu_edge.py::_run)
FIELDS_TOL = ("STATE", "LIDAR_D", "OBS64", "REWARD64", "INFO64", "NAV64")
FIELDS_EXACT = ("COLLISION", "NEARBY", "CULL_LIMITS", "WORLD_IDX")
SHAPE_FIELDS = ("MOVER_STATE", "LIDAR_D", "CULL_LIMITS", "NEARBY", "COLLISION")
SHAPE_MAX_TIMESTEPS = 29             # the step-shape runs: n_vel 9 rewinds inside an episode at both step sizes
LENGTHS = (5, 16)                    # steps per multi-step launch: rewinds of n_vel 3, 5, 9 at the first, the last, an inner step


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _env(cfg, bank, n, auto_reset=True, **kw):
    from gym_auv_amd.batched_env import BatchedAuvEnv
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (fewer worlds than environments: an episode restarts in its own world)
        return BatchedAuvEnv(cfg, bank, n, device=DEV, auto_reset=auto_reset, **kw)


def _assert_movers(got, want, msg):
    """MOVER_STATE [n, m_max, 4] against the oracle's: x, y, counter bit for bit, the heading by the rule of the docstring."""
    for c, name in ((0, "x"), (1, "y"), (3, "counter")):
        bad = np.argwhere(_bits(got[..., c]) != _bits(want[..., c]))
        assert len(bad) == 0, "%s: mover %s differs at (env, mover) %s: %r against %r" % (
            msg, name, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    h, w = got[..., 2], want[..., 2]
    zero = w == 0.0
    assert np.array_equal(_bits(h[zero]), _bits(w[zero])), "%s: a heading of +-0.0 differs" % msg
    assert np.array_equal(np.signbit(h), np.signbit(w)), "%s: a heading's sign differs" % msg
    diff = float(np.abs(h - w).max())
    print("%s: largest heading difference %.3e" % (msg, diff))
    assert diff <= HEADING_ATOL, "%s: heading off by %.3e" % (msg, diff)
    return diff


@functools.lru_cache(maxsize=None)
def _oracle_rows(dt, ns, nps, many, auto_reset, max_timesteps, per_kernel=False):
    """The oracle's fields after each of the 40 steps (computed once per configuration and shared, read only)."""
    from gym_auv_amd._capi import make_config
    from oracle.pyoracle import Oracle
    bank, n = mb.bank(dt, many), mb.n_envs(many)
    ora = Oracle(make_config(mb.config(dt, ns, nps, max_timesteps), auto_reset=auto_reset), n, bank)
    ora.reset()
    acts = mb.actions(dt, n, many)
    rows = []
    for t in range(mb.STEPS):
        if per_kernel:
            ora.step_dynamics(acts[t]), ora.lidar(True)
            done = ora.nav_reward(0)
        else:
            _, _, done = ora.step(acts[t])
        row = {f: ora.read(f) for f in FIELDS_TOL + FIELDS_EXACT + ("MOVER_STATE",)}
        row["done"] = done.copy()
        rows.append(row)
    ora.close()
    return rows


def _against_oracle(dt, mode, ns=8, nps=8, many=True, auto_reset=True, max_timesteps=mb.MAX_TIMESTEPS):
    bank, n = mb.bank(dt, many), mb.n_envs(many)
    want = _oracle_rows(dt, ns, nps, many, auto_reset, max_timesteps, mode == "kernels")
    env = _env(mb.config(dt, ns, nps, max_timesteps), bank, n, auto_reset=auto_reset)
    if mode != "kernels":
        env.set_step_mode(mode)
    env.reset()
    acts = torch.as_tensor(mb.actions(dt, n, many), device=DEV)
    worst, rewinds, dones = 0.0, 0, 0
    real = mb.n_vel_of(bank, n) > 0
    for t in range(mb.STEPS):
        if mode == "kernels":
            env.step_dynamics(acts[t]), env.lidar(True)
            done = env.nav_reward(0)
        else:
            _, _, done, _ = env.step(acts[t])
        torch.cuda.synchronize()
        msg = "dt %g %s step %d" % (dt, mode, t + 1)
        worst = max(worst, _assert_movers(_np(env.read("MOVER_STATE")), want[t]["MOVER_STATE"], msg))
        np.testing.assert_array_equal(_np(done), want[t]["done"], err_msg="done " + msg)
        for f in FIELDS_EXACT:
            np.testing.assert_array_equal(_np(env.read(f)), want[t][f], err_msg="%s %s" % (f, msg))
        for f in FIELDS_TOL:
            np.testing.assert_allclose(_np(env.read(f)), want[t][f], rtol=0, atol=ATOL, err_msg="%s %s" % (f, msg))
        rewinds += int((mb.restarts(want[t]["MOVER_STATE"][None], want[t]["done"][None])[0] & real).sum())
        dones += int(want[t]["done"].sum())
    assert env.health()["timeouts"] == 0
    env.close()
    print("dt %g %s: largest heading difference over the run %.3e" % (dt, mode, worst))
    return want, rewinds, dones


# ------------------------------------------------------------------------------------------------ a, b: against the oracle
@pytest.mark.parametrize("mode", ["one_launch", "side_by_side"])
@pytest.mark.parametrize("dt", mb.DTS, ids=["dt%g" % d for d in mb.DTS])
def test_movers_against_the_oracle(dt, mode):
    """The whole bank, the 70-mover world included, auto-reset on with episodes of 13 steps: an episode ends between rewinds and
    the next starts from mv_init, counter included."""
    _, rewinds, dones = _against_oracle(dt, mode)
    assert rewinds >= 500 and dones >= mb.n_envs() * 3


@pytest.mark.parametrize("dt", [0.5, 0.3], ids=["dt0.5", "dt0.3"])
def test_movers_in_the_stand_alone_sweep(dt):
    """step_dynamics / lidar / nav_reward: phase A as auv_lidar's own launch runs it, against the oracle's same three calls."""
    _against_oracle(dt, "kernels")


@pytest.mark.parametrize("ns,nps", [(8, 8), (9, 20)], ids=["S64", "S180"])
@pytest.mark.parametrize("auto_reset", [True, False], ids=["episodes13", "no_reset"])
def test_restart_onto_the_vessel(ns, nps, auto_reset):
    """An obstacle rewound onto the vessel at rest.  Without resets the nearby list is refreshed at vessel step 25: rewinds
    before it are seen or missed by the list of the reset, those after it by the list of step 25 (test_mover_edges.py asserts
    that both happen, and a collision with the rewound obstacle)."""
    want, _, _ = _against_oracle(0.5, "one_launch", ns, nps, many=False, auto_reset=auto_reset,
                                 max_timesteps=mb.MAX_TIMESTEPS if auto_reset else 10000)
    e = mb.world_index("onto", many=False)
    assert any(r["COLLISION"][e] for r in want)
    if not auto_reset:
        near = np.array([r["NEARBY"][e, 1:4] for r in want]).astype(bool)
        mv = np.array([r["MOVER_STATE"][e, :3] for r in want])
        on_top = np.hypot(mv[..., 0], mv[..., 1]) < mb.ONTO_WIDTH
        assert (on_top & ~near).any() and (on_top & near).any()


def test_loader_takes_n_vel_1_and_refuses_0():
    """n_vel = 1 is a trajectory of two waypoints one tick apart, which the reference rewinds on every update (the loader used to
    refuse it: "n_vel < 2"); n_vel = 0 has no row to read and stays refused."""
    from gym_auv_amd.world import build_world, pack_bank
    spec = mb.specs(0.5, many=False)[0]
    assert [m.n_vel for m in spec.movers] == [5, 1, 2]
    env = _env(mb.config(0.5), pack_bank([build_world(spec)]), 16)
    env.close()
    spec.movers[1].n_vel = 0
    with pytest.raises(RuntimeError, match="n_vel < 1"):
        _env(mb.config(0.5), pack_bank([build_world(spec)]), 16)


def test_multi_step_entry_points_refuse_the_70_mover_bank():
    dt = 0.5
    n = mb.n_envs()
    env = _env(mb.config(dt), mb.bank(dt), n)
    env.reset()
    ring = torch.as_tensor(mb.actions(dt, n), device=DEV).contiguous()
    before = env.read("MOVER_STATE")
    with pytest.raises(RuntimeError, match="more than 64 obstacles"):
        env.step_multi(ring, 0, 7)
    with pytest.raises(RuntimeError, match="more than 64 obstacles"):
        env.step_multi(ring, 0, 7, record=True)
    with pytest.raises(RuntimeError, match="more than 64 obstacles"):
        env.step_feedback(torch.zeros((2, 8), dtype=torch.float64, device=DEV), 7, ring=ring)
    torch.cuda.synchronize()
    assert torch.equal(env.read("MOVER_STATE"), before)
    env.close()


# ------------------------------------------------------------------------------------------------ c: every other step shape
def _shape_setup(dt, n):
    cfg = mb.config(dt, max_timesteps=SHAPE_MAX_TIMESTEPS)
    bank = mb.bank(dt, many=False)
    W = int(bank["n_worlds"])
    assert n % W == 0
    a = mb.actions(dt, mb.n_envs(False), many=False)
    ring = torch.as_tensor(np.tile(a, (1, n // a.shape[1], 1)), dtype=torch.float32, device=DEV).contiguous()
    return cfg, bank, ring


@functools.lru_cache(maxsize=None)
def _one_launch_run(dt, n):
    cfg, bank, ring = _shape_setup(dt, n)
    return shape_run("one_launch", cfg, bank, n, ring, mb.STEPS, fields=SHAPE_FIELDS)


def _launch_ends():
    ends, t, i = [], 0, 0
    while t < mb.STEPS:
        t += min(LENGTHS[i % len(LENGTHS)], mb.STEPS - t)
        ends.append(t)
        i += 1
    return ends


def _short_table_rewinds(dt, n):
    """Steps (1-based) of the one-launch run at which a mover of n_vel 3, 5 or 9 was rewound."""
    ref = _one_launch_run(dt, n)
    sel = np.isin(mb.n_vel_of(mb.bank(dt, many=False), n), (3, 5, 9))
    return {t for t, v in ref.items() if (mb.restarts(_np(v[1])[None], _np(v[-1])[None])[0] & sel).any()}


@pytest.mark.parametrize("n", [mb.n_envs(False), 4 * mb.n_envs(False)], ids=["n48", "n192"])
@pytest.mark.parametrize("dt", [0.5, 0.3], ids=["dt0.5", "dt0.3"])
def test_rewinds_fall_on_every_position_of_a_launch(dt, n):
    """From the one-launch run: movers of n_vel 3, 5, 9 are rewound at the first step of a multi-step launch, at its last step and
    inside it, and episodes end inside the compared stretch."""
    at = _short_table_rewinds(dt, n)
    ends = _launch_ends()
    first, last = {1} | {e + 1 for e in ends[:-1]}, set(ends)
    inner = set(range(1, mb.STEPS + 1)) - first - last
    assert at & first and at & last and at & inner, (sorted(at), ends)
    assert sum(int(v[-1].sum()) for v in _one_launch_run(dt, n).values()) > 0


@pytest.mark.parametrize("shape_name", ["side_by_side", "chains", "async", "graph", "multi_cohorts", "multi_steps"])
@pytest.mark.parametrize("n", [mb.n_envs(False), 4 * mb.n_envs(False)], ids=["n48", "n192"])
@pytest.mark.parametrize("dt", [0.5, 0.3], ids=["dt0.5", "dt0.3"])
def test_every_step_shape_moves_obstacles_bitwise_the_same(dt, n, shape_name):
    """n = 48 is 8 environments per world; 192 gives the chained shapes three sub-batches and the multi-step launches three
    cohorts (sub-batch slices and cohorts are multiples of 64 environments)."""
    cfg, bank, ring = _shape_setup(dt, n)
    ref = _one_launch_run(dt, n)
    got = shape_run(shape_name, cfg, bank, n, ring, mb.STEPS, fields=SHAPE_FIELDS, lengths=LENGTHS)
    assert len(got) == (len(_launch_ends()) if shape_name.startswith("multi") else mb.STEPS)
    for t, v in got.items():
        for k, (a, b) in enumerate(zip(ref[t], v)):
            assert torch.equal(a, b), (shape_name, t, (("obs",) + SHAPE_FIELDS + ("reward", "done"))[k])


@pytest.mark.parametrize("kind", ["record", "feedback"])
@pytest.mark.parametrize("dt", [0.5, 0.3], ids=["dt0.5", "dt0.3"])
def test_record_and_feedback_launches_over_the_same_stretch(dt, kind):
    """The recording launch, and the feedback launch with zero gains on the observation and 1 on the ring's action (the law
    then returns the ring's action: the open-loop stretch of the one-launch run): every step's record row and the fields after
    every launch are the one-launch run's bits."""
    n = mb.n_envs(False)
    cfg, bank, ring = _shape_setup(dt, n)
    ref = _one_launch_run(dt, n)
    env = _env(cfg, bank, n)
    env.reset()
    env.set_sub_batches(1, strict=True)
    gains = torch.zeros((2, 8), dtype=torch.float64, device=DEV)
    gains[:, 7] = 1.0
    t = 0
    for end in _launch_ends():
        T = end - t
        if kind == "record":
            rec = env.step_multi(ring, t % ring.shape[0], T, record=True)
        else:
            rec = env.step_feedback(gains, T, ring=ring, first_slot=t % ring.shape[0], record=True)
        torch.cuda.synchronize()
        for j in range(T):
            for k, name in ((0, "obs"), (1, "reward"), (2, "done")):
                assert torch.equal(rec[k][j], ref[t + j + 1][0 if k == 0 else k - 3]), (kind, name, t + j + 1)
        now = (env.obs,) + tuple(env.read(f) for f in SHAPE_FIELDS) + (env.reward, env.done)
        for a, b in zip(ref[end], now):
            assert torch.equal(a, b), (kind, end)
        t = end
    assert env.health()["timeouts"] == 0
    env.close()


# ------------------------------------------------------------------------------------------------ d: snapshot and restore
def test_snapshot_and_restore_across_a_restart():
    """A snapshot one step before movers of n_vel 3 are rewound (step 3 at dt = 0.5; n_vel 4 and 5 follow at steps 5 and 7),
    five steps, restore, the same five steps again: the same bits.  An environment forked into a row of another world at that
    point is its twin from then on."""
    dt = 0.5
    n = mb.n_envs(False)
    bank = mb.bank(dt, many=False)
    W = int(bank["n_worlds"])
    env = _env(mb.config(dt, max_timesteps=10000), bank, n, auto_reset=False)
    env.reset()
    acts = mb.actions(dt, n, many=False)
    src, dst = mb.world_index("short_b", False), mb.world_index("one", False) + W          # rows of different worlds
    acts[:, dst] = acts[:, src]
    acts = torch.as_tensor(acts, device=DEV)
    for t in range(2):
        env.step(acts[t])
    snap = env.snapshot()

    def stretch():
        out = []
        for t in range(2, 7):
            env.step(acts[t])
            torch.cuda.synchronize()
            out.append((env.read("MOVER_STATE"), env.read("LIDAR_D"), env.obs.clone(), env.read("STATE")))
        return out

    first = stretch()
    nv = mb.n_vel_of(bank, n)
    rewound = [mb.restarts(_np(r[0])[None])[0] for r in first]
    assert (rewound[0] & (nv == 3)).any() and (rewound[2] & (nv == 4)).any() and (rewound[4] & (nv == 5)).any()
    assert not torch.equal(first[0][0], first[4][0])
    env.restore(snap)
    second = stretch()
    for t, (x, y) in enumerate(zip(first, second)):
        for k, name in enumerate(("MOVER_STATE", "LIDAR_D", "obs", "STATE")):
            assert torch.equal(x[k], y[k]), (name, t)
    # the fork: row `dst` (world "one") becomes a copy of row `src` (world "short_b": n_vel 3, 9, 2, 5) one step before the rewind
    env.restore(snap)
    env.fork([src], [dst])
    torch.cuda.synchronize()
    assert int(env.read("WORLD_IDX")[dst]) == src
    third = stretch()
    for t, (x, y) in enumerate(zip(first, third)):
        assert torch.equal(y[0][dst], x[0][src]) and torch.equal(y[1][dst], x[1][src]) and torch.equal(y[2][dst], x[2][src]), t
        assert torch.equal(y[3][:, dst], x[3][:, src]), t
        assert torch.equal(y[0][src], x[0][src]) and torch.equal(y[2][src], x[2][src]), t
    env.close()


# ------------------------------------------------------------------------------------------------ e: the renderer
def test_render_right_after_a_restart_of_the_axis_headings():
    """auv_render takes the movers' poses from MOVER_STATE: one frame of the "axes" world right after its nine-row table and
    all its constant tables were rewound (step 7 at dt = 1), bit for bit the NumPy mirror's (as tests/test_gpu_render.py), and
    the pentagons it drew are the oracle's arithmetic on that row's poses -- headings +-pi, +-pi/2 and +-0 among them."""
    from gym_auv_amd import render as R
    dt = 1.0
    n = mb.n_envs(False)
    bank = mb.bank(dt, many=False)
    env = _env(mb.config(dt, max_timesteps=10000), bank, n, auto_reset=False)
    env.reset()
    acts = torch.as_tensor(mb.actions(dt, n, many=False), device=DEV)
    for t in range(7):
        env.step(acts[t])
    torch.cuda.synchronize()
    e = mb.world_index("axes", False)
    mv = _np(env.read("MOVER_STATE"))[e]
    assert (mv[:9, 3] == 0.0).all()                                       # every mover of the world has just been rewound
    assert {np.pi, -np.pi, np.pi / 2, -np.pi / 2} <= set(mv[:9, 2].tolist())
    size, zoom = (96, 128), 1.0
    frames, geo = env.render(envs=[e], size=size, zoom=zoom, view="north_up", return_geometry=True)
    torch.cuda.synchronize()
    frames = _np(frames)
    geo = {k: _np(v) for k, v in geo.items()}
    ref = R.render_reference(geo["cam"], geo["dyn_seg"], geo["ray_seg"], geo["ray_q"], [R.world_tables(bank, e)], None, None, None,
                             size[0], size[1], 1.0)
    assert frames.shape == ref.shape and int((frames != ref).any(axis=3).sum()) == 0
    away = geo["dyn_seg"].copy()
    away[:, :5 * 9] = 1e6                                                 # the same frame with the movers out of sight
    blank = R.render_reference(geo["cam"], away, geo["ray_seg"], geo["ray_q"], [R.world_tables(bank, e)], None, None, None,
                               size[0], size[1], 1.0)
    shown = int((blank != ref).any(axis=3).sum())
    print("pixels the movers' pentagons decide: %d" % shown)
    assert shown > 20
    m0 = int(bank["mv_off"][e])
    for m in range(9):
        w = bank["mv_param"][m0 + m, 0]
        cc, ss = np.cos(mv[m, 2]), np.sin(mv[m, 2])
        cc, ss = (0.0 if abs(cc) < 2.5e-16 else cc), (0.0 if abs(ss) < 2.5e-16 else ss)
        x0 = 5.0 * w / 18.0
        bx = np.array([-w / 2, -w / 2, w / 2, 3.0 / 2 * w, w / 2])
        by = np.array([-w / 2, w / 2, w / 2, 0.0, -w / 2])
        vx = (cc * bx + -ss * by + (x0 - x0 * cc)) + mv[m, 0]
        vy = (ss * bx + cc * by + (0.0 - x0 * ss)) + mv[m, 1]
        want = np.stack([vx, vy, np.roll(vx, -1), np.roll(vy, -1)], axis=1)
        assert np.abs(geo["dyn_seg"][0, 5 * m:5 * m + 5] - want).max() <= 1e-12, m
    env.close()
