"""Hand-built worlds for the edges of the moving obstacles' update (k2_movers, phase A of the LiDAR sweep; no GPU needed here).

Every world is a straight 300 m path along +x from the origin, the vessel at rest on its start, at most one static circle, and
movers given as `MoverSpec`s directly.  All of them go into ONE bank (`bank(dt)`), so that every velocity-table offset after
the first world is non-zero, and neighbours differ in table length and in mover count:

  short_a     n_vel 5, 1, 2 with full tables [n_vel, 2] (every row different) -- n_vel 1 and 2 restart on every step
  const       a constant table [1, 2] under n_vel 4 and 7: the clamp `idx > vlen - 1` and the restart together
  short_b     n_vel 3, 9, 2, 5 with full tables
  axes        headings on the axes and at the cut of atan2 as table rows -- (v, 0) (0, v) (0, -v) (-v, +0.0) (-v, -0.0) (0, 0)
              (-0.0, -0.0) (v, -0.0): +0, +pi/2, -pi/2, +pi, -pi, +0, -pi, -0 -- once as the rows of one table of n_vel 9 and once
              each as a constant table of n_vel 3 (so that every heading also comes at a dt that rewinds on every step)
  onto        restart onto the vessel: pos0 within one obstacle width of the vessel's start pose, row 0 of the table nearly at
              rest, row 1 at 400 m per tick (more than sensor_range away in one tick), n_vel 4, 3 and 14
  many        70 movers and no static obstacle (m_max = 70: a second trip of phase A's loop, a second pass of the obstacle phase)
  one         one mover

Widths 0.5, 6 and 30.  A mover's reset-time state is `world.advance_mover` with dt = 0.1 (the constructor's update) and then
with the step size (the scenario's trailing update), the way scenarios._mover_from_table does it -- so a bank belongs to one dt.

The expected values of the tests that use these worlds rest on `world.advance_mover` and on the oracle's update_movers, both
transcriptions of the reference's VesselObstacle._update (objects/obstacles.py:195-215); the reference itself is not run.
"""
import functools

import numpy as np

from gym_auv_amd.world import advance_mover, build_world, pack_bank
from gym_auv_amd.worldspec import MoverSpec, WorldSpec

DTS = (0.5, 1.0, 0.3, 8.0)          # the reference's; 1; a counter that accumulates rounding; past n_vel - 1 at once
STEPS = 40
MAX_TIMESTEPS = 13                  # the auto-resetting runs: episodes end between restarts
V = 3.0                             # speed of the axis rows (m per tick)
WORLD_NAMES = ("short_a", "const", "short_b", "axes", "onto", "many", "one")
ONTO_WIDTH = 6.0
AXIS_ROWS = ((V, 0.0), (0.0, V), (0.0, -V), (-V, 0.0), (-V, -0.0), (0.0, 0.0), (-0.0, -0.0), (V, -0.0))
AXIS_HEADINGS = (0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, 0.0, -np.pi, -0.0)


def make_mover(width, pos0, vel, n_vel, dt) -> MoverSpec:
    """A VesselObstacle of velocity table `vel` ([n_vel, 2], or [1, 2] for a constant one) in its reset-time state."""
    vel = np.array(vel, dtype=np.float64).reshape(-1, 2)
    pos0 = np.array(pos0, dtype=np.float64)
    assert len(vel) in (1, n_vel)
    param = (float(width), pos0[0], pos0[1], n_vel)
    st = (pos0[0], pos0[1], np.pi / 2, 0.0)
    st = advance_mover(param, vel, st, 0.1)          # the constructor's update(dt=0.1)
    st = advance_mover(param, vel, st, dt)           # the scenario's trailing _update()
    return MoverSpec(width=float(width), pos0=pos0, vel=vel, n_vel=int(n_vel), pos=np.array(st[:2]), heading=float(st[2]),
                     counter=float(st[3]))


def _table(n, seed):
    """[n, 2] with every component of every row different: multiples of 1/8 m per tick in [-4, 4], none zero."""
    rs = np.random.RandomState(seed)
    vals = np.concatenate([np.arange(-32, 0), np.arange(1, 33)]) / 8.0
    return rs.choice(vals, size=2 * n, replace=False).reshape(n, 2)


def _world(name, movers, circle=None):
    wp = np.array([[0.0, 300.0], [0.0, 0.0]])
    circles = np.zeros((0, 3)) if circle is None else np.array([circle], dtype=np.float64)
    return WorldSpec(waypoints=wp, vessel_init=np.array([0.0, 0.0, 0.0]), circles=circles, movers=movers, name=name)


def onto_table(n_vel):
    """Row 0 nearly at rest (the restart leaves the obstacle on the vessel), row 1 and the rows from 8 on at 400 m per tick, the
    others slow and distinct."""
    t = _table(n_vel, 40 + n_vel) / 4.0
    t[0] = (0.03125, -0.015625)
    t[1] = (400.0, 100.0)
    for k in range(8, n_vel):         # (row 8: the one a step size of 8 reads when it does not rewind)
        t[k] = (344.0 + 8.0 * k, 128.0 - 4.0 * k)
    return t


def specs(dt, many=True):
    """The edge worlds in the bank's order (WORLD_NAMES; without "many" when `many` is False)."""
    mk = lambda *a: make_mover(*a, dt)          # noqa: E731
    out = [
        _world("short_a", [mk(0.5, (40.0, -20.0), _table(5, 2), 5), mk(6.0, (60.0, 30.0), _table(1, 1), 1),
                           mk(30.0, (-20.0, 90.0), _table(2, 3), 2)], circle=(70.0, -40.0, 10.0)),
        _world("const", [mk(6.0, (50.0, 10.0), [(1.5, -0.75)], 4), mk(30.0, (-60.0, -50.0), [(-2.25, 1.125)], 7)]),
        _world("short_b", [mk(6.0, (80.0, 5.0), _table(3, 5), 3), mk(0.5, (30.0, 12.0), _table(9, 4), 9),
                           mk(6.0, (-30.0, -30.0), _table(2, 6), 2), mk(30.0, (20.0, 100.0), _table(5, 7), 5)],
               circle=(-50.0, 40.0, 5.0)),
        _world("axes", [mk(6.0, (40.0, 25.0), list(AXIS_ROWS) + [(1.0, -2.0)], 9)] +
               [mk((0.5, 6.0, 30.0)[k % 3], (-80.0 + 25.0 * k, -60.0 + 15.0 * (k % 4)), [row], 3) for k, row in enumerate(AXIS_ROWS)]),
        _world("onto", [mk(ONTO_WIDTH, (3.0, -1.0), onto_table(4), 4), mk(ONTO_WIDTH, (-2.0, 4.0), onto_table(3), 3),
                        mk(ONTO_WIDTH, (1.0, -3.0), onto_table(14), 14)], circle=(90.0, 60.0, 10.0)),
    ]
    if many:
        nv = (1, 2, 3, 5, 9)
        out.append(_world("many", [mk((0.5, 6.0, 30.0)[j % 3], (-140.0 + 4.0 * j, 50.0 - 3.0 * (j % 23)), _table(nv[j % 5], 100 + j), nv[j % 5])
                                   for j in range(70)]))
    out.append(_world("one", [mk(6.0, (25.0, -15.0), _table(5, 8), 5)], circle=(45.0, 30.0, 5.0)))
    return out


@functools.lru_cache(maxsize=None)
def bank(dt, many=True):
    return pack_bank([build_world(s) for s in specs(dt, many)])


def world_index(name, many=True):
    return [w for w in WORLD_NAMES if many or w != "many"].index(name)


def n_envs(many=True):
    """16 environments, or 8 times the number of worlds where that is larger (a multiple of it: an auto-reset keeps the world)."""
    return max(16, 8 * (len(WORLD_NAMES) - (0 if many else 1)))


def config(dt, ns=8, nps=8, max_timesteps=MAX_TIMESTEPS):
    from gym_auv_amd.config import effective_reference_config
    cfg = effective_reference_config(use_lidar=True)
    cfg.vessel.n_sectors, cfg.vessel.n_sensors_per_sector = ns, nps
    cfg.simulation.t_step_size = dt
    cfg.episode.max_timesteps = max_timesteps
    return cfg


def actions(dt, n, many=True, steps=STEPS, seed=0):
    """[steps, n, 2]: random thrust and rudder, zero for the environments of the "onto" world (the vessel stays put) -- and for
    all of them at dt = 8, where the explicit integration of the vessel's dynamics diverges (1e50 m within 40 steps): the vessel
    is not what these worlds are about."""
    rs = np.random.RandomState(seed)
    a = rs.uniform([0.0, -0.15], [1.0, 0.15], (steps, n, 2))
    if dt == 8.0:
        a[:] = 0.0
    W = len(WORLD_NAMES) - (0 if many else 1)
    a[:, np.arange(n) % W == world_index("onto", many)] = 0.0
    return a


def restart_steps(n_vel, dt, steps=STEPS):
    """The steps (1 .. steps) that rewind a mover of `n_vel` ticks: the counter's arithmetic alone -- 0.1, then dt per update,
    back to 0 when its floor reaches n_vel - 1 -- in the sequential fp64 sums every implementation forms."""
    c, out = 0.0, []
    for t, d in enumerate([0.1, dt] + [dt] * steps, start=-1):
        c += d
        if int(np.floor(c)) >= n_vel - 1:
            c = 0.0
            if t >= 1:
                out.append(t)
    return out


def movers_of(bank_, w):
    """(param [4], velocity table [vlen, 2], reset-time state [4]) of every mover of world `w`, from the bank's own tables."""
    m0, m1 = int(bank_["mv_off"][w]), int(bank_["mv_off"][w + 1])
    vo = bank_["mv_vtab_off"]
    return [(bank_["mv_param"][m], bank_["mv_vtab"][int(vo[m]):int(vo[m + 1])], bank_["mv_init"][m]) for m in range(m0, m1)]


def n_vel_of(bank_, n):
    """[n, m_max]: n_vel of every mover row of an n-environment handle (environment e in world e % n_worlds); 0 marks the
    padding rows of worlds with fewer movers."""
    W = int(bank_["n_worlds"])
    nv = np.zeros((n, max(1, int(bank_["m_max"]))), dtype=np.int64)
    for e in range(n):
        m0, m1 = int(bank_["mv_off"][e % W]), int(bank_["mv_off"][e % W + 1])
        nv[e, :m1 - m0] = bank_["mv_param"][m0:m1, 3]
    return nv


def restarts(mover_rows, done=None):
    """[steps, n, m_max] bool: the step rewound the mover (its counter is exactly 0 afterwards; any other step leaves it > 0).
    `done` [steps, n]: steps that ended an episode are left out -- an auto-reset has overwritten their rows with the reset state.
    (Padding rows are zero throughout: mask with n_vel_of(...) > 0.)"""
    r = np.asarray(mover_rows)[..., 3] == 0.0
    if done is not None:
        r = r & ~np.asarray(done, dtype=bool)[..., None]
    return r
