"""-m gpu: the vessel dynamics (K1) on the rows of tests/dynamics_edge_rows.py -- at the limit of stage_sincos's series branch,
with evaluations on both of its branches, across every branch of auv_princip, at the limits of the action clip, with non-finite
actions and states -- in every body that claims the one arithmetic: the stand-alone k1_dynamics (k1_group), the three-launch step
(k1_env), the one-launch step (k_step_roles, k1_group) and the multi-step and closed-loop launches (k1_group starting from the
carry record, the action from the ring slot or handed in by the feedback law).

Expected values: the 50-digit reference of dynamics_edge_rows.py.  Tolerance per bounds entry (row group and step size) and state
component: 8 times the error of the plain-float64 oracle recorded in tests/golden/k1_edge_bounds.json (tests/test_dynamics_edges.py
holds the file to the oracle), at least 4 ulp of the scale max(1, |value|); a reference heading within 1e-8 of +-pi is compared
modulo 2 pi.  Everything else is bit for bit between bodies, NaN positions counting as equal.

An environment whose STATE holds a NaN or an inf is held to the oracle: NaN where the oracle has NaN, an infinity where it has one,
its value (at the bound of the ordinary rows) where it is finite.  One exception, pinned as it is: the reference forms its
derivatives with dense products (Rz(psi).dot(nu), D.dot(nu), N(nu).dot(nu), M_inv.dot(...): vessel.py:567-568), whose zero
entries turn a non-finite v or r into NaN in EVERY component (0 * inf, 0 * NaN), the surge speed included, and the oracle does the
same; the kernel leaves the zero products out, and the surge equation holds neither v nor r (state_dot: o.v[3] = i11 * r0, r0 of
tau_u and u alone), so beside a non-finite v or r its new u is the bits of the same row without the poison."""
import functools
import warnings

import numpy as np
import pytest
import torch

import dynamics_edge_rows as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATOL = 1e-9                           # the suite's standing bound (tests/test_gpu_edge.py::_run)


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    """Bit for bit, NaN positions counting as equal."""
    return bool(((a.view(torch.int64) == b.view(torch.int64)) | (torch.isnan(a) & torch.isnan(b))).all())


def _diff_rows(a, b):
    bad = ~((a.view(torch.int64) == b.view(torch.int64)) | (torch.isnan(a) & torch.isnan(b)))
    return torch.nonzero(bad.any(dim=0)).flatten().tolist()


@functools.lru_cache(maxsize=None)
def _bank():
    from gym_auv_amd.scenarios import moving_obstacles_world
    from gym_auv_amd.world import build_world, pack_bank
    return pack_bank([build_world(moving_obstacles_world(0, 0, 0))])


def _env(dt, n):
    from gym_auv_amd.batched_env import BatchedAuvEnv
    from gym_auv_amd.config import effective_reference_config
    cfg = effective_reference_config(use_lidar=True)            # (without the sweep the library steps in three launches whatever is set)
    cfg.simulation.t_step_size = dt
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = BatchedAuvEnv(cfg, _bank(), n, device=DEV, auto_reset=False)
    env.reset()
    return env


def _rows_of(dt, group=None, poisoned=False):
    """(indices into R.table(), state [k, 6], action [k, 2]) of the rows of one step size; `poisoned`: the NaN / inf states of the
    neighbour batches behind them and, behind those, the same rows without the poison (no index)."""
    t = R.table()
    sel = t["dt"] == dt
    if group is not None:
        sel &= t["group"] == group
    idx = np.flatnonzero(sel)
    st, ac = t["state"][idx], t["action"][idx]
    if poisoned and dt == R.NEIGHBOUR_DT:
        ps, pa = R.poisoned_rows()
        st, ac = np.concatenate([st, ps, R.poisoned_clean_states()]), np.concatenate([ac, pa, pa])
    return idx, st, ac


def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _start(env, state):
    """Reset state, the rows written over it; returns the step counters before the step."""
    env.reset()
    env.write("STATE", np.ascontiguousarray(state.T))
    return env.read("COUNTERS")[:, 1].clone()


def _one_step(env, body, state, action):
    before = _start(env, state)
    if body == "k1_dynamics":
        env.step_dynamics(action)
    else:
        env.set_step_mode(body)
        assert env.effective_step_mode() == body
        env.step(action)
    torch.cuda.synchronize()
    assert torch.equal(env.read("COUNTERS")[:, 1], before + 1), body
    return env.read("STATE")


# ------------------------------------------------------------------------------------------------ one step, three bodies
@pytest.mark.parametrize("dt", R.DTS, ids=["dt%g" % d for d in R.DTS])
def test_one_step_in_three_bodies_against_the_reference(dt):
    idx, state, action = _rows_of(dt, poisoned=True)
    env = _env(dt, len(state))
    act = _t(action)
    out = {b: _one_step(env, b, state, act) for b in ("k1_dynamics", "side_by_side", "one_launch")}
    assert env.health()["timeouts"] == 0
    env.close()
    for b in ("side_by_side", "one_launch"):
        assert _same(out["k1_dynamics"], out[b]), (b, "rows", _diff_rows(out["k1_dynamics"], out[b]))
    got = _np(out["k1_dynamics"]).T[:len(idx)]
    assert np.isfinite(got).all()
    err = R.errors(got, idx)
    tol = R.tolerances()
    names = R.table()["bounds"][idx]
    limit = np.array([tol[g] for g in names])
    worst = {}
    for g in dict.fromkeys(names.tolist()):
        ratio = (err[names == g] / tol[g]).max(axis=0)
        worst[g] = float(ratio.max())
        print("%-20s largest error / bound per component: %s" % (g, " ".join("%s %.3f" % (c, r) for c, r in zip(R.COMPONENTS, ratio))))
    print("dt %g: closest to the bound: %s at %.3f of it" % (dt, max(worst, key=worst.get), max(worst.values())))
    bad = np.argwhere(err > limit)
    assert len(bad) == 0, [(int(idx[i]), names[i], R.COMPONENTS[c], err[i, c], limit[i, c]) for i, c in bad[:8]]
    assert (got[:, 2] >= -np.pi).all() and (got[:, 2] < np.pi).all()
    if len(state) > len(idx):
        _check_poisoned(_np(out["k1_dynamics"]).T[len(idx):], state[len(idx):], action[len(idx):], dt, tol["ordinary/dt%g" % dt])


def _check_poisoned(got, state, action, dt, tol):
    """`got`: the new states of the poisoned rows and, behind them, of the same rows without the poison.  See the module docstring."""
    k = len(got) // 2
    got, clean, state = got[:k], got[k:], state[:k]
    ora = R.oracle_step(state, action[:k], dt)
    assert np.isfinite(clean).all()
    pinned = np.zeros(got.shape, dtype=bool)                    # u beside a non-finite v or r
    pinned[:, 3] = ~np.isfinite(state[:, 4:6]).all(axis=1) & np.isfinite(state[:, 3])
    assert pinned.sum() >= 4 and np.isnan(ora[pinned]).all()    # (the oracle has NaN there, as the reference)
    assert np.array_equal(got[pinned].view(np.uint64), clean[pinned].view(np.uint64)), (got[pinned], clean[pinned])
    rest = ~pinned
    assert np.array_equal(np.isnan(got) & rest, np.isnan(ora) & rest), np.argwhere((np.isnan(got) != np.isnan(ora)) & rest)
    inf = np.isinf(ora) & rest
    assert np.array_equal(got[inf], ora[inf])
    fin = np.isfinite(ora) & rest
    assert fin.sum() >= 20                                       # (a poisoned x, y or psi leaves most of the row finite)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ora) / np.where(np.arange(6) == 2, 1.0, np.maximum(1.0, np.abs(ora)))
    assert (err[fin] <= np.broadcast_to(tol, err.shape)[fin]).all(), (np.argwhere(fin & (err > tol))[:8], np.nanmax(err[fin]))
    print("poisoned rows: %d values held to the oracle (largest error / bound %.3f), %d NaN as the oracle's, %d u pinned"
          % (fin.sum(), (err / tol)[fin].max(), (np.isnan(ora) & rest).sum(), pinned.sum()))


# ------------------------------------------------------------------------------------------------ action types
@pytest.mark.parametrize("dt", R.DTS, ids=["dt%g" % d for d in R.DTS])
def test_float32_actions_are_their_widened_values_and_nan_rows_the_zero_action(dt):
    _, state, action = _rows_of(dt, group="action")
    with np.errstate(over="ignore"):
        a32 = action.astype(np.float32)
    env = _env(dt, len(state))
    from32 = _one_step(env, "k1_dynamics", state, _t(a32, torch.float32))
    widened = _one_step(env, "k1_dynamics", state, _t(a32.astype(np.float64)))
    exact = _one_step(env, "k1_dynamics", state, _t(action))
    zero = action.copy()
    nan = np.isnan(action).any(axis=1)
    zero[nan] = 0.0
    zeroed = _one_step(env, "k1_dynamics", state, _t(zero))
    env.close()
    assert _same(from32, widened), _diff_rows(from32, widened)
    assert _same(exact, zeroed), _diff_rows(exact, zeroed)
    if dt == 0.5:
        assert nan.sum() >= 3
    # 0.1f is not 0.1: where the CLIPPED action of the float32 row is another number than that of the float64 row, the float32 run
    # is not the float64 run -- in every such row (a row read as its float64 original would be caught)
    def clipped(a):
        with np.errstate(invalid="ignore"):
            return np.stack([np.clip(a[:, 0], 0.0, 1.0), np.clip(a[:, 1], -1.0, 1.0)], axis=1)
    other = (clipped(a32.astype(np.float64)) != clipped(action)).any(axis=1) & ~nan
    assert other.sum() >= {0.5: 4, 1.0: 4, 8.0: 0}[dt], other.sum()
    differs = ~((from32.view(torch.int64) == exact.view(torch.int64)) | (torch.isnan(from32) & torch.isnan(exact))).all(dim=0)
    assert differs[torch.as_tensor(other, device=DEV)].all(), np.flatnonzero(other & ~_np(differs))
    assert not differs[torch.as_tensor(~other, device=DEV)].any()   # (and the same clipped action is the same step)


# ------------------------------------------------------------------------------------------------ neighbours
@pytest.mark.parametrize("body", ["k1_dynamics", "one_launch"])
@pytest.mark.parametrize("batch", range(len(R.NEIGHBOUR_SIZES)), ids=["n%d" % n for n in R.NEIGHBOUR_SIZES])
def test_a_non_finite_state_leaves_its_neighbours_bit_unchanged(batch, body):
    """Eight lanes per environment, eight environments per wave, DPP moves within rows of 16 lanes; the last environment, the one
    idle lane groups clamp to, always holds a NaN or an inf.  n = 1 has no neighbour to compare: that case runs a wave whose eight
    lane groups all compute on the one poisoned environment, and checks that it completes and stays non-finite."""
    b = R.neighbour_batches()[batch]
    env = _env(R.NEIGHBOUR_DT, b["n"])
    act = _t(b["action"])
    clean = _one_step(env, body, b["clean_state"], act)
    dirty = _one_step(env, body, b["state"], act)
    assert env.health()["timeouts"] == 0
    env.close()
    keep = torch.ones(b["n"], dtype=torch.bool, device=DEV)
    keep[torch.as_tensor(b["poisoned"], device=DEV)] = False
    assert torch.isfinite(clean).all()
    assert _same(clean[:, keep], dirty[:, keep]), _diff_rows(clean[:, keep], dirty[:, keep])
    assert not torch.isfinite(dirty[:, ~keep]).all(dim=0).any()    # (the poisoned ones stay non-finite)


# ------------------------------------------------------------------------------------------------ the carry-record body
def _episode_free_cfg(dt):
    """The configuration of the multi-step comparison.  On the empty bank nothing collides, but a written state ends an episode in
    two other ways (k3_nav_reward.hip, reward_apply: done = collision || reached || ... || cum < min_cumulative_reward): the rows
    drawn as the goldens are (x, y in +-1500) project past the end of the bank's 880 m path, progress >= min_path_progress (0.99)
    = reached -- 87 of the 286 rows of dt 0.5; and at dt = 8, where the explicit scheme is unstable, the yaw-rate penalty
    10 |r| takes the return below min_cumulative_reward (-2000) within three steps in 49 of 50 rows.  Both limits are moved out
    of reach here; neither enters the dynamics."""
    from gym_auv_amd.config import effective_reference_config
    cfg = effective_reference_config(use_lidar=True)
    cfg.simulation.t_step_size = dt
    cfg.episode.min_cumulative_reward = -1e300
    cfg.episode.min_path_progress = 2.0                          # (progress is arc length / path length: never above 1 + 2e-6)
    return cfg


def _feedback_open_loop_gains():
    """The gain row that hands the ring's action on (feedback.py: columns 0 .. 6 zero, column 7 one): a_j = 0 + ... + 1 * ring_j."""
    g = np.zeros((2, 8))
    g[:, 7] = 1.0
    return g


@pytest.mark.parametrize("dt", R.DTS, ids=["dt%g" % d for d in R.DTS])
def test_carry_record_body_is_t_one_launch_steps(dt):
    """step_multi (T = 1, 3; both workgroup orders; the action from the ring slot) and step_feedback (T = 1, 3; the action handed
    in by the law, `a_in`) from the written rows against T one-launch steps from the same rows, bit for bit: STATE and the step
    counter.  With T = 3 the second and third step start from the carry record (`have_y`), with a heading that was wrapped there.
    The one-launch steps of the feedback comparison are fed feedback.affine_action of the OBS64 rows, the launch's documented
    equivalent: with the gains above that is the ring's action, except that the law's sum turns a ring action of -0.0 into +0.0
    and that a NaN observation (an environment with a NaN state) makes the action NaN, hence zero.  Rows that end an episode
    within the T steps are left out; they must be fewer than 5 % (see _episode_free_cfg)."""
    from gym_auv_amd.batched_env import BatchedAuvEnv
    from gym_auv_amd.feedback import affine_action
    _, state, action = _rows_of(dt, poisoned=True)
    n = len(state)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = BatchedAuvEnv(_episode_free_cfg(dt), _bank(), n, device=DEV, auto_reset=False)
    env.reset()
    env.set_sub_batches(1, strict=True)                           # one chain, as helpers.shape_run sets the multi-step shapes up
    env.set_step_mode("one_launch")
    assert env.effective_step_mode() == "one_launch"
    act = _t(action)
    ring = act.unsqueeze(0).expand(2, n, 2).contiguous()          # the row's action in every slot
    gains = _feedback_open_loop_gains()
    gains_t = _t(gains)

    def one_launch_steps(T, law):
        before = _start(env, state)
        ended = torch.zeros(n, dtype=torch.bool, device=DEV)
        fed = []
        for _ in range(T):
            a = act
            if law:
                a = _t(affine_action(_np(env.read("OBS64"))[:, :6], gains, action))
            fed.append(_np(a))
            env.step(a)
            torch.cuda.synchronize()
            ended |= env.done.bool()
        assert torch.equal(env.read("COUNTERS")[:, 1], before + T)
        return env.read("STATE").clone(), ended, fed

    def launch(T, order, law):
        before = _start(env, state)
        env.set_multi_order(order)
        torch.cuda.synchronize()
        if law:
            env.step_feedback(gains_t, T, ring=ring, first_slot=1)
        else:
            env.step_multi(ring, 1, T)
        torch.cuda.synchronize()
        assert torch.equal(env.read("COUNTERS")[:, 1], before + T), (T, order, law)
        return env.read("STATE").clone()

    finite_rows = np.isfinite(state).all(axis=1)
    for T in (1, 3):
        for law in (False, True):
            want, ended, fed = one_launch_steps(T, law)
            if law:                                               # the `a_in` route did deliver the ring's action on the finite rows
                for a in fed:
                    assert np.array_equal(a[finite_rows], action[finite_rows], equal_nan=True)
            left_out = int(ended.sum())
            print("dt %g T %d %s: %d of %d rows end an episode" % (dt, T, "feedback" if law else "multi", left_out, n))
            assert left_out < 0.05 * n
            for order in ("cohorts", "steps"):
                got = launch(T, order, law)
                assert _same(want[:, ~ended], got[:, ~ended]), (T, order, law, "rows", _diff_rows(want[:, ~ended], got[:, ~ended]))
    assert env.health()["timeouts"] == 0
    env.close()


# ------------------------------------------------------------------------------------------------ 20 steps across wraps
GROWTH_LIMIT = 1e4


@pytest.mark.parametrize("dt", R.DTS, ids=["dt%g" % d for d in R.DTS])
def test_twenty_steps_across_wraps_against_the_oracle(dt):
    """The wrap rows, 20 steps of the stand-alone kernel against the oracle at the suite's standing bound (1e-9 on psi modulo 2 pi
    and on u, v, r; 1e-9 max(1, |x|) on x, y), and -pi <= psi < pi after every step of every row.

    dt = 8 deviates, and says how.  There the explicit scheme itself is unstable for the sway / yaw pair (the step size times their
    decay rate lies outside RKF45's stability interval -- the reference's own behaviour, odesolver.py:2-47): the oracle's v and r
    are 11 .. 60 after one step, 1e3 after two and 1e17 .. 1e27 after twenty.  (a) u, v and r are scaled like x and y, by
    max(1, |oracle's value|): an absolute 1e-9 on a value of 1e4 would ask for 1e-13 of it.  (b) A row is compared while the
    oracle's |v| and |r| are at most GROWTH_LIMIT = 1e4: the heading of an evaluation is then a sum of the order dt r = 1e5 .. 1e6,
    whose own rounding (2^-53 of it, 1e-10) comes within a tenth of the bound on psi, and past it psi modulo 2 pi, and x and y
    through its sine and cosine, are rounding noise in any float64 code.  Every dt = 8 row is compared for at least two steps; the
    range of psi is checked on all twenty."""
    from gym_auv_amd._capi import make_config
    from gym_auv_amd.config import effective_reference_config
    from oracle.pyoracle import Oracle
    _, state, action = _rows_of(dt, group="wrap")
    cfg = effective_reference_config()
    cfg.simulation.t_step_size = dt
    ora = Oracle(make_config(cfg, auto_reset=False), len(state), _bank())
    ora.reset()
    ora.write("STATE", np.ascontiguousarray(state.T))
    env = _env(dt, len(state))
    _start(env, state)
    act = _t(action)
    worst = 0.0
    compared = np.zeros(len(state), dtype=int)
    live = np.ones(len(state), dtype=bool)
    for t in range(20):
        env.step_dynamics(act)
        ora.step_dynamics(action)
        g, o = _np(env.read("STATE")), ora.read("STATE")
        assert np.isfinite(g).all() and (g[2] >= -np.pi).all() and (g[2] < np.pi).all(), t
        live &= (np.abs(o[4:6]) <= GROWTH_LIMIT).all(axis=0)
        assert dt == 8.0 or live.all()
        compared += live
        d = np.abs(g - o)
        d[2] = np.minimum(d[2], np.abs(R.TWO_PI - d[2]))
        d[:2] /= np.maximum(1.0, np.abs(o[:2]))
        if dt == 8.0:
            d[3:] /= np.maximum(1.0, np.abs(o[3:]))
        d = d[:, live]
        if d.size:
            worst = max(worst, float(d.max()))
        assert (d <= ATOL).all(), (t, np.argwhere(d > ATOL)[:4], float(d.max()))
    assert (compared >= 2).all(), compared
    print("dt %g: largest difference to the oracle %.3e; steps compared per row %d .. %d" % (dt, worst, compared.min(), compared.max()))
    env.close(), ora.close()


