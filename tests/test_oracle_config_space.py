"""The CPU oracle against G7: reference rollouts under non-default configs (oracle/ref_harness/make_golden.py,
gen_config_space), and the checks that make those rollouts worth comparing with -- each moved knob changes the trace,
and the termination knobs end the episode at the recorded step for the recorded cause.  Also: configs that would put NaN
or infinity into the per-handle constants are refused by make_config and auv_create."""
import ctypes as C
import math

import numpy as np
import pytest

from gym_auv_amd._capi import make_config
from gym_auv_amd.config import effective_reference_config
from gym_auv_amd.world import build_world, pack_bank
from gym_auv_amd.worldspec import unpack_world
from helpers import cfg_from_scalars, load
from oracle.pyoracle import Oracle

G7 = "g7_config_space.npz"

# case -> ({knob it moves: what that knob must change}, how the recorded episode ends).  "state" / "obs" / "d": a per-step
# field of the trace (the actions are replayed, so e.g. the look-ahead cannot change the state); "end": with the knob at
# its default the episode does not end at the recorded last step or before.  The end: None (not done), or the cause the
# recorded episode ends for at its last step.
KNOBS = {
    "log_off": ({"sensor_log_transform": "obs"}, None),
    "range60": ({"sensor_range": "d"}, None),
    "range400": ({"sensor_range": "d"}, None),
    "thrust_moment": ({"thrust_max_auv": "state", "moment_max_auv": "state"}, None),
    "width4": ({"vessel_width": "end"}, "collision"),
    "lookahead25": ({"look_ahead_distance": "obs"}, None),
    "lookahead_past_end": ({"look_ahead_distance": "obs"}, None),
    "interval1": ({"sensor_interval_load_obstacles": "d"}, None),
    "interval7": ({"sensor_interval_load_obstacles": "d"}, None),
    "min_cumulative_reward": ({"min_cumulative_reward": "end"}, "min_cumulative_reward"),
    "min_path_progress": ({"min_path_progress": "end"}, "reached_goal"),
    "min_goal_distance": ({"min_goal_distance": "end"}, "reached_goal"),
    "max_timesteps": ({"max_timesteps": "end"}, "max_timesteps"),
    "dt02": ({"dt": "state"}, None),
    "pathfollow_nolidar": ({"dt": "state", "thrust_max_auv": "state", "look_ahead_distance": "obs"}, None),
    "s64_bundle": ({"sensor_range": "d", "sensor_log_transform": "obs", "vessel_width": "end",
                    "sensor_interval_load_obstacles": "d"}, "collision"),
}
SECTION = {"dt": "simulation", "min_goal_distance": "episode", "min_cumulative_reward": "episode",
           "min_path_progress": "episode", "max_timesteps": "episode"}
ATTR = {"dt": "t_step_size"}
FAR = 1e-4           # "far more than the tolerance": the replay tolerances are 1e-8 .. 1e-9


def _names():
    return [str(n) for n in load(G7)["names"]]


@pytest.fixture(scope="module")
def g7():
    return load(G7)


def _set(cfg, knob, value):
    setattr(getattr(cfg, SECTION.get(knob, "vessel")), ATTR.get(knob, knob), value)


def _get(cfg, knob):
    return getattr(getattr(cfg, SECTION.get(knob, "vessel")), ATTR.get(knob, knob))


def replay(z, k, cfg=None):
    """Free-running oracle replay of G7 case k (same world, start and actions) under `cfg` (default: the recorded one).
    Returns per-step arrays up to the recorded length or the replay's first done, whichever comes first."""
    pre = "r%d_" % k
    if cfg is None:
        cfg = cfg_from_scalars(z["cfg_keys"], z[pre + "cfg"])
    o = Oracle(make_config(cfg, rewarder=str(z["rewarder"][k])), 1, pack_bank([build_world(unpack_world(z, pre + "w_"))]))
    obs0 = o.reset()
    st = o.read("STATE")
    st[:, 0] = z[pre + "start_state"]         # teleported runs start elsewhere (nearby cache kept)
    o.write("STATE", st)
    rec = {key: [] for key in ("state", "obs", "reward", "done", "info", "d", "movers")}
    for t in range(len(z[pre + "reward"])):
        obs, rew, done = o.step(z[pre + "action"][t][None])
        rec["state"].append(o.read("STATE")[:, 0].copy())
        rec["obs"].append(obs[0].copy())
        rec["reward"].append(float(rew[0]))
        rec["done"].append(bool(done[0]))
        rec["info"].append(o.read("INFO64")[0].copy())
        rec["d"].append(o.read("LIDAR_D")[0].copy())
        rec["movers"].append(o.read("MOVER_STATE")[0].copy())
        if done[0]:
            break
    o.close()
    return obs0[0], {key: np.array(v) for key, v in rec.items()}


@pytest.mark.parametrize("k", range(16), ids=_names())
def test_g7_rollout_free_running(g7, k):
    """test_oracle_golden.test_rollout_free_running's tolerances, under the case's config."""
    z = g7
    pre = "r%d_" % k
    cfg = cfg_from_scalars(z["cfg_keys"], z[pre + "cfg"])
    D = 6 + (cfg.vessel.n_sensors if cfg.vessel.use_lidar else 0)
    obs0, rec = replay(z, k, cfg)
    np.testing.assert_allclose(obs0[:D], z[pre + "obs0"], rtol=0, atol=1e-12)
    T = len(z[pre + "reward"])
    assert len(rec["reward"]) == T                                    # no early done
    for t in range(T):
        gi, info = z[pre + "info"][t], rec["info"][t]
        np.testing.assert_allclose(rec["state"][t], z[pre + "state"][t], rtol=0, atol=1e-9, err_msg="state step %d" % t)
        np.testing.assert_allclose(rec["obs"][t, :D], z[pre + "obs"][t], rtol=0, atol=1e-9, err_msg="obs step %d" % t)
        assert rec["reward"][t] == pytest.approx(z[pre + "reward"][t], abs=1e-8), t
        assert rec["done"][t] == bool(z[pre + "done"][t]), t
        assert info[0] == gi[0] and info[1] == gi[1], t                 # collision, reached_goal
        np.testing.assert_allclose(info[2:6], gi[2:6], rtol=0, atol=1e-8, err_msg="info step %d" % t)
        if cfg.vessel.use_lidar:
            np.testing.assert_allclose(rec["d"][t], z[pre + "d"][t], rtol=0, atol=1e-8, err_msg="d step %d" % t)
        mv = z[pre + "movers"][t]
        if mv.size:
            np.testing.assert_allclose(rec["movers"][t, :len(mv)], mv, rtol=0, atol=1e-8, err_msg="movers step %d" % t)


def test_g7_cases_and_recorded_configs(g7):
    """Every case is in KNOBS; its recorded config has exactly its knobs off the defaults (and n_sectors x
    n_sensors_per_sector / use_lidar where the case says so)."""
    z = g7
    assert _names() == list(KNOBS)
    assert list(z["cfg_keys"][:12]) == list(load("g5_rollouts.npz")["cfg_keys"])
    base = effective_reference_config(use_lidar=True)
    for k, name in enumerate(_names()):
        cfg = cfg_from_scalars(z["cfg_keys"], z["r%d_cfg" % k])
        moved = [kn for kn in ("dt", "min_goal_distance", "max_timesteps", "min_cumulative_reward", "min_path_progress",
                               "sensor_range", "vessel_width", "look_ahead_distance", "sensor_interval_load_obstacles",
                               "thrust_max_auv", "moment_max_auv", "sensor_log_transform", "feasibility_width_multiplier")
                 if _get(cfg, kn) != _get(base, kn)]
        assert set(moved) == set(KNOBS[name][0]), (name, moved)
        assert cfg.vessel.use_lidar == (name != "pathfollow_nolidar")
        assert cfg.vessel.n_sensors == (64 if name == "s64_bundle" else 180)


def _default_of(knob):
    return _get(effective_reference_config(use_lidar=True), knob)


def _cause(info_row, t, cfg):
    """Why an episode that is done at step index t ended (environment.py:375-384)."""
    if info_row[0]:
        return "collision"
    if info_row[1]:
        return "reached_goal"
    if t >= cfg.episode.max_timesteps - 1:
        return "max_timesteps"
    assert info_row[4] < cfg.episode.min_cumulative_reward
    return "min_cumulative_reward"


@pytest.mark.parametrize("k", range(16), ids=_names())
def test_g7_each_knob_changes_the_result(g7, k):
    """Replayed with one of the case's knobs back at its default, the trace differs from G7 far beyond the replay
    tolerances; a termination case ends at its recorded last step for the cause it was built for, and does not end there
    (or before) at the default."""
    z = g7
    pre = "r%d_" % k
    name = _names()[k]
    knobs, end = KNOBS[name]
    cfg = cfg_from_scalars(z["cfg_keys"], z[pre + "cfg"])
    T = len(z[pre + "reward"])
    assert not z[pre + "done"][:-1].any() and bool(z[pre + "done"][-1]) == (end is not None)
    if end is not None:
        assert _cause(z[pre + "info"][-1], T - 1, cfg) == end, name
        gi = z[pre + "info"][-1]
        if name == "min_goal_distance":
            assert gi[2] <= cfg.episode.min_goal_distance and gi[3] < 0.99
        elif name == "min_path_progress":
            assert gi[3] >= cfg.episode.min_path_progress and gi[2] > 0.1
        elif end == "collision":
            assert _get(cfg, "vessel_width") > z[pre + "d"][-1].min() >= _default_of("vessel_width")
        elif end == "min_cumulative_reward":
            assert T - 1 < cfg.episode.max_timesteps - 1
    for knob, what in knobs.items():
        other = cfg.copy()
        _set(other, knob, _default_of(knob))
        assert _get(other, knob) != _get(cfg, knob)
        _, rec = replay(z, k, other)
        n = len(rec["reward"])
        if what == "end":
            assert n == T and not rec["done"].any(), (name, knob, n)
        else:
            ref = z[pre + what][:n]
            got = rec[what][:, :ref.shape[1]]
            assert np.abs(got - ref).max() > FAR, (name, knob)


# ----------------------------------------------------------------------------------- configs that are refused
def _bad_configs():
    out = []
    for knob in ("dt", "sensor_range"):
        for v in (0.0, -1.0, math.inf, math.nan):
            out.append((knob, v))
    for knob in ("vessel_width", "thrust_max_auv", "moment_max_auv", "look_ahead_distance"):
        for v in (math.inf, -math.inf, math.nan):
            out.append((knob, v))
    return out


@pytest.mark.parametrize("knob,value", _bad_configs(), ids=["%s=%r" % kv for kv in _bad_configs()])
def test_non_finite_configs_are_refused(knob, value):
    """make_config raises ValueError; auv_create (through the C ABI, before any device call) returns AUV_EINVAL with a
    message naming the knob."""
    from gym_auv_amd import _capi
    cfg = effective_reference_config(use_lidar=True)
    _set(cfg, knob, value)
    with pytest.raises(ValueError, match=knob if knob != "dt" else "t_step_size|dt"):
        make_config(cfg)
    good = make_config(effective_reference_config(use_lidar=True))
    field = {"dt": "dt", "thrust_max_auv": "thrust_max", "moment_max_auv": "moment_max"}.get(knob, knob)
    setattr(good, field, value)
    lib = _capi.load_library()
    h = C.c_void_p()
    assert lib.auv_create(C.byref(good), 8, 0, C.byref(h)) == -1          # AUV_EINVAL
    assert not h.value
    msg = lib.auv_last_error()
    msg = msg.decode() if isinstance(msg, bytes) else str(msg)
    assert field in msg, msg
