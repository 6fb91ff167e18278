"""-m gpu: the HIP path under non-default configs.

The kernels get the config by three routes -- AuvDev::cfg by value, per-handle constants that k_derive computes from it,
and the finish roles' hand-written copy into StepTabs::cfg -- and at the default config a knob lost on any of them can
go unnoticed.  So: the G7 reference rollouts (one knob moved per case) through the C ABI; every G7 knob set batched
against the oracle with auto-reset; every step shape bit for bit against the one-launch shape under every knob set (the
comparison that catches a bad StepTabs copy); pooled observations under a non-default range / linear closeness /
opening width; and device-generated fresh worlds under a non-default width and dt."""
import numpy as np
import pytest
import torch

from gym_auv_amd._capi import make_config
from gym_auv_amd.config import effective_reference_config
from gym_auv_amd.scenarios import moving_obstacles_world, polygon_world, static_circles_world
from gym_auv_amd.world import build_world, pack_bank
from gym_auv_amd.worldspec import unpack_world
from helpers import cfg_from_scalars, load, shape_run

pytestmark = pytest.mark.gpu
G7 = "g7_config_space.npz"
FIELDS_F = ("STATE", "LIDAR_D", "OBS64", "REWARD64", "INFO64", "NAV64", "MOVER_STATE")
FIELDS_I = ("NEARBY", "COLLISION", "CULL_LIMITS", "WORLD_IDX")
# G7 case -> the termination its knob controls (how a batched episode that it ends shows in the EPISODE row)
CAUSE = {"width4": "collision", "s64_bundle": "collision", "min_cumulative_reward": "return",
         "min_path_progress": "goal", "min_goal_distance": "goal", "max_timesteps": "length"}


def _np(t):
    return t.detach().cpu().numpy()


def _env(cfg, bank, n, **kw):
    import warnings
    from gym_auv_amd.batched_env import BatchedAuvEnv
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return BatchedAuvEnv(cfg, bank, n, device="cuda:0", **kw)


def _names():
    return [str(n) for n in load(G7)["names"]]


def _knob_sets():
    """(id, cfg, rewarder, cull) of every G7 case, and cull="exact" at sensor_range 400."""
    z = load(G7)
    out = [(str(name), cfg_from_scalars(z["cfg_keys"], z["r%d_cfg" % k]), str(z["rewarder"][k]), "reference")
           for k, name in enumerate(z["names"])]
    r400 = [c for c in out if c[0] == "range400"][0][1]
    out.append(("range400_exact", r400.copy(), "colav", "exact"))
    return out


KNOB_SETS = _knob_sets()
KNOB_IDS = [c[0] for c in KNOB_SETS]


# ------------------------------------------------------------------------------- G7 through the C ABI
@pytest.mark.parametrize("mode", ["one_launch", "side_by_side"])
@pytest.mark.parametrize("k", range(16), ids=_names())
def test_g7_rollout_vs_reference(k, mode):
    """test_gpu_parity.test_rollout_vs_reference_golden's tolerances, one env per G7 case."""
    z = load(G7)
    pre = "r%d_" % k
    cfg = cfg_from_scalars(z["cfg_keys"], z[pre + "cfg"])
    env = _env(cfg, pack_bank([build_world(unpack_world(z, pre + "w_"))]), 1, rewarder=str(z["rewarder"][k]),
               auto_reset=False)
    env.set_step_mode(mode)
    D = env.obs_dim
    assert D == 6 + (cfg.vessel.n_sensors if cfg.vessel.use_lidar else 0)
    obs0 = _np(env.reset())
    np.testing.assert_allclose(_np(env.read("OBS64"))[0, :D], z[pre + "obs0"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(obs0[0], z[pre + "obs0"], rtol=0, atol=1e-7)
    st = _np(env.read("STATE"))
    st[:, 0] = z[pre + "start_state"]
    env.write("STATE", st)
    for t in range(len(z[pre + "reward"])):
        obs, rew, done, _ = env.step(torch.as_tensor(z[pre + "action"][t][None], device="cuda:0"))
        info = _np(env.read("INFO64"))[0]
        gi = z[pre + "info"][t]
        np.testing.assert_allclose(_np(env.read("STATE"))[:, 0], z[pre + "state"][t], rtol=0, atol=1e-9, err_msg="step %d" % t)
        np.testing.assert_allclose(_np(env.read("OBS64"))[0, :D], z[pre + "obs"][t], rtol=0, atol=1e-9, err_msg="step %d" % t)
        np.testing.assert_allclose(_np(obs)[0], z[pre + "obs"][t], rtol=0, atol=1e-5)
        assert _np(env.read("REWARD64"))[0] == pytest.approx(z[pre + "reward"][t], abs=1e-8), t
        assert bool(_np(done)[0]) == bool(z[pre + "done"][t]), t
        assert info[0] == gi[0] and info[1] == gi[1], t
        np.testing.assert_allclose(info[2:6], gi[2:6], rtol=0, atol=1e-8, err_msg="step %d" % t)
        if cfg.vessel.use_lidar:
            np.testing.assert_allclose(_np(env.read("LIDAR_D"))[0], z[pre + "d"][t], rtol=0, atol=1e-8, err_msg="step %d" % t)
        mv = z[pre + "movers"][t]
        if mv.size:
            np.testing.assert_allclose(_np(env.read("MOVER_STATE"))[0, :len(mv)], mv, rtol=0, atol=1e-8)
    env.close()


# ------------------------------------------------------------------------------- batched against the oracle
def _mixed_specs(n):
    specs = []
    for i in range(n):
        if i % 3 == 0:
            specs.append(moving_obstacles_world(1000 + i))
        elif i % 3 == 1:
            specs.append(static_circles_world(1000 + i, 20))
        else:
            specs.append(polygon_world(1000 + i, 12, n_circles=4, n_moving=3))
    return specs


def _poses(worlds, world_idx, state, rs):
    """Starts that drive the terminations, by env group i % 5: 0 -- 9 m from the circle nearest the reset pose, heading
    at it; on the path, heading along it: 1 -- at 3 % of its length (min_path_progress 0.05), 2 -- 170 m before its end
    (min_goal_distance 150), 3 -- at 98.5 % (the default progress bound); 4 -- where the reset put them."""
    st = state.copy()
    for i, w in enumerate(world_idx):
        bw = worlds[int(w)]
        path, L = bw.path, bw.path.length
        if i % 5 == 0 and len(bw.spec.circles):
            c = bw.spec.circles[np.argmin(np.hypot(*(bw.spec.circles[:, :2] - st[:2, i]).T) - bw.spec.circles[:, 2])]
            ang = rs.uniform(-np.pi, np.pi)
            p = c[:2] + (c[2] + 9.0) * np.array([np.cos(ang), np.sin(ang)])
            st[:, i] = [p[0], p[1], np.arctan2(np.sin(ang + np.pi), np.cos(ang + np.pi)), 0.4, 0.0, 0.0]
        elif i % 5 in (1, 2, 3):
            s0 = {1: 0.03 * L, 2: max(L - 170.0, 0.5 * L), 3: 0.985 * L}[i % 5]
            p = path(s0)
            st[:, i] = [p[0], p[1], path.get_direction(s0), 0.5, 0.0, 0.0]
    return st


@pytest.fixture(scope="module")
def mixed():
    specs = _mixed_specs(48)
    worlds = [build_world(s) for s in specs]
    return worlds, pack_bank(worlds)


BATCHED = [(launch,) + c for launch in ("one_step", "multi") for c in KNOB_SETS if launch == "one_step" or c[1].vessel.use_lidar]


@pytest.mark.parametrize("launch,name,cfg,rewarder,cull", BATCHED, ids=["%s-%s" % (b[0], b[1]) for b in BATCHED])
def test_batched_vs_oracle_with_auto_reset(mixed, launch, name, cfg, rewarder, cull):
    """1024 envs over 48 mixed worlds, 60 steps, auto-reset: every fp64 field at 1e-9, integer fields and done bit for
    bit, after every launch -- one step per launch, or (LiDAR on) launches of 1, 5 and 3 steps (auv_step_multi, whose
    finish role keeps its own copy of the config); episodes turn over, by the knob's own termination where the knob is
    one."""
    from oracle.pyoracle import Oracle
    worlds, bank = mixed
    n, steps = 1024, 60
    env = _env(cfg, bank, n, rewarder=rewarder, cull=cull, auto_reset=True)
    ora = Oracle(make_config(cfg, rewarder=rewarder, cull=cull, auto_reset=True), n, bank)
    np.testing.assert_allclose(_np(env.reset()), ora.reset()[:, :env.obs_dim], rtol=0, atol=1e-6)
    rs = np.random.RandomState(len(name))
    st = _poses(worlds, ora.read("WORLD_IDX"), ora.read("STATE"), rs)
    env.write("STATE", st), ora.write("STATE", st)
    acts = rs.uniform([0, -0.15], [1, 0.15], (steps, n, 2))
    acts[:, np.arange(n) % 5 != 4] = [1.0, 0.0]
    ring = torch.as_tensor(acts, device="cuda:0").contiguous()
    if launch == "multi":
        env.set_sub_batches(1, strict=True)
    causes = {"collision": 0, "goal": 0, "goal_default": 0, "return": 0, "length": 0}
    first = np.ones(n, dtype=bool)                  # (the group's start only holds for an env's first episode)
    t = 0
    while t < steps:
        T = 1 if launch == "one_step" else min((1, 5, 3)[t % 3], steps - t)
        if launch == "one_step":
            obs, rew, done, _ = env.step(ring[t])
        else:
            env.step_multi(ring, t, T)
            torch.cuda.synchronize()
            obs, done = env.obs, env.done
        for k in range(t, t + T):
            o_obs, o_rew, o_done = ora.step(acts[k])
            ep = ora.read("EPISODE")
            for e in np.flatnonzero(o_done):
                ret, _, col, goal = ep[e]
                if goal:       # reached from the start that the goal knobs are tuned for, or from the 98.5 % start
                    causes["goal" if first[e] and e % 5 in (1, 2) else "goal_default"] += 1
                else:
                    causes["collision" if col else "return" if ret < cfg.episode.min_cumulative_reward else "length"] += 1
                first[e] = False
        t += T
        np.testing.assert_array_equal(_np(done), o_done, err_msg="done step %d" % t)
        for f in FIELDS_F + ("EPISODE",):
            np.testing.assert_allclose(_np(env.read(f)), ora.read(f), rtol=0, atol=1e-9, err_msg="%s step %d" % (f, t))
        for f in FIELDS_I:
            np.testing.assert_array_equal(_np(env.read(f)), ora.read(f), err_msg="%s step %d" % (f, t))
        np.testing.assert_array_equal(_np(env.read("COUNTERS"))[:, :3], ora.read("COUNTERS")[:, :3], err_msg="step %d" % t)
        np.testing.assert_allclose(_np(obs), o_obs[:, :env.obs_dim], rtol=0, atol=1e-6)
    env.close()
    assert sum(causes.values()) >= 1, causes
    if name in CAUSE:
        assert causes[CAUSE[name]] >= 1, (name, causes)


# ------------------------------------------------------------------------------- every step shape, bitwise
@pytest.mark.parametrize("name,cfg,rewarder,cull", KNOB_SETS, ids=KNOB_IDS)
def test_every_step_shape_bitwise_under_the_knobs(mixed, name, cfg, rewarder, cull):
    """side_by_side, chains, async, graph, multi_cohorts and multi_steps == one_launch, bit for bit: obs, reward, done,
    STATE, LIDAR_D, INFO64 after every step (launch); with the LiDAR off the multi-step shapes are refused.  n = 1024 (ne % 64 == 0: the cohort order is taken).  Episodes
    are cut at 29 steps (40 for the max_timesteps case itself) so that auto-resets fall inside the compared stretch."""
    _, bank = mixed
    n, steps = 1024, 64
    cfg = cfg.copy()
    cfg.episode.max_timesteps = min(cfg.episode.max_timesteps, 29 if name != "max_timesteps" else 40)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(11)
    ring = (torch.rand((steps, n, 2), generator=g, device="cuda:0") * torch.tensor([1.0, 0.3], device="cuda:0")
            - torch.tensor([0.0, 0.15], device="cuda:0")).contiguous()
    fields = ("STATE", "LIDAR_D", "INFO64")
    kw = dict(rewarder=rewarder, cull=cull, fields=fields)
    ref = shape_run("one_launch", cfg, bank, n, ring, steps, **kw)
    assert sum(int(v[-1].sum()) for v in ref.values()) > 0            # auto-resets inside the compared stretch
    shapes = ("side_by_side", "chains", "async", "graph", "multi_cohorts", "multi_steps")
    if not cfg.vessel.use_lidar:
        # no one-launch shape without the LiDAR, and so no multi-step launch: refused, not run some other way
        with pytest.raises(RuntimeError, match="one-launch"):
            shape_run("multi_steps", cfg, bank, n, ring, steps, **kw)
        shapes = shapes[:4]
    for shape_name in shapes:
        got = shape_run(shape_name, cfg, bank, n, ring, steps, **kw)
        assert len(got) > 0
        for t, v in got.items():
            for j, (a, b) in enumerate(zip(ref[t], v)):
                assert torch.equal(a, b), (name, shape_name, t, (("obs",) + fields + ("reward", "done"))[j])


# ------------------------------------------------------------------------------- pooled observation with the knobs
def _pooled_cfg():
    from test_gpu_pooled_obs import _cfg
    cfg = _cfg(9, 20, pooled=True, velocity=True, max_timesteps=23)
    cfg.vessel.sensor_log_transform = False
    cfg.vessel.sensor_range = 60.0
    cfg.vessel.feasibility_width_multiplier = 2.0
    return cfg


@pytest.mark.parametrize("shape_name", ["one_launch", "multi_steps"])
def test_pooled_observation_under_the_knobs(shape_name):
    """test_gpu_pooled_obs._check_row (closeness from this config's range, linear) after every step / launch, and the
    k4_pooling post-kernel on the same ranges: distances bit for bit, closeness within float32 rounding."""
    from test_gpu_pooled_obs import _bank, _check_row, _closeness, _Pool
    cfg = _pooled_cfg()
    n, steps = 256, 60
    bank = _bank("moving28", 32)
    env = _env(cfg, bank, n, auto_reset=True)
    pool = _Pool(cfg, n, bank)
    assert pool.width == pytest.approx(1.255 * 2.0)
    env.reset()
    _check_row(env, pool, 9, 3)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(3)
    ring = (torch.rand((steps, n, 2), generator=g, device="cuda:0") * torch.tensor([2.0, 0.3], device="cuda:0")
            - torch.tensor([1.0, 0.15], device="cuda:0")).contiguous()
    if shape_name == "multi_steps":
        env.set_sub_batches(1, strict=True)
        env.set_multi_order("steps")
    t, near = 0, 0
    while t < steps:
        T = 1 if shape_name == "one_launch" else min((1, 6, 16)[t % 3], steps - t)
        if shape_name == "one_launch":
            env.step(ring[t])
        else:
            env.step_multi(ring, t, T)
        t += T
        torch.cuda.synchronize()
        sd = _check_row(env, pool, 9, 3)
        dist, clos = env.feasibility_pooling()
        np.testing.assert_array_equal(_np(dist), sd)
        assert np.abs(_np(clos) - _closeness(sd, cfg)).max() <= 1e-6
        near += int((sd < 60.0).sum())
    assert (sd <= 60.0).all() and near > 0
    assert int(env.read("COUNTERS")[:, 2].sum()) > 0              # episodes ended (inside the launches too)
    env.close()


# ------------------------------------------------------------------------------- fresh worlds
def test_fresh_worlds_under_width_and_dt():
    """vessel_width 2.5 and dt 0.2 reach the generator (the mover tables and the start clearance depend on them): slots,
    initial and regenerated, equal the host builder's under this config, and a rollout equals the never-repeating bank
    bit for bit."""
    from gym_auv_amd.devgen import FreshWorlds, GeneratedWorlds
    from test_gpu_fresh import BITWISE, _check_slots_against_host
    cfg = effective_reference_config(use_lidar=True)
    cfg.vessel.n_sectors, cfg.vessel.n_sensors_per_sector = 4, 8
    cfg.vessel.vessel_width, cfg.simulation.t_step_size = 2.5, 0.2
    cfg.episode.max_timesteps = 7
    n, steps = 64, 60
    spec = FreshWorlds(depth=2, seed=31, period=1, batch_cap=64)
    fresh = _env(cfg, spec, n, auto_reset=True)
    _check_slots_against_host(cfg, spec, fresh, n)
    n_serial = steps // 7 + 3
    rows = fresh.fresh_draws([i % n for i in range(n * n_serial)], [i // n for i in range(n * n_serial)])
    big = _env(cfg, GeneratedWorlds(n * n_serial, seed=0), n, auto_reset=True)
    big.generate(GeneratedWorlds(n * n_serial, seed=0), draws=rows)
    assert torch.equal(fresh.reset(), big.reset())
    g = torch.Generator(device="cuda:0")
    g.manual_seed(6)
    for t in range(steps):
        a = torch.rand((n, 2), generator=g, device="cuda:0") * torch.tensor([2.0, 0.3], device="cuda:0") - torch.tensor([1.0, 0.15], device="cuda:0")
        o0, r0, d0, _ = big.step(a)
        o1, r1, d1, _ = fresh.step(a)
        torch.cuda.synchronize()
        assert torch.equal(o0, o1) and torch.equal(r0, r1) and torch.equal(d0, d1), t
        if t % 5 == 4:
            for f in BITWISE:
                assert torch.equal(big.read(f), fresh.read(f)), (t, f)
    assert int(big.read("COUNTERS")[:, 2].sum()) >= (steps // 7) * n
    fresh.refill(flush=True)
    assert fresh.fresh_stats()["reused"] == 0
    s1 = _check_slots_against_host(cfg, spec, fresh, n)           # the regenerated slots too
    assert s1.max() >= 3
    big.close(), fresh.close()
