"""Shared test helpers: golden loading, config reconstruction, world construction."""
import os

import numpy as np

from gym_auv_amd.config import Config
from gym_auv_amd.worldspec import MoverSpec, WorldSpec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    return np.load(os.path.join(GOLDEN, name))


def cfg_from_scalars(keys, vals) -> Config:
    cs = dict(zip([str(k) for k in keys], vals))
    cfg = Config()
    cfg.simulation.t_step_size = float(cs["dt"])
    cfg.episode.min_goal_distance = float(cs["min_goal_distance"])
    cfg.episode.max_timesteps = int(cs["max_timesteps"])
    cfg.episode.min_cumulative_reward = float(cs["min_cumulative_reward"])
    cfg.episode.min_path_progress = float(cs["min_path_progress"])
    cfg.vessel.use_lidar = bool(cs["use_lidar"])
    cfg.vessel.n_sectors = int(cs["n_sectors"])
    cfg.vessel.n_sensors_per_sector = int(cs["n_sensors_per_sector"])
    cfg.vessel.sensor_range = float(cs["sensor_range"])
    cfg.vessel.vessel_width = float(cs["vessel_width"])
    cfg.vessel.look_ahead_distance = int(cs["look_ahead_distance"])
    cfg.vessel.sensor_interval_load_obstacles = int(cs["sensor_interval_load_obstacles"])
    # recorded by G7 only: absent keys keep the defaults
    if "thrust_max_auv" in cs:
        cfg.vessel.thrust_max_auv = float(cs["thrust_max_auv"])
    if "moment_max_auv" in cs:
        cfg.vessel.moment_max_auv = float(cs["moment_max_auv"])
    if "sensor_log_transform" in cs:
        cfg.vessel.sensor_log_transform = bool(cs["sensor_log_transform"])
    if "feasibility_width_multiplier" in cs:
        cfg.vessel.feasibility_width_multiplier = float(cs["feasibility_width_multiplier"])
    return cfg


def scene_world(z, i) -> WorldSpec:
    """G3 scene i -> WorldSpec (dummy straight path; movers frozen in their recorded pose).
    Obstacle order in the built world is circles, polygons, movers; `scene_order` maps the
    reference's obstacle list onto it."""
    pre = "s%d_" % i
    off = z[pre + "poly_off"]
    pts = z[pre + "poly_pts"]
    polys = [pts[off[j]:off[j + 1]] for j in range(len(off) - 1)]
    movers = [MoverSpec(width=float(m[0]), pos0=m[1:3].copy(), vel=np.array([[1.0, 0.0]]), n_vel=9999,
                        pos=m[1:3].copy(), heading=float(m[3]), counter=0.0) for m in z[pre + "movers_now"]]
    return WorldSpec(waypoints=np.array([[0.0, 1000.0], [0.0, 0.0]]), vessel_init=z[pre + "pose"].copy(),
                     circles=z[pre + "circles"], polygons=polys, movers=movers, name=str(z["names"][i]))


def scene_order(z, i):
    """index in the built world's obstacle list for each reference obstacle of scene i."""
    pre = "s%d_" % i
    order = z[pre + "order"]
    nc = len(z[pre + "circles"])
    npoly = len(z[pre + "poly_off"]) - 1
    base = {0: 0, 1: nc, 2: nc + npoly}
    return np.array([base[int(k)] + int(j) for k, j in order], dtype=np.int64)


def shape_run(shape_name, cfg, bank, n, ring, steps, fields=(), lengths=(1, 6, 16, 64), **kw):
    """-m gpu: (obs, *fields read, reward, done) after every step (multi-step launches: after every launch) of one step
    shape; auto-reset on, actions ring[t % slots].  lengths: steps per launch of the multi-step shapes, cycled through.
    kw: further BatchedAuvEnv arguments (rewarder, cull)."""
    import warnings

    import torch
    from gym_auv_amd.batched_env import BatchedAuvEnv
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = BatchedAuvEnv(cfg, bank, n, device="cuda:0", auto_reset=True, **kw)
    env.reset()
    out = {}
    if shape_name == "side_by_side":
        env.set_step_mode("side_by_side")
    if shape_name in ("chains", "async") or shape_name.startswith("multi"):
        env.set_sub_batches(1 if shape_name.startswith("multi") else 4, strict=shape_name.startswith("multi"))
    if shape_name == "multi_steps":
        env.set_multi_order("steps")
    if shape_name == "graph":
        env.capture_graph(steps=1)

    def snap(t):
        torch.cuda.synchronize()
        out[t] = (env.obs.clone(),) + tuple(env.read(f) for f in fields) + (env.reward.clone(), env.done.clone())

    slots = ring.shape[0]
    if shape_name.startswith("multi"):
        t = 0
        while t < steps:
            T = min(lengths[len(out) % len(lengths)], steps - t)
            env.step_multi(ring, t % slots, T)
            t += T
            snap(t)
    else:
        for t in range(steps):
            a = ring[t % slots]
            if shape_name == "one_launch" or shape_name == "side_by_side":
                env.step(a)
            elif shape_name == "chains":
                env.step_pipelined(a)
            elif shape_name == "async":
                env.step_async(a)
                env.step_wait()
            elif shape_name == "graph":
                env.step_graph(a)
            snap(t + 1)
    env.close()
    return out
