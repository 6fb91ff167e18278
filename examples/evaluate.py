#!/usr/bin/env python3
"""Closed-loop evaluation of a policy, batched: the reference's `enjoy` / `test` loop -- agent.predict(obs, deterministic=True), then
env.step (scripts/run.py:175, 273, 567) -- for N environments at once.  Per step ONE launch evaluates the actor
(FusedActorCritic.predict writes the deterministic action straight into the action buffer) and the environment steps; episodes that end
are auto-reset into the next world of the bank, and the episode log says how they ended.

    python examples/evaluate.py --envs 256 --episodes 4                    # a freshly initialised policy
    python examples/evaluate.py --ckpt policy.pt --task pathfollow          # a state_dict of examples/ppo.py's ActorCritic
    python examples/evaluate.py --envs 64 --frames out/                     # and pictures of the first 16 environments
    python examples/evaluate.py --ckpt policy.pt --frame-stack 4            # a policy trained with examples/ppo.py --frames 4
    python examples/evaluate.py --ckpt policy.pt --squash 1                 # a policy trained with examples/ppo.py --squash 1
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gym_auv_amd import scenarios  # noqa: E402
from gym_auv_amd.batched_env import BatchedAuvEnv  # noqa: E402
from gym_auv_amd.config import effective_reference_config  # noqa: E402
from gym_auv_amd.policy import FusedActorCritic  # noqa: E402
from gym_auv_amd.world import build_world, pack_bank  # noqa: E402


def load_policy(ckpt, obs_dim, device, seed=0, hidden=(256, 128, 64)):
    """examples/ppo.py's ActorCritic, initialised (ckpt None) or with a state_dict loaded (a file holding the state_dict itself or a
    dict with it under "model")."""
    import ppo
    torch.manual_seed(seed)
    net = ppo.ActorCritic(obs_dim, hidden=tuple(hidden)).to(device)
    if ckpt:
        sd = torch.load(ckpt, map_location=device)
        net.load_state_dict(sd["model"] if isinstance(sd, dict) and "model" in sd else sd)
    return net.eval()


def save_frames(env, frames_dir, step, n_frames=16):
    """Frames of the first `n_frames` environments, drawn on the device (BatchedAuvEnv.render): the stack as
    frames_<step>.npy [B, H, W, 3] and, tiled into one picture, frames_<step>.ppm (a binary PPM: any viewer opens it)."""
    from gym_auv_amd.render import tile_frames, write_ppm
    frames = env.render(envs=list(range(min(env.n_envs, n_frames)))).cpu().numpy()
    np.save(os.path.join(frames_dir, "frames_%06d.npy" % step), frames)
    write_ppm(os.path.join(frames_dir, "frames_%06d.ppm" % step), tile_frames(frames))


def evaluate(env, fused, episodes, max_steps=100000, frames_dir=None):
    """Step until every environment has finished `episodes` episodes (or max_steps): returns the episode-log rows [k, 8] (float64,
    BatchedAuvEnv.EPISODE_LOG_COLUMNS) of the first `episodes` episodes of every environment, and the number of steps taken.
    frames_dir: a picture of the first environments every 50 steps (save_frames)."""
    env.episode_log()                                      # (drop whatever ended before)
    rows, steps = [], 0
    count = torch.zeros(env.n_envs, dtype=torch.int64, device=env.device)
    while steps < max_steps:
        for _ in range(50):                                # one read-back every 50 steps
            if fused.frames > 1:                           # frame stacking: the history moves on with every step (FrameStack.push)
                fused.predict(fused.stack.push(env.obs, env.done))
            else:
                fused.predict()                            # -> fused.actions
            env.step(fused.actions)
        steps += 50
        if frames_dir:
            save_frames(env, frames_dir, steps)
        log = env.episode_log()
        if log.shape[0]:
            rows.append(log)
            count += torch.bincount(log[:, 0].long(), minlength=env.n_envs)
        if int(count.min()) >= episodes:
            break
    log = torch.cat(rows) if rows else torch.zeros((0, 8), dtype=torch.float64, device=env.device)
    if log.shape[0]:
        # the first `episodes` episodes of every environment, in completion order
        e = log[:, 0].long()
        order = torch.argsort(e, stable=True)
        rank = torch.empty_like(e)
        se = e[order]
        first = torch.searchsorted(se, se)
        rank[order] = torch.arange(e.numel(), device=e.device) - first
        log = log[rank < episodes]
    return log, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", default=None, help="state_dict of examples/ppo.py's ActorCritic (default: a freshly initialised policy)")
    ap.add_argument("--task", default="colav", choices=["colav", "pathfollow"])
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--episodes", type=int, default=2, help="episodes per environment")
    ap.add_argument("--worlds", type=int, default=0, help="worlds of the bank (default: 2 per environment)")
    ap.add_argument("--feasibility-pooling", type=int, default=0)
    ap.add_argument("--act-space", default="raw", choices=["raw", "normalized"])
    ap.add_argument("--squash", type=int, default=0, choices=[0, 1],
                    help="1: the checkpoint is a tanh-squashed policy (examples/ppo.py --squash 1): action = mid + half * tanh(mu); implies "
                         "--act-space normalized")
    ap.add_argument("--max-steps", type=int, default=100000, help="stop after this many steps even if episodes are still open")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--frames", default=None, metavar="DIR", help="write frames of the first 16 environments every 50 steps: .npy stacks and .ppm pictures")
    ap.add_argument("--frame-stack", type=int, default=1, metavar="K",
                    help="the policy sees the last K observations as one row (examples/ppo.py --frames K; here --frames is the picture directory)")
    ap.add_argument("--net-arch", default="256,128,64", metavar="H1,H2,H3",
                    help="hidden widths of the checkpoint's nets (examples/ppo.py --net-arch): one of gym_auv_amd.policy.SUPPORTED_HIDDEN")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    colav = a.task == "colav"
    cfg = effective_reference_config(use_lidar=colav)
    cfg.vessel.sensor_use_feasibility_pooling = bool(a.feasibility_pooling)
    n_worlds = a.worlds or 2 * a.envs
    bank = pack_bank([build_world(scenarios.moving_obstacles_world(a.seed + i) if colav else scenarios.moving_obstacles_world(a.seed + i, 0, 0))
                      for i in range(n_worlds)])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = BatchedAuvEnv(cfg, bank, a.envs, device=a.device, rewarder="colav" if colav else "pathfollow", auto_reset=True)
    env.reset()
    net = load_policy(a.ckpt, a.frame_stack * env.obs_dim, a.device, a.seed, hidden=tuple(int(h) for h in a.net_arch.split(",")))
    kw = {}
    if a.act_space == "normalized" or a.squash:                        # the policy speaks [-1, 1]^2; the map stretches it onto the action space
        lo, hi = env.action_space.low, env.action_space.high
        kw = dict(act_mid=((lo + hi) / 2).tolist(), act_half=((hi - lo) / 2).tolist(), clip_lo=[-1.0, -1.0], clip_hi=[1.0, 1.0])
    fused = FusedActorCritic(net, env, rollout=1, frames=a.frame_stack, squash=bool(a.squash), **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if a.frames:
        os.makedirs(a.frames, exist_ok=True)
        save_frames(env, a.frames, 0)
    log, steps = evaluate(env, fused, a.episodes, a.max_steps, frames_dir=a.frames)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    k = int(log.shape[0])
    res = dict(task=a.task, envs=a.envs, episodes=k, steps=steps, env_steps_per_s=steps * a.envs / dt)
    if k:
        col = {c: log[:, i] for i, c in enumerate(BatchedAuvEnv.EPISODE_LOG_COLUMNS)}
        goal, coll = col["reached_goal"] != 0, col["collision"] != 0
        res.update(goal_rate=float(goal.double().mean()), collision_rate=float(coll.double().mean()),
                   other_rate=float((~goal & ~coll).double().mean()), return_mean=float(col["reward"].mean()),
                   length_mean=float(col["timesteps"].mean()), progress_mean=float(col["progress"].mean()),
                   cross_track_error_mean=float(col["cross_track_error"].mean()))
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
