#!/usr/bin/env python3
"""Augmented Random Search (V1; Mania, Guy, Recht 2018) of a linear policy on the PathFollow task, every rollout step chosen INSIDE
the launch (BatchedAuvEnv.step_feedback):
    python examples/ars.py [--envs 4096] [--iterations 200] [--horizon 256] [--out profiles/feedback/ars_curve.jsonl]
The policy is a 2 x 7 matrix M on (six navigation features, 1): thrust and rudder, clipped by the dynamics.  An iteration draws
P = envs / 2 directions d_k, gives environment k the gain row M + nu d_k and environment P + k the row M - nu d_k (both in world k,
from its reset state), runs `horizon` steps in launches of at most 64, takes every environment's return from the reward / done
record up to and including its first done (auv_plan_score, group 1, gamma 1) and steps
    M += alpha / (b sigma_R) * sum over the b best directions of (r+ - r-) d_k.
Prints mean return and mean progress per iteration.  No learning result is promised.
    python examples/ars.py --sectors [--out profiles/feedback_sectors/ars_curve.jsonl]
also searches a 2 x 4 matrix Hs on the LiDAR's four sector inputs (the largest closeness in each of the configuration's 4 x 8
sectors, step_feedback(..., sector_gains=)): the same directions d_k are drawn for (M, Hs) together, both matrices are perturbed
and stepped alike.  Hs starts at zero.
    python examples/ars.py --fresh-worlds 1
runs every rollout on worlds nobody has seen (FreshWorlds(multi_step=True, closed_loop=True): the generator's 17 movers + 11
circles, one chain) instead of the fixed bank -- every iteration's reset() moves every environment to its next unseen world, so
the two environments of a direction no longer share a world -- and prints fresh_stats() (`reused`, `regenerated`) at the end."""
import argparse
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_auv_amd import planning  # noqa: E402
from gym_auv_amd.batched_env import BatchedAuvEnv  # noqa: E402
from gym_auv_amd.config import effective_reference_config  # noqa: E402
from gym_auv_amd.feedback import los_gains  # noqa: E402
from gym_auv_amd.world import build_bank_parallel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--iterations", type=int, default=200)
ap.add_argument("--horizon", type=int, default=256)
ap.add_argument("--nu", type=float, default=0.05)
ap.add_argument("--alpha", type=float, default=0.02)
ap.add_argument("--top", type=float, default=0.25, help="share of the directions an update uses")
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--out", default=None)
ap.add_argument("--fresh-worlds", type=int, default=0, choices=(0, 1),
                help="1: every rollout on worlds nobody has seen (FreshWorlds, closed loop allowed) instead of the fixed bank")
ap.add_argument("--sectors", action="store_true", help="also perturb gains on the LiDAR's sector inputs")
args = ap.parse_args()
dev = torch.device("cuda:0")
n, H = args.envs, args.horizon
P = n // 2
assert n == 2 * P and P >= 1
cfg = effective_reference_config(use_lidar=True)
cfg.vessel.n_sectors, cfg.vessel.n_sensors_per_sector = 4, 8
cfg.episode.max_timesteps = H
if args.fresh_worlds:
    # a fresh world on every reset, as the reference trains: reset() moves every environment to its next unseen world (the library
    # chooses it), so the two environments of a direction meet two different worlds and r+ - r- carries that difference too
    from gym_auv_amd.devgen import FreshWorlds  # noqa: E402
    env = BatchedAuvEnv(cfg, FreshWorlds(depth=3, multi_step=True, closed_loop=True, seed=args.seed, batch_cap=min(n, 512)), n, device=dev, rewarder="pathfollow",
                        auto_reset=True)
else:
    bank = build_bank_parallel("static_circles_world", 4000 + np.arange(P), procs=16, n_circles=8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                        # (one world per pair of environments, on purpose)
        env = BatchedAuvEnv(cfg, bank, n, device=dev, rewarder="pathfollow", auto_reset=True)
env.set_sub_batches(1, inline_first=True)               # the one chain IS the caller's stream: launches, resets and scoring in order
worlds = torch.arange(n, device=dev, dtype=torch.int32) % P
gen = torch.Generator(device=dev)
gen.manual_seed(args.seed)
M = torch.zeros((2, 7), dtype=torch.float64, device=dev)
M[0, 6] = 0.5                                               # start: half thrust, rudder amidships
NS = cfg.vessel.n_sectors                                   # 4 sector inputs; the other 12 columns of the sector gains stay 0
Hs = torch.zeros((2, NS), dtype=torch.float64, device=dev)
b = max(1, int(args.top * P))
log = open(args.out, "w") if args.out else None
if log:
    log.write(json.dumps(dict(command=" ".join(sys.argv), envs=n, directions=P, horizon=H, nu=args.nu, alpha=args.alpha, top=b, sectors=bool(args.sectors),
                              baseline_los_gains=los_gains(0.5, 1.0, 0.5).tolist())) + "\n")
for it in range(args.iterations):
    t0 = time.perf_counter()
    d = torch.randn((P, 2, 7), generator=gen, dtype=torch.float64, device=dev)
    gains = torch.zeros((n, 2, 8), dtype=torch.float64, device=dev)
    gains[:P, :, :7] = M + args.nu * d
    gains[P:, :, :7] = M - args.nu * d
    sgains = None
    if args.sectors:
        ds = torch.randn((P, 2, NS), generator=gen, dtype=torch.float64, device=dev)
        sgains = torch.zeros((n, 2, 16), dtype=torch.float64, device=dev)
        sgains[:P, :, :NS] = Hs + args.nu * ds
        sgains[P:, :, :NS] = Hs - args.nu * ds
    env.reset(world_idx=None if args.fresh_worlds else worlds)
    rew, done = [], []
    for t in range(0, H, 64):
        _, r, dn = env.step_feedback(gains, min(64, H - t), record="reward", sector_gains=sgains)
        rew.append(r), done.append(dn)
    rew, done = torch.cat(rew).contiguous(), torch.cat(done).contiguous()
    ret, _ = planning.plan_score(env, rew, done, 1, 1.0)
    ret = ret.double()
    # progress along the path when the first episode ended (episode log), or now for an environment that is still in it
    prog = env.read("INFO64")[:, 3].clone()
    rows = env.episode_log().cpu().numpy()
    if len(rows):
        first = np.unique(rows[:, 0].astype(np.int64), return_index=True)
        prog[torch.as_tensor(first[0], device=dev)] = torch.as_tensor(rows[first[1], 5], device=dev)
    rp, rm = ret[:P], ret[P:]
    top = torch.topk(torch.maximum(rp, rm), b).indices
    sigma = torch.cat([rp[top], rm[top]]).std().clamp_min(1e-8)
    M += args.alpha / (b * sigma) * ((rp[top] - rm[top])[:, None, None] * d[top]).sum(dim=0)
    if args.sectors:
        Hs += args.alpha / (b * sigma) * ((rp[top] - rm[top])[:, None, None] * ds[top]).sum(dim=0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    row = dict(iteration=it, mean_return=float(ret.mean()), best_return=float(ret.max()), mean_progress=float(prog.mean()),
               rate_M=round(n * H / dt / 1e6, 2), health_ok=env.health()["timeouts"] == 0)
    print(json.dumps(row), flush=True)
    if log:
        log.write(json.dumps(row) + "\n")
        log.flush()
if log:
    log.write(json.dumps(dict(final_policy=M.tolist(), final_sector_gains=Hs.tolist() if args.sectors else None)) + "\n")
    log.close()
if args.fresh_worlds:
    st = env.fresh_stats()
    print(json.dumps(dict(fresh_stats=dict(reused=st["reused"], regenerated=st["regenerated"]))), flush=True)
env.close()
