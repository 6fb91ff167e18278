#!/usr/bin/env python3
"""Augmented Random Search (V1; Mania, Guy, Recht 2018) of a ONE-HIDDEN-LAYER policy on the PathFollow task, every rollout step
chosen INSIDE the launch (BatchedAuvEnv.step_feedback(..., hidden=)):
    python examples/ars_hidden.py [--envs 4096] [--iterations 200] [--horizon 256] [--units 8] [--activation relu] [--out curve.jsonl]
The loop of examples/ars.py over the packed hidden block of gym_auv_amd/feedback.py.  The policy is
    a = M (six navigation features, 1) + V act(W1 v + b1),   v = (six navigation features, 0, 0, the LiDAR's four sector inputs)
with `--units` <= 16 hidden units (the other rows of the block stay zero).  The search vector theta is the block's live entries --
W1 on the 6 + 4 inputs that carry something, b1 and V -- and the 2 x 7 matrix M.  An iteration draws P = envs / 2 directions d_k,
one per pair of environments: environment k runs theta + nu d_k, environment P + k runs theta - nu d_k, both in world k from its
reset state, each with its OWN [16, 28] block in the launch; returns and the update are examples/ars.py's.  W1 and b1 start as
N(0, 0.1) (with W1 = 0 and V = 0 together no direction changes the return to first order), V at zero -- the first rollouts are the
affine policy's -- and M at half thrust.  Prints mean return and mean progress per iteration.  No learning result is promised.
`--fresh-worlds 1`: as in examples/ars.py -- every rollout on worlds nobody has seen, fresh_stats() printed at the end."""
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
from gym_auv_amd.feedback import HIDDEN_ROW, N_HIDDEN  # noqa: E402
from gym_auv_amd.world import build_bank_parallel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--iterations", type=int, default=200)
ap.add_argument("--horizon", type=int, default=256)
ap.add_argument("--units", type=int, default=8)
ap.add_argument("--activation", default="relu", choices=("relu", "hardtanh"))
ap.add_argument("--nu", type=float, default=0.05)
ap.add_argument("--alpha", type=float, default=0.02)
ap.add_argument("--top", type=float, default=0.25, help="share of the directions an update uses")
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--out", default=None)
ap.add_argument("--fresh-worlds", type=int, default=0, choices=(0, 1),
                help="1: every rollout on worlds nobody has seen (FreshWorlds, closed loop allowed) instead of the fixed bank")
args = ap.parse_args()
dev = torch.device("cuda:0")
n, H, U = args.envs, args.horizon, args.units
P = n // 2
assert n == 2 * P and P >= 1 and 1 <= U <= N_HIDDEN
cfg = effective_reference_config(use_lidar=True)
cfg.vessel.n_sectors, cfg.vessel.n_sensors_per_sector = 4, 8
cfg.episode.max_timesteps = H
NS = cfg.vessel.n_sectors
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
# the block's live entries: rows < U; columns 0..5 (navigation), 8..8 + NS - 1 (sectors), 24 (bias), 25, 26 (V); no ring, so 6, 7 stay 0
live = torch.zeros((N_HIDDEN, HIDDEN_ROW), dtype=torch.bool, device=dev)
live[:U, :6] = live[:U, 8:8 + NS] = live[:U, 24:27] = True
theta = torch.zeros((N_HIDDEN, HIDDEN_ROW), dtype=torch.float64, device=dev)
theta[:, :25] = 0.1 * torch.randn((N_HIDDEN, 25), generator=gen, dtype=torch.float64, device=dev)
theta *= live
theta[:, 25:27] = 0.0                                       # V = 0: the first rollouts are the affine policy's
M = torch.zeros((2, 7), dtype=torch.float64, device=dev)
M[0, 6] = 0.5                                               # start: half thrust, rudder amidships
zero_sectors = torch.zeros((2, 16), dtype=torch.float64, device=dev)      # the affine sector terms are off: the layer sees the sectors
b = max(1, int(args.top * P))
log = open(args.out, "w") if args.out else None
if log:
    log.write(json.dumps(dict(command=" ".join(sys.argv), envs=n, directions=P, horizon=H, units=U, activation=args.activation, nu=args.nu,
                              alpha=args.alpha, top=b, parameters=int(live.sum()) + 14)) + "\n")
for it in range(args.iterations):
    t0 = time.perf_counter()
    d = torch.randn((P, 2, 7), generator=gen, dtype=torch.float64, device=dev)
    dh = torch.randn((P, N_HIDDEN, HIDDEN_ROW), generator=gen, dtype=torch.float64, device=dev) * live
    gains = torch.zeros((n, 2, 8), dtype=torch.float64, device=dev)
    gains[:P, :, :7] = M + args.nu * d
    gains[P:, :, :7] = M - args.nu * d
    hidden = torch.cat([theta + args.nu * dh, theta - args.nu * dh])
    env.reset(world_idx=None if args.fresh_worlds else worlds)
    rew, done = [], []
    for t in range(0, H, 64):
        _, r, dn = env.step_feedback(gains, min(64, H - t), record="reward", sector_gains=zero_sectors, hidden=hidden, activation=args.activation)
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
    wgt = (args.alpha / (b * sigma) * (rp[top] - rm[top]))[:, None, None]
    M += (wgt * d[top]).sum(dim=0)
    theta += (wgt * dh[top]).sum(dim=0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    row = dict(iteration=it, mean_return=float(ret.mean()), best_return=float(ret.max()), mean_progress=float(prog.mean()),
               rate_M=round(n * H / dt / 1e6, 2), health_ok=env.health()["timeouts"] == 0)
    print(json.dumps(row), flush=True)
    if log:
        log.write(json.dumps(row) + "\n")
        log.flush()
if log:
    log.write(json.dumps(dict(final_policy=M.tolist(), final_hidden=theta.tolist())) + "\n")
    log.close()
if args.fresh_worlds:
    st = env.fresh_stats()
    print(json.dumps(dict(fresh_stats=dict(reused=st["reused"], regenerated=st["regenerated"]))), flush=True)
env.close()
