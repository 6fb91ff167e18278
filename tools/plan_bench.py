#!/usr/bin/env python3
"""What a shooting plan costs beside the launch it is built around (measured, not gated):
    python tools/plan_bench.py [--out profiles/plan] [--workloads polygons50,moving28] [--real 64] [--candidates 64] [--horizon 16]
One process; B real environments, B * K planner environments, T steps.  Per workload:
    restore_us      auv_restore of the B * K planner environments (K-fold fork of B rows): HIP events on its stream, warmed, median of 30
    launch_us       the step_multi(record="reward") launch it precedes, same handle, same events
    score_us        auv_plan_score over the [T][B * K] record
    plans_per_s     whole ShootingPlanner.plan() calls over >= 1 s of wall clock, ended by a synchronise (snapshot, restore, sampling,
                    launch, scoring, the choice: everything a decision costs)
    other_share     1 - launch_us * plans_per_s / 1e6: the share of a plan that is NOT the launch
Writes README.md and plan_bench.jsonl under --out, with the snapshot row size and the library's sha256.

    python tools/plan_bench.py --compare-samplers [--out profiles/plan_device] [--workloads moving28] [--passes 5]
The planner's two samplers side by side instead: per workload and for iterations = 1 and 3, ShootingPlanner(sampler="torch") and
(sampler="device") on the same real batch, timed in ALTERNATING passes of one session (torch, device, torch, device, ...: a drift of
the machine hits both alike).  A pass is >= 0.5 s of back-to-back plan() calls ended by a synchronise; the figure is the median of
the passes.  With it the step_multi launch inside the plan alone (event-timed) and the launches per iteration, counted in
gym_auv_amd/planning.py -- not measured."""
import argparse
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_auv_amd import _capi, planning  # noqa: E402
from gym_auv_amd.batched_env import BatchedAuvEnv  # noqa: E402
from gym_auv_amd.config import effective_reference_config  # noqa: E402
from gym_auv_amd.world import build_bank_parallel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/plan")
ap.add_argument("--workloads", default="polygons50,moving28")
ap.add_argument("--real", type=int, default=64)
ap.add_argument("--candidates", type=int, default=64)
ap.add_argument("--horizon", type=int, default=16)
ap.add_argument("--worlds", type=int, default=128)
ap.add_argument("--compare-samplers", action="store_true")
ap.add_argument("--passes", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda:0")
B, K, T = args.real, args.candidates, args.horizon


def timed(fn, reps=30, warm=5):
    """median / min of `reps` event-timed calls of fn() on the current stream, in microseconds"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(out)), float(np.min(out))


# launches per iteration, read off ShootingPlanner.plan / _plan_device (restore, step_multi and the scorer are common to both):
#   torch   randn, multiply, add, the slice copy for candidate 0, minimum, maximum; in a refit nan_to_num, topk (sort + gather), gather,
#           mean, std, clamp_min -- 6 around every launch and about 7 more per refit; behind the last iteration 4 for the choice
#   device  auv_plan_sample, auv_plan_refit
LAUNCHES = {"torch": "3 + 6 (sampling) + about 7 (refit; not behind the last iteration) and 4 once per plan (the choice)",
            "device": "3 + 2 (auv_plan_sample, auv_plan_refit)"}


def plan_pass(planner, seconds=0.5):
    """microseconds per plan() over >= `seconds` of back-to-back calls, ended by a synchronise"""
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds:
        for _ in range(10):
            planner.plan()
        n += 10
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / n


def compare_samplers():
    rows = []
    for wl in args.workloads.split(","):
        gen, kw = ("polygon_world", dict(n_polygons=50)) if wl == "polygons50" else ("moving_obstacles_world", dict())
        bank = build_bank_parallel(gen, 1000 + np.arange(args.worlds), procs=16, **kw)
        cfg = effective_reference_config(use_lidar=True)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            real = BatchedAuvEnv(cfg, bank, B, device=dev, auto_reset=True)
        real.reset()
        warm = torch.rand((20, B, 2), device=dev) * torch.tensor([2.0, 0.3], device=dev) - torch.tensor([1.0, 0.15], device=dev)
        for t in range(20):
            real.step(warm[t])
        for iterations in (1, 3):
            planners = {s: planning.ShootingPlanner(real, candidates=K, horizon=T, gamma=0.99, seed=1, iterations=iterations, sampler=s)
                        for s in ("torch", "device")}
            for p in planners.values():
                for _ in range(5):
                    p.plan()
            torch.cuda.synchronize()
            sim = planners["device"].sim
            last = planners["device"].last
            rec = (None, torch.empty_like(last["reward"]), torch.empty_like(last["done"]))
            launch = timed(lambda: sim.step_multi(last["ring"], 0, T, record=rec))
            us = {s: [] for s in planners}
            for _ in range(args.passes):
                for s in ("torch", "device"):
                    us[s].append(plan_pass(planners[s]))
            row = dict(workload=wl, real_envs=B, candidates=K, horizon=T, planner_envs=B * K, iterations=iterations,
                       plan_us_torch=float(np.median(us["torch"])), plan_us_device=float(np.median(us["device"])),
                       plan_us_torch_passes=us["torch"], plan_us_device_passes=us["device"], launch_us_median=launch[0], launch_us_min=launch[1],
                       launches_per_iteration=LAUNCHES, lib_sha256=sha, health=sim.health())
            row["device_over_torch"] = row["plan_us_device"] / row["plan_us_torch"]
            rows.append(row)
            print(json.dumps(row), flush=True)
            for p in planners.values():
                p.close()
        real.close()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "plan_bench.jsonl"), "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    with open(os.path.join(args.out, "README.md"), "w") as f:
        f.write("# The planner's sampler on the device beside the torch one\n\n`python tools/plan_bench.py --compare-samplers` on one MI355X, one "
                "process; %d real environments x %d candidates = %d planner environments, horizon %d.  Library sha256 `%s`.\n\n"
                "`plan us` is wall clock per `plan()` over >= 0.5 s of back-to-back calls ended by a synchronise: the median of %d passes per "
                "sampler, the two samplers taking turns pass by pass in one session.  `launch us` is the `step_multi(record=\"reward\")` launch "
                "inside an iteration alone (events, median of 30).  The plans differ (the samplers draw different noise); the work per plan is "
                "the same.\n\n| workload | iterations | launch us | plan us, torch | plan us, device | device / torch |\n|---|---|---|---|---|---|\n"
                % (B, K, B * K, T, sha, args.passes))
        for r in rows:
            f.write("| %s | %d | %.1f | %.1f | %.1f | %.2f |\n" % (r["workload"], r["iterations"], r["launch_us_median"], r["plan_us_torch"],
                                                                 r["plan_us_device"], r["device_over_torch"]))
        slower = [r for r in rows if r["device_over_torch"] > 1.0]
        f.write("\nLaunches per iteration (counted in `gym_auv_amd/planning.py`, not measured; restore, `step_multi` and the scorer are the 3 both "
                "have): torch %s; device %s.\n" % (LAUNCHES["torch"], LAUNCHES["device"]))
        if slower:
            f.write("\n**The device sampler's `plan()` is SLOWER than the torch one** in: %s.\n"
                    % "; ".join("%s, %d iteration(s): by %.1f %%" % (r["workload"], r["iterations"], 100 * (r["device_over_torch"] - 1)) for r in slower))
        else:
            f.write("\nThe device sampler's `plan()` is not slower than the torch one in any row.\n")
        f.write("\nRaw rows, with every pass: `plan_bench.jsonl`.\n")


rows = []
sha = hashlib.sha256(open(_capi.LIB_PATH, "rb").read()).hexdigest()
if args.compare_samplers:
    compare_samplers()
    sys.exit(0)
for wl in args.workloads.split(","):
    gen, kw = ("polygon_world", dict(n_polygons=50)) if wl == "polygons50" else ("moving_obstacles_world", dict())
    bank = build_bank_parallel(gen, 1000 + np.arange(args.worlds), procs=16, **kw)
    cfg = effective_reference_config(use_lidar=True)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        real = BatchedAuvEnv(cfg, bank, B, device=dev, auto_reset=True)
    real.reset()
    warm = torch.rand((20, B, 2), device=dev) * torch.tensor([2.0, 0.3], device=dev) - torch.tensor([1.0, 0.15], device=dev)
    for t in range(20):
        real.step(warm[t])
    planner = planning.ShootingPlanner(real, candidates=K, horizon=T, gamma=0.99, seed=1)
    sim = planner.sim
    planner.plan()
    torch.cuda.synchronize()
    snap = real.snapshot()
    ring, rew, done = planner.last["ring"], planner.last["reward"], planner.last["done"]
    rec = (None, torch.empty_like(rew), torch.empty_like(done))
    restore = timed(lambda: sim.restore(snap, rows=planner._rows, envs=planner._envs, validate=False))
    launch = timed(lambda: sim.step_multi(ring, 0, T, record=rec))
    score = timed(lambda: planning.plan_score(sim, rew, done, K, 0.99))
    snapshot = timed(lambda: real.snapshot())
    for _ in range(5):
        planner.plan()
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < 1.5:
        for _ in range(20):
            planner.plan()
        n += 20
    torch.cuda.synchronize()
    rate = n / (time.perf_counter() - t0)
    row = dict(workload=wl, real_envs=B, candidates=K, horizon=T, planner_envs=B * K, row_bytes=real.snapshot_row_bytes,
               snapshot_us_median=snapshot[0], restore_us_median=restore[0], restore_us_min=restore[1], launch_us_median=launch[0],
               launch_us_min=launch[1], score_us_median=score[0], score_us_min=score[1], plans_per_s=rate, plan_us=1e6 / rate,
               other_share=1.0 - launch[0] * rate / 1e6, env_steps_per_s_inside_plans=rate * B * K * T, lib_sha256=sha,
               health=sim.health(), skipped=sim.snapshot_skipped())
    rows.append(row)
    print(json.dumps(row), flush=True)
    planner.close(), real.close()

os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, "plan_bench.jsonl"), "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
with open(os.path.join(args.out, "README.md"), "w") as f:
    f.write("# What a shooting plan costs beside its launch\n\n`python tools/plan_bench.py` on one MI355X, one process; %d real environments x %d "
            "candidates = %d planner environments, horizon %d.  Library sha256 `%s`.\n\nEvent-timed figures are medians of 30 calls on the "
            "stream they run on, after a warm-up; `plans/s` is wall clock over >= 1.5 s of back-to-back `plan()` calls ended by a synchronise. "
            "`other` is the share of a plan that is not the `step_multi(record=\"reward\")` launch: snapshot, restore, sampling the ring, scoring, "
            "choosing, and the host's time per call where the GPU waits for it.\n\n"
            "| workload | row bytes | restore us | launch us | score us | plan us | plans/s | other |\n|---|---|---|---|---|---|---|---|\n"
            % (B, K, B * K, T, sha))
    for r in rows:
        f.write("| %s | %d | %.1f | %.1f | %.1f | %.1f | %.0f | %.0f %% |\n" % (r["workload"], r["row_bytes"], r["restore_us_median"],
                                                                            r["launch_us_median"], r["score_us_median"], r["plan_us"],
                                                                            r["plans_per_s"], 100 * r["other_share"]))
    f.write("\nRaw rows: `plan_bench.jsonl`.\n")
