#!/usr/bin/env python3
"""Closed-loop rate with the action chosen INSIDE a launch of several steps (auv_step_feedback) against the open-loop launch and
against what a caller had before -- one step() per step with the same law as torch ops on env.obs:
    python tools/feedback_bench.py [--out profiles/feedback] [--envs 4096] [--steps 1920] [--passes 5]
4096 x 180 beams, 50 polygons, one chain, 64 steps per launch.  `--passes` alternating passes of
    (a) open_loop   step_multi(ring, record="reward"): the open-loop kernel
    (b) feedback    step_feedback(los_gains(...), record="reward"): the line-of-sight autopilot, no ring
    (c) per_step    obs -> six columns -> the same gain row as two torch matrix-vector products -> step(), once per step
each warmed by half a pass, timed by the host clock around `--steps` steps ended by a device synchronise.  Writes every figure,
the library's sha256 and the command to feedback_bench.jsonl and a table to README.md under --out (an ARS curve that
examples/ars.py left in ars_curve.jsonl there is added to the README).
    python tools/feedback_bench.py --sectors [--out profiles/feedback_sectors]
measures instead, in the same alternating passes, (b) against
    (d) feedback_sectors   step_feedback(los_gains(...), sector_gains=..., record="reward"): the same autopilot with the LiDAR's
                           sector inputs in the law (auv_step_feedback_sectors; the reference's 9 x 20 partition, every sector gain
                           non-zero: the rudder steers away from the side of the nearest return, the thrust drops with it)
and writes the rows to feedback_sectors_bench.jsonl and the ranges and their ratio to feedback_sectors_bench.md under --out.
    python tools/feedback_bench.py --hidden [--out profiles/feedback_hidden]
measures, in the same alternating passes,
    (d) feedback_sectors   as above: the yardstick
    (e) feedback_hidden    step_feedback(los_gains(...), sector_gains=..., hidden=..., record="reward"): the same law with 16 relu
                           units over its 24 inputs (auv_step_feedback_hidden; per-environment N(0, 0.3) weights, every entry non-zero)
    (f) per_step_hidden    one step() per step with the same law as torch ops on env.obs (float32: a gather and a maximum for the
                           sector inputs, two matrix products for the layer)
and writes the rows to feedback_hidden_bench.jsonl and the ranges, b / a and the verdict to README.md under --out.
    python tools/feedback_bench.py --fresh-worlds [--depth 3] [--batch-cap 256] [--out profiles/feedback_fresh]
measures on the generator's moving28 worlds (17 movers + 11 circles), in the same alternating passes, the open-loop launch and the
three closed-loop launches (affine, sectors, hidden) each on a cycling bank of 2 N generated worlds and -- `fresh_` -- on a handle
with a fresh world on every reset (FreshWorlds(depth, multi_step=True, closed_loop=True, batch_cap), one chain), and `per_step_fresh`: one step()
per step on that handle with the affine law as torch ops.  Fresh rows carry the re-uses counted during their timed pass; a census
behind the passes counts the episodes of `--steps` steps.  Writes feedback_fresh_bench_depth<D>.jsonl and .md under --out."""
import argparse
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_auv_amd import _capi  # noqa: E402
from gym_auv_amd.batched_env import BatchedAuvEnv  # noqa: E402
from gym_auv_amd.config import effective_reference_config  # noqa: E402
from gym_auv_amd.feedback import default_sector_bounds, los_gains, pack_hidden  # noqa: E402
from gym_auv_amd.world import build_bank_parallel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--sectors", action="store_true", help="measure the launch with sector inputs against the one without")
ap.add_argument("--hidden", action="store_true", help="measure the launch with a hidden layer against the sector launch and per-step torch ops")
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--steps", type=int, default=1920)
ap.add_argument("--passes", type=int, default=5)
ap.add_argument("--launch", type=int, default=64)
ap.add_argument("--fresh-worlds", action="store_true", help="measure the closed-loop launches on a fresh world per reset (moving28) against a cycling bank")
ap.add_argument("--depth", type=int, default=3, help="--fresh-worlds: bank slots per environment")
ap.add_argument("--batch-cap", type=int, default=256, help="--fresh-worlds: worlds per refill pass at most (profiles/multi_fresh: 256)")
args = ap.parse_args()
if args.out is None:
    args.out = "profiles/feedback_hidden" if args.hidden else ("profiles/feedback_sectors" if args.sectors else "profiles/feedback")
    if args.fresh_worlds:
        args.out = "profiles/feedback_fresh"
dev = torch.device("cuda:0")
n, T, steps = args.envs, args.launch, args.steps
cfg = effective_reference_config(use_lidar=True)
if args.fresh_worlds:
    # moving28 (17 movers, 11 circles: the generator's worlds) on both handles: a cycling bank of 2 N generated worlds, and a fresh
    # world on every reset with the closed loop allowed
    from gym_auv_amd.devgen import FreshWorlds, GeneratedWorlds  # noqa: E402
    bank = GeneratedWorlds(2 * n, seed=0)
else:
    bank = build_bank_parallel("polygon_world", 1000 + np.arange(2 * n), procs=16, n_polygons=50)
ring = torch.rand((T, n, 2), device=dev) * torch.tensor([2.0, 0.3], device=dev) - torch.tensor([1.0, 0.15], device=dev)
g_np = los_gains(0.7, 0.8, 0.4, 0.5)
gains = torch.as_tensor(np.broadcast_to(g_np, (n, 2, 8)).copy(), device=dev)
# (c): the same row in float32 on the float32 observation -- a = W obs[:, :6] + b, what a caller writes in torch
W = torch.as_tensor(g_np[:, :6], dtype=torch.float32, device=dev).t().contiguous()
b = torch.as_tensor(g_np[:, 6], dtype=torch.float32, device=dev)
env = BatchedAuvEnv(cfg, bank, n, device=dev, auto_reset=True)
env.reset()
env.set_sub_batches(1)


def open_loop(m):
    for i in range(0, m, T):
        env.step_multi(ring, 0, T, record="reward")


def feedback(m):
    for i in range(0, m, T):
        env.step_feedback(gains, T, record="reward")


# (d): every sector gain non-zero -- rudder away from the side of the nearest return (the first sectors are to starboard: the beams
# run from -pi to pi, sensor.py:110), thrust down with any return
h_np = np.zeros((2, 16))
ns = cfg.vessel.n_sectors
h_np[0, :ns] = -0.3 / ns
h_np[1, :ns] = np.where(np.arange(ns) < ns / 2.0, 0.1, -0.1)
sector_gains = torch.as_tensor(np.broadcast_to(h_np, (n, 2, 16)).copy(), device=dev)


def feedback_sectors(m):
    for i in range(0, m, T):
        env.step_feedback(gains, T, record="reward", sector_gains=sector_gains)


# (e): one block per environment (the parameter traffic of a population), every entry non-zero
_rs = np.random.RandomState(7)
W1_np, b1_np, V_np = _rs.normal(0, 0.3, (n, 16, 24)), _rs.normal(0, 0.3, (n, 16)), _rs.normal(0, 0.05, (n, 2, 16))
hidden = torch.as_tensor(pack_hidden(W1_np, b1_np, V_np), device=dev) if (args.hidden or args.fresh_worlds) else None


def feedback_hidden(m):
    for i in range(0, m, T):
        env.step_feedback(gains, T, record="reward", sector_gains=sector_gains, hidden=hidden)


# (f): the same law in float32 on the float32 observation, what a caller writes in torch.  The sector maxima: one gather of the
# closeness columns into [N, K, widest sector] (short sectors repeat their last beam) and a maximum
if args.hidden:
    sb = default_sector_bounds(cfg)
    wide = int(np.diff(sb).max())
    idx_np = np.stack([6 + np.minimum(sb[k] + np.arange(wide), sb[k + 1] - 1) for k in range(ns)])
    sec_idx = torch.as_tensor(idx_np.reshape(-1), dtype=torch.long, device=dev)
    W1_t = torch.as_tensor(W1_np, dtype=torch.float32, device=dev)                           # [N, 16, 24]
    b1_t = torch.as_tensor(b1_np, dtype=torch.float32, device=dev)
    V_t = torch.as_tensor(V_np, dtype=torch.float32, device=dev)                              # [N, 2, 16]
    H_t = torch.as_tensor(h_np[:, :ns], dtype=torch.float32, device=dev).t().contiguous()     # [K, 2]
    v_buf = torch.zeros((n, 24), dtype=torch.float32, device=dev)                             # v_6 = v_7 = 0 (no ring), padding sectors 0


def per_step_hidden(m):
    for i in range(m):
        obs = env.obs
        z = obs.index_select(1, sec_idx).view(n, ns, wide).amax(dim=2)
        v_buf[:, :6] = obs[:, :6]
        v_buf[:, 8:8 + ns] = z
        y = torch.relu(torch.baddbmm(b1_t.unsqueeze(2), W1_t, v_buf.unsqueeze(2)))            # [N, 16, 1]
        a = torch.addmm(b, obs[:, :6], W) + z @ H_t + torch.bmm(V_t, y).squeeze(2)
        env.step(a)


def per_step(m):
    for i in range(m):
        env.step(torch.addmm(b, env.obs[:, :6], W))


FORMS = (("open_loop", open_loop), ("feedback", feedback), ("per_step", per_step))
if args.sectors:
    FORMS = (("feedback", feedback), ("feedback_sectors", feedback_sectors))
if args.hidden:
    FORMS = (("feedback_sectors", feedback_sectors), ("feedback_hidden", feedback_hidden), ("per_step_hidden", per_step_hidden))
fre = None
if args.fresh_worlds:
    # every form on the cycling bank (`cyc`: the launches as they were) and on the fresh-world handle (`fre`), one after the other in
    # every pass; the forms above step the global `env`, so a form is bound to its handle by naming it there
    cyc = env
    fre = BatchedAuvEnv(cfg, FreshWorlds(depth=args.depth, multi_step=True, closed_loop=True, batch_cap=args.batch_cap), n, device=dev, auto_reset=True)
    fre.reset()
    fre.set_sub_batches(1)

    def on(handle, run):
        def bound(m):
            global env
            env = handle
            run(m)
        return bound

    FORMS = tuple((prefix + name, on(handle, run)) for name, run in (("open_loop", open_loop), ("feedback", feedback),
                                                                      ("feedback_sectors", feedback_sectors), ("feedback_hidden", feedback_hidden))
                  for prefix, handle in (("", cyc), ("fresh_", fre))) + (("per_step_fresh", on(fre, per_step)),)
sha = hashlib.sha256(open(_capi.LIB_PATH, "rb").read()).hexdigest()
rows = []
for p in range(args.passes):
    for name, run in FORMS:
        run(steps // 2)
        torch.cuda.synchronize()
        reused0 = fre.fresh_stats()["reused"] if fre is not None else 0
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        row = dict(form=name, pass_=p, envs=n, beams=env.n_sensors, steps=steps, steps_per_launch=1 if name.startswith("per_step") else T,
                   rate_M=round(n * steps / dt / 1e6, 2), us_per_step=round(1e6 * dt / steps, 2), health=env.health(), lib_sha256=sha,
                   command=" ".join(sys.argv))
        if fre is not None and env is fre:
            row["reused"] = fre.fresh_stats()["reused"] - reused0
        rows.append(row)
        print(json.dumps(row), flush=True)
if fre is not None:
    # episodes per `steps` steps of the fresh closed loop (hidden law), counted beside the timed passes: the done record summed on
    # the device behind the chain, read once at the end
    fre.episode_log()
    ep = torch.zeros((), dtype=torch.int64, device=dev)
    reused0 = fre.fresh_stats()["reused"]
    for i in range(0, steps, T):
        _, _, dn = fre.step_feedback(gains, T, record="reward", sector_gains=sector_gains, hidden=hidden)
        fre._join_chains()
        ep += dn.sum()
    torch.cuda.synchronize()
    census = dict(form="census_fresh_feedback_hidden", depth=args.depth, steps=steps, episodes=int(ep), reused=fre.fresh_stats()["reused"] - reused0,
                  fresh_stats=fre.fresh_stats(), health=fre.health(), lib_sha256=sha, command=" ".join(sys.argv))
    rows.append(census)
    print(json.dumps(census), flush=True)
    cyc.close(), fre.close()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "feedback_fresh_bench_depth%d.jsonl" % args.depth), "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    med = lambda v: sorted(v)[len(v) // 2]
    with open(os.path.join(args.out, "feedback_fresh_bench_depth%d.md" % args.depth), "w") as f:
        f.write("`python %s`: %d environments x %d beams, moving28, one chain, %d steps per launch, depth %d, batch_cap %d; %d alternating passes over %d "
                "steps.  Library sha256 `%s`.\n\n| form | M env-steps/s per pass | median | min | max | reused per pass |\n|---|---|---|---|---|---|\n"
                % (" ".join(sys.argv), n, cyc.n_sensors, T, args.depth, args.batch_cap, args.passes, steps, sha))
        for name, _ in FORMS:
            v = [r["rate_M"] for r in rows if r["form"] == name]
            ru = [str(r["reused"]) for r in rows if r["form"] == name and "reused" in r]
            f.write("| %s | %s | %.1f | %.1f | %.1f | %s |\n" % (name, ", ".join("%.1f" % x for x in v), med(v), min(v), max(v), ", ".join(ru) or "-"))
        f.write("\nfresh / cycling, medians: %s.\n\nCensus (hidden law, %d steps): %d episodes, %d re-used.\n"
                % ("; ".join("%s %.3f" % (k, med([r["rate_M"] for r in rows if r["form"] == "fresh_" + k]) / med([r["rate_M"] for r in rows if r["form"] == k]))
                             for k in ("open_loop", "feedback", "feedback_sectors", "feedback_hidden")), steps, census["episodes"], census["reused"]))
    sys.exit(0)
env.close()

os.makedirs(args.out, exist_ok=True)
if args.hidden:
    with open(os.path.join(args.out, "feedback_hidden_bench.jsonl"), "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    ra, rb, rc = ([r["rate_M"] for r in rows if r["form"] == k] for k in ("feedback_sectors", "feedback_hidden", "per_step_hidden"))
    POLICY_LAUNCH = (75.0, 81.0)                               # the separate fused policy launch in the loop (README.md)
    with open(os.path.join(args.out, "README.md"), "w") as f:
        f.write("# Closed-loop launches: a hidden layer in the feedback law\n\n`python %s` on one MI355X, one process: %d environments x %d "
                "beams, 50 polygons, one chain, %d steps per launch, 9 x 20 sectors; %d alternating passes in one session, each form warmed by "
                "half a pass and timed by the host clock over %d steps ended by a synchronise.  Library sha256 `%s`.\n\n"
                "| form | M env-steps/s per pass | min | max |\n|---|---|---|---|\n" % (" ".join(sys.argv), n, env.n_sensors, T, args.passes, steps, sha))
        f.write("| (a) `step_feedback(los_gains, sector_gains=..., record=\"reward\")`, the sector launch | %s | %.1f | %.1f |\n"
                % (", ".join("%.1f" % x for x in ra), min(ra), max(ra)))
        f.write("| (b) `step_feedback(..., sector_gains=..., hidden=..., record=\"reward\")`, 16 relu units per environment | %s | %.1f | %.1f |\n"
                % (", ".join("%.1f" % x for x in rb), min(rb), max(rb)))
        f.write("| (c) one `step()` per step, the same law as torch ops on `env.obs` | %s | %.1f | %.1f |\n"
                % (", ".join("%.1f" % x for x in rc), min(rc), max(rc)))
        f.write("\n(b) / (a), pass by pass: %s.\n\nEvery run of (b) above every run of (c): **%s** (min (b) %.1f, max (c) %.1f).  Every run of (b) "
                "above the %.0f-%.0f M of the separate policy launch in the loop: **%s**.\n\nRaw rows: `feedback_hidden_bench.jsonl`.\n"
                % (", ".join("%.3f" % (y / x) for x, y in zip(ra, rb)), "yes" if min(rb) > max(rc) else "NO", min(rb), max(rc),
                   POLICY_LAUNCH[0], POLICY_LAUNCH[1], "yes" if min(rb) > POLICY_LAUNCH[1] else "NO"))
    sys.exit(0)
if args.sectors:
    with open(os.path.join(args.out, "feedback_sectors_bench.jsonl"), "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    a, b_ = [r["rate_M"] for r in rows if r["form"] == "feedback"], [r["rate_M"] for r in rows if r["form"] == "feedback_sectors"]
    with open(os.path.join(args.out, "feedback_sectors_bench.md"), "w") as f:
        f.write("`python %s`: %d environments x %d beams, %d steps per launch, %d alternating passes over %d steps.  Library sha256 `%s`.\n\n"
                "| form | M env-steps/s per pass | min | max |\n|---|---|---|---|\n" % (" ".join(sys.argv), n, env.n_sensors, T, args.passes, steps, sha))
        f.write("| `step_feedback(los_gains, record=\"reward\")` | %s | %.1f | %.1f |\n" % (", ".join("%.1f" % x for x in a), min(a), max(a)))
        f.write("| `step_feedback(los_gains, sector_gains=..., record=\"reward\")` | %s | %.1f | %.1f |\n" % (", ".join("%.1f" % x for x in b_), min(b_), max(b_)))
        f.write("\nsectors / without, pass by pass: %s.\n" % ", ".join("%.3f" % (y / x) for x, y in zip(a, b_)))
    sys.exit(0)
with open(os.path.join(args.out, "feedback_bench.jsonl"), "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
rate = {name: [r["rate_M"] for r in rows if r["form"] == name] for name, _ in FORMS}
with open(os.path.join(args.out, "README.md"), "w") as f:
    f.write("# Closed-loop launches: the action chosen inside a launch of several steps\n\n`python %s` on one MI355X, one process: %d "
            "environments x %d beams, 50 polygons, one chain, %d steps per launch; %d alternating passes, each form warmed by half a pass "
            "and timed by the host clock over %d steps ended by a synchronise.  Library sha256 `%s`.\n\n"
            "| form | M env-steps/s per pass | min | max |\n|---|---|---|---|\n" % (" ".join(sys.argv), n, env.n_sensors, T, args.passes, steps, sha))
    what = dict(open_loop="(a) `step_multi(record=\"reward\")`, open loop", feedback="(b) `step_feedback(los_gains, record=\"reward\")`",
                per_step="(c) one `step()` per step, the law as torch ops on `env.obs`")
    for name, _ in FORMS:
        f.write("| %s | %s | %.1f | %.1f |\n" % (what[name], ", ".join("%.1f" % x for x in rate[name]), min(rate[name]), max(rate[name])))
    f.write("\n(b) / (a), pass by pass: %s.  Every run of (b) above every run of (c): **%s** (min (b) %.1f, max (c) %.1f).\n\nRaw rows: "
            "`feedback_bench.jsonl`.\n" % (", ".join("%.3f" % (x / y) for x, y in zip(rate["feedback"], rate["open_loop"])),
                                           "yes" if min(rate["feedback"]) > max(rate["per_step"]) else "NO", min(rate["feedback"]),
                                           max(rate["per_step"])))
    curve = os.path.join(args.out, "ars_curve.jsonl")
    if os.path.exists(curve):
        pts = [json.loads(x) for x in open(curve) if x.strip()]
        its = [p for p in pts if "iteration" in p]
        f.write("\n## ARS (V1) of a 2 x 7 linear policy, PathFollow (`examples/ars.py`)\n\nOne run, as it came out; no learning result is "
                "claimed.  `%s`\n\n| iteration | mean return | mean progress | M env-steps/s |\n|---|---|---|---|\n" % pts[0].get("command", ""))
        keep = sorted(set(list(range(0, len(its), max(1, len(its) // 20))) + [len(its) - 1])) if its else []
        for i in keep:
            p = its[i]
            f.write("| %d | %.3f | %.4f | %.1f |\n" % (p["iteration"], p["mean_return"], p["mean_progress"], p.get("rate_M", float("nan"))))
        f.write("\nEvery iteration: `ars_curve.jsonl`.\n")
