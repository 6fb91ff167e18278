#!/usr/bin/env python3
"""What the fused policy evaluation (auv_policy_eval, csrc/k9_policy_eval.hip) costs beside the eager torch modules it replaces
outside a rollout (measured, not gated by a test):
    python tools/policy_eval_bench.py [--out profiles/policy_eval] [--skip-plan]
One process.  HIP events on the stream the calls run on, 10 warm-up calls, then 60 timed calls: median, min, p90, in microseconds.
  launch times   value only, policy only (mean + action) and both, at M in {1024, 4096, 65536} rows and obs_dim in {15, 186};
                 the baseline is eager net.v(obs) / net.pi(obs) / both on the same rows in the same process and session.
  acceptance     the fused median is below the eager median of the same session at every shape measured (eager is a dozen launches
                 for the same arithmetic: no extra margin is claimed; the ratio is written down whatever it is).
  plan cost      ShootingPlanner.plan() at 64 real x 64 candidates, horizon 16 (the shape of tools/plan_bench.py) with value=None,
                 value=<FusedActorCritic> and value=<eager torch callable>: wall clock over >= 1.5 s of back-to-back plans.
Writes README.md and policy_eval_bench.jsonl under --out, with the library's sha256."""
import argparse
import hashlib
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_auv_amd import _capi, planning  # noqa: E402
from gym_auv_amd.policy import pack_policy_params, policy_eval  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/policy_eval")
ap.add_argument("--skip-plan", action="store_true")
ap.add_argument("--rows", default="1024,4096,65536")
ap.add_argument("--obs-dims", default="15,186")
args = ap.parse_args()
dev = torch.device("cuda:0")
WARM, REPS = 10, 60


def timed(fn):
    """(median, min, p90) of REPS event-timed calls of fn() on the current stream after WARM calls, in microseconds"""
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(out)), float(np.min(out)), float(np.percentile(out, 90))


import ppo  # noqa: E402  (examples/ppo.py: the torch modules)

bank = None
if not args.skip_plan:                                     # (the bank's worker processes start before this process opens the GPU)
    from gym_auv_amd.world import build_bank_parallel
    bank = build_bank_parallel("moving_obstacles_world", 1000 + np.arange(128), procs=16)

sha = hashlib.sha256(open(os.environ.get("AUV_HIP_LIB") or _capi.LIB_PATH, "rb").read()).hexdigest()   # (the library the loader picks)
rows = []
ok = True
with torch.no_grad():
    for D in [int(x) for x in args.obs_dims.split(",")]:
        torch.manual_seed(D)
        net = ppo.ActorCritic(D).to(dev)
        params = pack_policy_params(net, D)
        for M in [int(x) for x in args.rows.split(",")]:
            X = torch.rand((M, D), device=dev) * 2 - 1
            o = dict(mu=torch.empty((M, 2), device=dev), action=torch.empty((M, 2), device=dev), value=torch.empty(M, device=dev))
            cases = (("value", ("value",), lambda: net.v(X)),
                     ("policy", ("mu", "action"), lambda: net.pi(X)),
                     ("both", ("mu", "action", "value"), lambda: (net.pi(X), net.v(X))))
            for name, want, eager in cases:
                out = {w: o[w] for w in want}
                f = timed(lambda: policy_eval(params, D, X, want=want, out=out))
                e = timed(eager)
                row = dict(kind="launch", what=name, obs_dim=D, M=M, fused_us_median=f[0], fused_us_min=f[1], fused_us_p90=f[2],
                           eager_us_median=e[0], eager_us_min=e[1], eager_us_p90=e[2], eager_over_fused=e[0] / f[0], lib_sha256=sha)
                ok = ok and f[0] < e[0]
                rows.append(row)
                print(json.dumps(row), flush=True)

plan_rows = []
if not args.skip_plan:
    from gym_auv_amd.batched_env import BatchedAuvEnv
    from gym_auv_amd.config import effective_reference_config
    from gym_auv_amd.policy import FusedActorCritic
    B, K, T = 64, 64, 16
    cfg = effective_reference_config(use_lidar=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        real = BatchedAuvEnv(cfg, bank, B, device=dev, auto_reset=True)
    real.reset()
    warm = torch.rand((20, B, 2), device=dev) * torch.tensor([2.0, 0.3], device=dev) - torch.tensor([1.0, 0.15], device=dev)
    for t in range(20):
        real.step(warm[t])
    torch.manual_seed(0)
    net = ppo.ActorCritic(real.obs_dim).to(dev)
    fused = FusedActorCritic(net, real, rollout=1)

    def eager_value(obs):
        with torch.no_grad():
            return net.v(obs).squeeze(-1)
    for name, value in (("none", None), ("fused", fused), ("eager", eager_value)):
        planner = planning.ShootingPlanner(real, candidates=K, horizon=T, gamma=0.99, seed=1, value=value, value_scale=100.0)
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
        row = dict(kind="plan", value=name, real_envs=B, candidates=K, horizon=T, plans_per_s=rate, plan_us=1e6 / rate, lib_sha256=sha,
                   health=planner.sim.health())
        plan_rows.append(row)
        print(json.dumps(row), flush=True)
        planner.close()
    real.close()

os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, "policy_eval_bench.jsonl"), "w") as f:
    for r in rows + plan_rows:
        f.write(json.dumps(r) + "\n")
with open(os.path.join(args.out, "README.md"), "w") as f:
    f.write("# Fused policy evaluation on arbitrary rows against the eager torch modules\n\n`python tools/policy_eval_bench.py` on one MI355X, one "
            "process.  Library sha256 `%s`.\n\nHIP events on the stream the calls run on, %d warm-up calls, median / min / p90 of %d calls, in "
            "microseconds.  `fused`: one `auv_policy_eval` launch through `policy.policy_eval` (the Python binding's validation included).  "
            "`eager`: `net.v(X)`, `net.pi(X)` or both under `torch.no_grad()`, same rows, same session.  `policy` asks for the mean and the "
            "deterministic action.\n\n"
            "| what | obs_dim | M | fused median | min | p90 | eager median | min | p90 | eager / fused |\n|---|---|---|---|---|---|---|---|---|---|\n"
            % (sha, WARM, REPS))
    for r in rows:
        f.write("| %s | %d | %d | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.2f |\n"
                % (r["what"], r["obs_dim"], r["M"], r["fused_us_median"], r["fused_us_min"], r["fused_us_p90"], r["eager_us_median"],
                   r["eager_us_min"], r["eager_us_p90"], r["eager_over_fused"]))
    f.write("\nAcceptance (the fused median below the eager median of the same session at every shape): **%s**.\n" % ("met" if ok else "NOT met"))
    if plan_rows:
        f.write("\n## A plan with a terminal value\n\n`ShootingPlanner.plan()` at 64 real x 64 candidates (4096 planner rows), horizon 16, 186 columns; "
                "wall clock over >= 1.5 s of back-to-back plans ended by a synchronise.\n\n| terminal value | plan us | plans/s |\n|---|---|---|\n")
        for r in plan_rows:
            f.write("| %s | %.1f | %.0f |\n" % (r["value"], r["plan_us"], r["plans_per_s"]))
    else:
        f.write("\nPlan cost: not measured in this run (`--skip-plan`).\n")
    f.write("\nRaw rows: `policy_eval_bench.jsonl`.\n")
sys.exit(0 if ok else 1)
