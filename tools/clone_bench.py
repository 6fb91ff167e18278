#!/usr/bin/env python3
"""The supervised (clone) step of the fused updater, measured against its neighbours in one session:

  clone   FusedPPOUpdate.clone_step (k8_clone + the weight-gradient pass, the reduction, the norm, Adam)
  (a)     the eager torch step: clone_loss_terms on gathered rows, backward, torch.optim.Adam
  (b)     FusedPPOUpdate.step, the fused PPO step on the same rows
  (c)     decisions per second of examples/distill.py's loop with the fused step, and with the eager step (--loop 1)

16384 rows of obs_dim 186 by default.  Every timed window follows a warm-up of the same shape and ends in a device synchronise; the
variants alternate, `--repeats` windows each, and the median window is reported.  Prints one JSON line per hidden-width triple of
--arch H1,H2,H3[:H1,H2,H3...] (gym_auv_amd.ppo_update.SUPPORTED_HIDDEN; default the reference's); `--passes` goes through the list again.

    python tools/clone_bench.py --rows 16384 --obs-dim 186 --steps 200 --repeats 5 --loop 1
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3                   # ms per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--obs-dim", type=int, default=186)
    ap.add_argument("--steps", type=int, default=200, help="steps per timed window")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kind", default="nll", choices=["nll", "mse"])
    ap.add_argument("--loop", type=int, default=0, help="1: also time examples/distill.py's loop with the fused and with the eager step")
    ap.add_argument("--loop-decisions", type=int, default=100)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--arch", default="256,128,64", metavar="H1,H2,H3[:H1,H2,H3...]", help="hidden widths; several separated by ':'")
    ap.add_argument("--passes", type=int, default=1, help="times the list of widths is gone through")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clone_bench measures on the GPU: none is visible")
    for k in range(a.passes):
        for s in a.arch.split(":"):
            res = measure(a, tuple(int(x) for x in s.split(",")))
            res["pass"] = k
            print(json.dumps(res), flush=True)


def measure(a, arch):
    import copy
    import ppo
    from gym_auv_amd.ppo_update import FusedPPOUpdate, clone_loss_terms
    dev, B, D = a.device, a.rows, a.obs_dim
    torch.manual_seed(0)
    net = ppo.ActorCritic(D, hidden=arch).to(dev)
    twin = copy.deepcopy(net)
    O, A, RET = torch.randn(B, D, device=dev), 0.5 * torch.randn(B, 2, device=dev), torch.randn(B, device=dev)
    W = torch.rand(B, device=dev) + 0.5
    with torch.no_grad():
        LP = net.log_prob(net.pi(O), A).contiguous()
    ADV = torch.randn(B, device=dev)
    idx = torch.randperm(B, device=dev)
    upd = FusedPPOUpdate(net, lr=1e-5, max_batch=B)
    opt = torch.optim.Adam(twin.parameters(), lr=1e-5)

    def eager():
        opt.zero_grad()
        clone_loss_terms(twin, O[idx], A[idx], RET[idx], W[idx], a.kind, 0.5, 0.01)[0].backward()
        opt.step()
    variants = {"clone_step_ms": lambda: upd.clone_step(O, A, RET, W, idx, kind=a.kind),
                "ppo_step_ms": lambda: upd.step(O, A, LP, ADV, RET, idx),
                "eager_clone_step_ms": eager}
    for fn in variants.values():
        window(fn, a.warmup)
    times = {k: [] for k in variants}
    for _ in range(a.repeats):
        for k, fn in variants.items():
            times[k].append(window(fn, a.steps if k != "eager_clone_step_ms" else max(10, a.steps // 10)))
    res = dict(rows=B, obs_dim=D, arch=list(arch), kind=a.kind, steps=a.steps, repeats=a.repeats)
    for k, v in times.items():
        res[k] = statistics.median(v)
        res[k.replace("_ms", "_spread")] = (max(v) - min(v)) / statistics.median(v)
    res["clone_over_ppo"] = res["clone_step_ms"] / res["ppo_step_ms"]
    res["eager_over_clone"] = res["eager_clone_step_ms"] / res["clone_step_ms"]
    res["nonfinite_inputs"] = float(upd.log[:min(upd.n_steps, upd.LOG_ROWS), 5].sum())
    if a.loop:
        import distill
        for eager_step in (False, True):                              # warm-up: every kernel of either loop has run once
            distill.run(decisions=20, eager=eager_step, eval_steps=50, log=lambda *_: None, net_arch=arch)
        for name, eager_step in (("fused", False), ("eager", True)):
            r = distill.run(decisions=a.loop_decisions, eager=eager_step, eval_steps=50, log=lambda *_: None, net_arch=arch)
            res["loop_decisions_per_s_" + name] = r["decisions_per_s"]
            res["loop_clone_steps_" + name] = r["clone_steps"]
    return res


if __name__ == "__main__":
    main()
