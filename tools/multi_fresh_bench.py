#!/usr/bin/env python3
"""A fresh world on every reset in 64-step launches against the two loops it sits between, in ONE session:
python tools/multi_fresh_bench.py [envs] [--depth=3[,4,...]] [--chains=3] [--batch-cap=256] [--steps=3840] [--passes=5]
Workload moving28 (17 movers + 11 circles, built on the device), `envs` (4096) environments x the default 180 sensors, i.i.d.
uniform actions from a ring of 64 slots, open loop.  The loops, alternating, `passes` timed passes of `steps` steps each:
  fresh_multi_d<D>   64 steps per launch, FreshWorlds(depth=D, multi_step=True), one pass of up to `batch-cap` worlds per launch
  bank_multi         the same launches over a cycling generated bank of two worlds per environment (what the headline measures)
  fresh_one_step     today's fresh-world loop: one step per launch (step_pipelined), FreshWorlds(depth=3), a pass every 16 steps
All on `chains` sub-batch chains (the fresh handles put their passes on one further stream).  One JSON line per loop: the median
and every pass's env-steps/s, `reused` / `regenerated` / `queued` (fresh_stats after the last pass), episodes finished, health;
the first line names the library's sha256."""
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gym_auv_amd import _capi  # noqa: E402
from gym_auv_amd.batched_env import BatchedAuvEnv  # noqa: E402
from gym_auv_amd.config import effective_reference_config  # noqa: E402
from gym_auv_amd.devgen import FreshWorlds, GeneratedWorlds  # noqa: E402


def opt(name, default):
    for a in sys.argv[1:]:
        if a.startswith("--%s=" % name):
            return a.split("=", 1)[1]
    return default


argv = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(argv[0]) if argv else 4096
depths = [int(x) for x in opt("depth", "3").split(",")]
chains, cap, steps, passes = int(opt("chains", 3)), int(opt("batch-cap", 256)), int(opt("steps", 3840)), int(opt("passes", 5))
T, slots = 64, 64
dev = torch.device("cuda:0")
cfg = effective_reference_config(use_lidar=True)
ring = torch.rand((slots, n, 2), device=dev) * torch.tensor([2.0, 0.3], device=dev) - torch.tensor([1.0, 0.15], device=dev)


def make(spec):
    env = BatchedAuvEnv(cfg, spec, n, device=dev, auto_reset=True)
    env.reset()
    env.set_sub_batches(chains)
    return env


def multi(env):
    def run(m):
        for i in range(0, m, T):
            env.step_multi(ring, i % slots, T)
    return run


def one_step(env):
    def run(m):
        for i in range(m):
            env.step_pipelined(ring[i % slots])
    return run


loops = []
for D in depths:
    e = make(FreshWorlds(depth=D, seed=1000, batch_cap=cap, period=16, multi_step=True))
    loops.append(("fresh_multi_d%d" % D, e, multi(e), T))
e = make(GeneratedWorlds(2 * n, seed=1000))
loops.append(("bank_multi", e, multi(e), T))
e = make(FreshWorlds(depth=3, seed=1000))
loops.append(("fresh_one_step", e, one_step(e), 1))

print(json.dumps(dict(lib_sha256=hashlib.sha256(open(_capi.LIB_PATH, "rb").read()).hexdigest(), envs=n, n_sensors=loops[0][1].n_sensors,
                      steps_per_pass=steps, passes=passes, chains=chains)), flush=True)
rates = {name: [] for name, _, _, _ in loops}
for name, env, run, _ in loops:                 # warm-up: past the first turn-overs, the passes running
    run(steps)
    torch.cuda.synchronize()
for p in range(passes):
    for name, env, run, _ in loops:
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        rates[name].append(n * steps / (time.perf_counter() - t0) / 1e6)
for name, env, run, per in loops:
    r = sorted(rates[name])
    st = env.fresh_stats()
    print(json.dumps(dict(loop=name, steps_per_launch=per, chains=env.sub_batches, rate_M=round(r[len(r) // 2], 1), passes_M=[round(x, 1) for x in rates[name]],
                          reused=st["reused"], regenerated=st["regenerated"], queued=st["queued"], passes_issued=st["passes_issued"],
                          depth=st["depth"], batch_cap=st["batch_cap"], episodes=int(env.read("COUNTERS")[:, 2].sum()), health=env.health())), flush=True)
    env.close()
