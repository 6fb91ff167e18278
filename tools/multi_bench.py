#!/usr/bin/env python3
"""Open-loop rate with SEVERAL steps per launch (auv_step_multi) against one step per launch, by chains and launch length:
python tools/multi_bench.py [workload polygons50|moving28] [envs] [--feasibility-pooling] [--quick] [--record | --record=reward]
--feasibility-pooling: the observation pooled to 9 sectors (VesselConfig.sensor_use_feasibility_pooling);
--quick: one chain only, one step per launch and 64-step launches in cohort order;
--record: the launches of several steps keep every step's obs / reward / done in a preallocated [T][N] buffer
(auv_step_multi_record); --record=reward: reward and done only.  The one-step-per-launch row is the same loop either way: it
hands out every step already."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_auv_amd.batched_env import BatchedAuvEnv  # noqa: E402
from gym_auv_amd.config import effective_reference_config  # noqa: E402
from gym_auv_amd.world import build_bank_parallel  # noqa: E402

POOL, QUICK = "--feasibility-pooling" in sys.argv, "--quick" in sys.argv
RECORD = "obs" if "--record" in sys.argv else ("reward" if "--record=reward" in sys.argv else None)
argv = [a for a in sys.argv if not a.startswith("--")]
wl = argv[1] if len(argv) > 1 else "polygons50"
n = int(argv[2]) if len(argv) > 2 else 4096
dev = torch.device("cuda:0")
cfg = effective_reference_config(use_lidar=True)
cfg.vessel.sensor_use_feasibility_pooling = POOL
gen, kw = ("polygon_world", dict(n_polygons=50)) if wl == "polygons50" else ("moving_obstacles_world", dict())
cache = "/tmp/multi_bench_%s_%d.npz" % (wl, n)
if os.path.exists(cache):
    z = np.load(cache)
    bank = {k: (z[k] if z[k].ndim else z[k].item()) for k in z.files}
else:
    bank = build_bank_parallel(gen, 1000 + np.arange(2 * n), procs=16, **kw)
    np.savez(cache, **bank)
slots = 64
ring = torch.rand((slots, n, 2), device=dev) * torch.tensor([2.0, 0.3], device=dev) - torch.tensor([1.0, 0.15], device=dev)
for k in ((1,) if QUICK else (1, 2, 4)):
    env = BatchedAuvEnv(cfg, bank, n, device=dev, auto_reset=True)
    env.reset()
    env.set_sub_batches(k, strict=True)
    steps = 1920
    rec = None
    if RECORD:
        rec = (torch.zeros((64, n, env.obs_dim), dtype=torch.float32, device=dev) if RECORD == "obs" else None,
               torch.zeros((64, n), dtype=torch.float32, device=dev), torch.zeros((64, n), dtype=torch.uint8, device=dev))
        torch.cuda.synchronize()
    shapes = ((0, "-"), (64, "cohorts")) if QUICK else \
        ((0, "-"), (8, "steps"), (64, "steps"), (8, "cohorts"), (16, "cohorts"), (64, "cohorts"), (64, "cohorts:6:16"), (64, "cohorts:20:40"))
    for T, order in shapes:
        if T:
            o = order.split(":")
            env.set_multi_order(o[0], *([int(o[1]), int(o[2])] if len(o) > 1 else []))
        def run(m):
            if T == 0:
                for i in range(m):
                    env.step_pipelined(ring[i % slots])
            else:
                for i in range(0, m, T):
                    env.step_multi(ring, i % slots, T, record=rec and (rec[0] if rec[0] is None else rec[0][:T], rec[1][:T], rec[2][:T]))
        run(steps // 2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps(dict(workload=wl, envs=n, pooled=POOL, obs_dim=env.obs_dim, chains=k, steps_per_launch=T or 1, order=order, record=RECORD if T else None, rate_M=round(n * steps / dt / 1e6, 1), us_per_step=round(1e6 * dt / steps, 2),
                              health=env.health())), flush=True)
    env.close()
