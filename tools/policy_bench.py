#!/usr/bin/env python3
"""Time of the fused policy launch alone (csrc/k6_policy.hip) and of policy + environment step chains:
tools/policy_bench.py [envs] [bf16] [--feasibility-pooling] [--quick] [--arch=H1,H2,H3] [--chains=K] [--squash=1]
--squash=1: the tanh-squashed launches (auv_policy_act_squash / _rollout_squash) in the plain ones' place; --feasibility-pooling: the observation pooled to 9 sectors (obs_dim 15 instead of 186); --quick: one chain only; --chains=K: K chains only;
--arch: the hidden widths of both nets, one of gym_auv_amd.policy.SUPPORTED_HIDDEN (default 256,128,64).  Every line ends with the first
12 hex digits of the loaded library's sha256 (AUV_HIP_LIB selects another build)."""
import hashlib
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import ppo  # noqa: E402
from gym_auv_amd.batched_env import BatchedAuvEnv  # noqa: E402
from gym_auv_amd.config import effective_reference_config  # noqa: E402
from gym_auv_amd.devgen import GeneratedWorlds  # noqa: E402
from gym_auv_amd.policy import FusedActorCritic  # noqa: E402

from gym_auv_amd import _capi  # noqa: E402

POOL, QUICK = "--feasibility-pooling" in sys.argv, "--quick" in sys.argv
OPT = dict(a[2:].split("=", 1) for a in sys.argv if a.startswith("--") and "=" in a)
ARCH = tuple(int(x) for x in OPT.get("arch", "256,128,64").split(","))
SQUASH = OPT.get("squash", "0") == "1"
CHAINS = (int(OPT["chains"]),) if "chains" in OPT else ((1,) if QUICK else (1, 2, 4))
LIB_HASH = hashlib.sha256(open(os.environ.get("AUV_HIP_LIB") or _capi.LIB_PATH, "rb").read()).hexdigest()[:12]
argv = [a for a in sys.argv if not a.startswith("--")]
n = int(argv[1]) if len(argv) > 1 else 4096
cfg = effective_reference_config(use_lidar=True)
cfg.vessel.sensor_use_feasibility_pooling = POOL
BF16 = len(argv) > 2 and argv[2] == "bf16"
for k in CHAINS:
    env = BatchedAuvEnv(cfg, GeneratedWorlds(2 * n, 17, 11, seed=1), n, device="cuda:0")
    env.reset()
    env.set_sub_batches(k)
    net = ppo.ActorCritic(env.obs_dim, hidden=ARCH).to("cuda:0")
    T = 256
    fused = FusedActorCritic(net, env, rollout=T, reward_scale=0.01, bf16=BF16, squash=SQUASH)
    # the policy launch alone, back to back on each chain's stream
    fused.begin_rollout()
    for _ in range(3):
        for i in range(env.sub_batches):
            fused.act(i)
    torch.cuda.synchronize()
    fused.begin_rollout()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        for i in range(env.sub_batches):
            fused.act(i)
    torch.cuda.synchronize()
    t_pol = (time.perf_counter() - t0) / 200
    # policy + step chains
    fused.begin_rollout()
    fused.rollout(16, flush=False)
    torch.cuda.synchronize()
    fused.begin_rollout()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fused.rollout(T)
    t_host = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_roll = (time.perf_counter() - t0) / T
    print("%sarch %s envs %d obs_dim %d chains %d: policy launches alone %.1f us per full step; policy + env step %.1f us per step = %.1f M env-steps/s "
          "(host enqueue %.1f us per step) lib %s" % ("squash " if SQUASH else "", "-".join(str(x) for x in ARCH), n, env.obs_dim, env.sub_batches, 1e6 * t_pol, 1e6 * t_roll,
                                                     n / t_roll / 1e6, 1e6 * t_host / T, LIB_HASH), flush=True)
    env.close()
