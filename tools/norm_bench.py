#!/usr/bin/env python3
"""Cost of running normalisation in the fused rollout (csrc/k16_policy_norm.hip) against the plain launch of the SAME build:
tools/norm_bench.py [envs] [--passes=P] [--chains=K] [--arch=H1,H2,H3]
4096 x 186, four chains, hidden widths [256, 128, 64] and [64, 64, 64] unless --arch names one.  Per width, P alternating passes (plain,
norm, plain, norm, ...) in ONE session, each pass: rollouts of T = 128 steps -- env-steps/s by the wall clock around synchronised rollout
calls -- and the launch alone by HIP events (every chain's launch once per sample, back to back).  Then the fold's and the return pass's
time per T = 128 rollout by HIP events.  Every line is JSON and carries the first 12 hex digits of the loaded library's sha256."""
import hashlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import ppo  # noqa: E402
from gym_auv_amd import _capi  # noqa: E402
from gym_auv_amd.batched_env import BatchedAuvEnv  # noqa: E402
from gym_auv_amd.config import effective_reference_config  # noqa: E402
from gym_auv_amd.devgen import GeneratedWorlds  # noqa: E402
from gym_auv_amd.normalize import RunningNorm  # noqa: E402
from gym_auv_amd.policy import FusedActorCritic  # noqa: E402

OPT = dict(a[2:].split("=", 1) for a in sys.argv if a.startswith("--") and "=" in a)
argv = [a for a in sys.argv if not a.startswith("--")]
N = int(argv[1]) if len(argv) > 1 else 4096
PASSES, CHAINS = int(OPT.get("passes", 3)), int(OPT.get("chains", 4))
ARCHS = [tuple(int(x) for x in OPT["arch"].split(","))] if "arch" in OPT else [(256, 128, 64), (64, 64, 64)]
T, ROLLOUTS, SAMPLES = 128, 4, 200
LIB_HASH = hashlib.sha256(open(os.environ.get("AUV_HIP_LIB") or _capi.LIB_PATH, "rb").read()).hexdigest()[:12]
DEV = "cuda:0"


def make(arch, normalize):
    cfg = effective_reference_config(use_lidar=True)
    env = BatchedAuvEnv(cfg, GeneratedWorlds(2 * N, 17, 11, seed=1), N, device=DEV)
    env.reset()
    env.set_sub_batches(CHAINS)
    torch.manual_seed(0)
    net = ppo.ActorCritic(env.obs_dim, hidden=arch).to(DEV)
    norm = RunningNorm(env.obs_dim, 0.999) if normalize else None
    return env, FusedActorCritic(net, env, rollout=T, reward_scale=0.01, normalize=norm), norm


def rollout_rate(env, fused):
    fused.begin_rollout()
    fused.rollout(16, flush=False)                          # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ROLLOUTS):
        fused.begin_rollout()
        fused.rollout(T)
        torch.cuda.synchronize()
    return ROLLOUTS * T * env.n_envs / (time.perf_counter() - t0)


def launch_us(env, fused):
    """Every chain's act launch once per sample, on the chains' streams, by HIP events on chain 0 around a joined sample."""
    k = env.sub_batches
    cur = torch.cuda.current_stream(DEV)
    fused.begin_rollout()
    for i in range(k):
        fused.act(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(cur)
    for s in range(SAMPLES):
        if s % (T - 1) == 0:
            fused.begin_rollout()
        for i in range(k):
            env._sub_streams[i].wait_stream(cur)
            fused.act(i)
        for i in range(k):
            cur.wait_stream(env._sub_streams[i])
    e1.record(cur)
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / SAMPLES


def event_us(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


for arch in ARCHS:
    plain = make(arch, False)
    normd = make(arch, True)
    for p in range(PASSES):
        for name, (env, fused, norm) in (("plain", plain), ("norm", normd)):
            rate = rollout_rate(env, fused)
            us = launch_us(env, fused)
            if norm is not None:
                norm.fold()                                 # (the table moves as it would in training)
                torch.cuda.synchronize()
            print(json.dumps(dict(kind="pass", arch=list(arch), envs=N, obs_dim=env.obs_dim, chains=env.sub_batches, launch=name, pass_=p,
                                  env_steps_per_s=round(rate), launch_us_all_chains=round(us, 2), lib=LIB_HASH)), flush=True)
    env, fused, norm = normd
    fused.begin_rollout()
    fused.rollout(T)
    torch.cuda.synchronize()
    part, pcnt = norm.pcnt.clone(), None

    def fold():
        norm.pcnt.copy_(part)                               # (fold() empties the slots: refill them, inside the timing -- a 4 KB copy)
        norm.fold()
    R0 = fused.R.clone()

    def returns():
        norm.returns(R0, fused.Dn, out=fused.R)
    print(json.dumps(dict(kind="between_rollouts", arch=list(arch), envs=N, T=T, slots=int(norm.pcnt.numel()), fold_us=round(event_us(fold), 2),
                          returns_us=round(event_us(returns), 2), lib=LIB_HASH)), flush=True)
    for e in (plain[0], normd[0]):
        e.close()
