#!/usr/bin/env python3
"""Cost of frame stacking in the fused policy rollout (csrc/k12_policy_stacked.hip) against the plain launch it is built from:
tools/framestack_bench.py [envs] [--chains K] [--steps T] [--passes P] [--quick] [--arch H1,H2,H3[:H1,H2,H3...]] [--only v1,v2,...]

One process is ONE session: every variant is built once and then measured in P alternating passes (variant after variant, pass after
pass), so that drift of the machine lands on all of them alike.  Per variant and pass, one JSON line:
  env_steps_per_s   a rollout of T steps of every chain, policy launch + environment step (wall clock around one C call)
  policy_us         the policy launch alone, 200 launches back to back on each chain's stream, by HIP events, per full step
Variants:
  parent      auv_policy_rollout, the plain launch (k6_policy_act)
  stacked_k1  auv_policy_rollout_stacked with frames = 1: the new kernel on the same rows -- the cost of the kernel itself
  stacked_k2, stacked_k4   frames = 2, 4: nets of 2 x and 4 x the input width, the history read and O written by the launch
  stacked_k4_no_O          frames = 4 without the rollout's O (store_obs=False): the launch minus 12 MB of stores per step
  eval_k4     policy_us only: auv_policy_eval (mean and value) on resident [N, 4 x obs_dim] rows -- the 4 x wider nets' matrix work and
              weight traffic with no history read and no O write: what of stacked_k4's launch the WEIGHTS explain
  torch_k2, torch_k4       the alternative in stock tensor operations: per step and chain a ring write, a gather of the older frames, the
              age mask and a cat into the row buffer, in front of the PLAIN launch and the environment's step.  The launch still runs the
              one-frame net, so this is a LOWER bound of that alternative (its first layer would be k times wider on top).
--arch: hidden widths of the nets (gym_auv_amd.policy.SUPPORTED_HIDDEN); several, separated by ':', are measured side by side in the same
passes, every variant once per triple (its name then ends in @H1-H2-H3).  --only: these variants only.  Every line carries the first 12
hex digits of the loaded library's sha256.
The last line summarises: median and min .. max over the passes.  Shape: 4096 x 180 beams, a fresh world on every reset, the chains of
tools/policy_bench.py.  tools/framestack_bench.sh runs it under a time limit."""
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import ppo  # noqa: E402
from gym_auv_amd import _capi  # noqa: E402
from gym_auv_amd.batched_env import BatchedAuvEnv, _LIB, _check  # noqa: E402
from gym_auv_amd.config import effective_reference_config  # noqa: E402
from gym_auv_amd.devgen import FreshWorlds  # noqa: E402
from gym_auv_amd.policy import FusedActorCritic  # noqa: E402


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


QUICK = "--quick" in sys.argv
pos_args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and not sys.argv[i - 1].startswith("--")]
N = int(pos_args[0]) if pos_args else 4096
CHAINS, T, PASSES = arg("--chains", 4), arg("--steps", 64 if QUICK else 256), arg("--passes", 2 if QUICK else 5)
DEV = "cuda:0"
ARCHS = [tuple(int(x) for x in t.split(",")) for t in (sys.argv[sys.argv.index("--arch") + 1] if "--arch" in sys.argv else "256,128,64").split(":")]
ONLY = sys.argv[sys.argv.index("--only") + 1].split(",") if "--only" in sys.argv else None
LIB_HASH = hashlib.sha256(open(os.environ.get("AUV_HIP_LIB") or _capi.LIB_PATH, "rb").read()).hexdigest()[:12]


class Variant:
    def __init__(self, name, frames, mode, store_obs=True, arch=(256, 128, 64)):
        self.name, self.frames, self.mode, self.arch = name, frames, mode, arch
        cfg = effective_reference_config(use_lidar=True)
        self.env = env = BatchedAuvEnv(cfg, FreshWorlds(n_moving=17, n_static=11, seed=1000), N, device=DEV)
        env.reset()
        env.set_sub_batches(CHAINS)
        torch.manual_seed(0)
        k_net = frames if mode in ("stacked", "eval") else 1
        net = ppo.ActorCritic(k_net * env.obs_dim, hidden=arch).to(DEV)
        self.fused = f = FusedActorCritic(net, env, rollout=T, reward_scale=0.01, frames=k_net, store_obs=store_obs)
        self.sios = None
        if mode == "stacked" and frames == 1:
            # the stacked export on one frame: the plain io blocks with no history behind them
            self.sios = (_capi.AuvPolicyStack * len(f.slices))()
            for i in range(len(f.slices)):
                self.sios[i].io, self.sios[i].hist, self.sios[i].stk, self.sios[i].frames = f._ios[i], None, None, 1
        if mode == "eval":
            from gym_auv_amd.policy import policy_eval
            rows = torch.randn((N, k_net * env.obs_dim), device=DEV)
            outs = dict(mu=torch.empty((N, 2), device=DEV), value=torch.empty(N, device=DEV))
            self.eval_once = lambda: policy_eval(f.params, k_net * env.obs_dim, rows, want=("mu", "value"), out=outs, hidden=arch)
        if mode == "torch":
            D = env.obs_dim
            self.ring = torch.zeros((frames, N, D), device=DEV)
            self.age = torch.zeros(N, dtype=torch.int64, device=DEV)
            self.rows = torch.zeros((N, frames * D), device=DEV)
            self.pos = 0

    # ---- one policy launch of chain i on its stream
    def act(self, i):
        f = self.fused
        if self.sios is not None:
            lo, cnt = f.slices[i]
            _check(_LIB.auv_policy_act_stacked_arch(self.env._h, lo, cnt, C.byref(self.sios[i]), C.byref(_capi.AuvPolicyArch(*self.arch)),
                                                    C.c_void_p(self.env._sub_streams[i].cuda_stream)), "auv_policy_act_stacked_arch")
            f._t[i], f._g[i] = min(f._t[i] + 1, T + 1), f._g[i] + 1
        else:
            f.act(i)

    def torch_rows(self, i, pos):
        """The stacked rows of chain i in stock tensor operations (enqueued on the current stream)."""
        lo, cnt = self.fused.slices[i]
        env, k, D = self.env, self.frames, self.env.obs_dim
        sl = slice(lo, lo + cnt)
        age = torch.where(env.done[sl] != 0, torch.zeros_like(self.age[sl]), self.age[sl]).add_(1).clamp_(max=k)
        self.age[sl] = age
        old = [torch.where((age > j).unsqueeze(1), self.ring[(pos - j) % k, sl], torch.zeros((), device=DEV)) for j in range(1, k)]
        torch.cat([env.obs[sl]] + old, 1, out=self.rows[sl])
        self.ring[pos, sl] = env.obs[sl]

    def rollout(self):
        f, env = self.fused, self.env
        if self.mode == "eval":
            self.eval_once()
            return
        f.begin_rollout()
        if self.mode == "torch":
            for t in range(T):
                if t % 16 == 0:
                    env.refill()                           # (a loop that steps slice by slice: the library cannot tick by itself)
                self.pos = (self.pos + 1) % self.frames
                for i in range(env.sub_batches):
                    with torch.cuda.stream(env._sub_streams[i]):
                        self.torch_rows(i, self.pos)
                        f.act(i)
                        env.step_slice(i, f.actions)
            for i in range(env.sub_batches):
                f.act(i)
        elif self.sios is not None:
            k = len(f.slices)
            t0, g0 = (C.c_int64 * k)(*f._t), (C.c_int64 * k)(*f._g)
            _check(_LIB.auv_policy_rollout_stacked_arch(env._h, env.sub_batches, env._bounds_c, env._streams_c, self.sios,
                                                        C.byref(_capi.AuvPolicyArch(*self.arch)), C.c_void_p(env.obs.data_ptr()),
                                                        C.c_void_p(env.reward.data_ptr()), C.c_void_p(env.done.data_ptr()), T, 1, t0, g0),
                   "auv_policy_rollout_stacked_arch")
            for i in range(k):
                f._t[i], f._g[i] = min(f._t[i] + T + 1, T + 1), f._g[i] + T + 1
        else:
            f.rollout(T)

    def measure(self):
        f, env = self.fused, self.env
        if self.mode == "eval":
            # one launch over all N rows on the current stream
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(200):
                self.eval_once()
            b.record()
            torch.cuda.synchronize()
            return dict(variant=self.name, envs=N, chains=1, steps=0, env_steps_per_s=0.0, step_us=0.0, policy_us=1e3 * a.elapsed_time(b) / 200,
                        lib=LIB_HASH)
        # the policy launch alone, by events on every chain's stream
        f.begin_rollout()
        torch.cuda.synchronize()
        reps = 200
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(env.sub_batches)]
        for i in range(env.sub_batches):
            ev[i][0].record(env._sub_streams[i])
        for _ in range(reps):
            if reps and f._t[0] >= T:                      # (stay inside the rollout buffers)
                f.begin_rollout()
            for i in range(env.sub_batches):
                self.act(i)
        for i in range(env.sub_batches):
            ev[i][1].record(env._sub_streams[i])
        torch.cuda.synchronize()
        policy_us = 1e3 * max(a.elapsed_time(b) for a, b in ev) / reps
        if f.stack is not None:
            f.reset_frames()
        # policy + environment step
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.rollout()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dict(variant=self.name, envs=N, chains=env.sub_batches, steps=T, env_steps_per_s=N * T / dt, step_us=1e6 * dt / T, policy_us=policy_us,
                    lib=LIB_HASH)


def main():
    specs = [("parent", 1, "plain"), ("stacked_k1", 1, "stacked"), ("stacked_k2", 2, "stacked"), ("stacked_k4", 4, "stacked"),
             ("stacked_k4_no_O", 4, "stacked", False), ("eval_k4", 4, "eval"), ("torch_k2", 2, "torch"), ("torch_k4", 4, "torch")]
    if ONLY is not None:
        specs = [s for s in specs if s[0] in ONLY]
    if len(ARCHS) == 1:
        variants = [Variant(*s, arch=ARCHS[0]) for s in specs]
    else:
        variants = [Variant(s[0] + "@" + "-".join(str(x) for x in h), *s[1:], arch=h) for s in specs for h in ARCHS]
    for v in variants:                                     # warm-up: every kernel loaded, every allocation made
        v.rollout()
        torch.cuda.synchronize()
    res = {v.name: [] for v in variants}
    for p in range(PASSES):
        for v in variants:
            r = v.measure()
            r["pass"] = p
            res[v.name].append(r)
            print(json.dumps(r), flush=True)
    summary = {}
    for name, rows in res.items():
        s = [r["env_steps_per_s"] for r in rows]
        u = [r["policy_us"] for r in rows]
        summary[name] = dict(env_steps_per_s=dict(median=statistics.median(s), min=min(s), max=max(s)),
                             policy_us=dict(median=statistics.median(u), min=min(u), max=max(u)))
    print(json.dumps(dict(summary=summary, envs=N, chains_asked=CHAINS, chains=variants[0].env.sub_batches, steps=T, passes=PASSES,
                          lib=LIB_HASH)), flush=True)
    for v in variants:
        v.env.close()


if __name__ == "__main__":
    main()
