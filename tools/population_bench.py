#!/usr/bin/env python3
"""Rate of PolicyPopulation.rollout against the shared-policy rollout of a PARENT build, in alternating passes of one session:

    tools/population_bench.py --parent-root DIR [--passes 3] [--envs 4096] [--steps 256] [--net-arch H1,H2,H3]

DIR is a built checkout of the commit to compare against; a pass runs its `tools/policy_bench.py ENVS --quick` (one policy for the
whole batch, one chain), then this tree's population rollout with 256 members x 16 rows and with 64 members x 64 rows -- each in a
fresh child process, one after the other.  Without --parent-root only the population passes run.  Also: the duration of one
k11_population_act launch against one k9_policy_eval launch (policy net only) on the same rows.  Prints one line per measurement and
a summary (medians over the passes), and the sha256 of this tree's library."""
import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(envs, rows, steps, hidden=(256, 128, 64)):
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import ppo
    from gym_auv_amd.batched_env import BatchedAuvEnv
    from gym_auv_amd.config import effective_reference_config
    from gym_auv_amd.devgen import GeneratedWorlds
    from gym_auv_amd.policy import pack_policy_params, policy_eval
    from gym_auv_amd.population import PolicyPopulation, population_act
    cfg = effective_reference_config(use_lidar=True)
    env = BatchedAuvEnv(cfg, GeneratedWorlds(2 * envs, 17, 11, seed=1), envs, device="cuda:0")      # (tools/policy_bench.py's batch)
    env.reset()
    net = ppo.ActorCritic(env.obs_dim, hidden=hidden).to("cuda:0")
    pop = PolicyPopulation(env, envs // rows, rows, net=net, seed=1)      # (reads the widths off the net)
    pop.perturb(0.02, 0)
    pop.rollout(16)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pop.rollout(steps)
    t_host = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_roll = (time.perf_counter() - t0) / steps
    # one launch of each kernel on the same rows, back to back on one stream
    params = pack_policy_params(net, env.obs_dim, hidden=hidden)
    out = {"action": pop.actions}

    def timed(fn, reps=200):
        for _ in range(10):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return 1e3 * a.elapsed_time(b) / reps
    us_pop = timed(lambda: population_act(pop.members, env.obs_dim, rows, env.obs, want=("action",), action_map=pop.action_map, out=out,
                                          hidden=hidden))
    us_k9 = timed(lambda: policy_eval(params, env.obs_dim, env.obs, want=("action",), action_map=pop.action_map, out=out, hidden=hidden))
    env.close()
    print(json.dumps(dict(kind="population", hidden=list(hidden), envs=envs, members=envs // rows, rows=rows, us_per_step=1e6 * t_roll,
                          m_env_steps_s=envs / t_roll / 1e6,
                          host_us_per_step=1e6 * t_host / steps, k11_population_act_us=us_pop, k9_policy_eval_us=us_k9)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--child", type=int, default=0, help="(internal) rows per member: run one population measurement")
    ap.add_argument("--net-arch", default="256,128,64", metavar="H1,H2,H3",
                    help="hidden widths of the members' net, one of gym_auv_amd.policy.SUPPORTED_HIDDEN (the parent's shared-policy pass "
                         "stays at its own default)")
    a = ap.parse_args()
    hidden = tuple(int(h) for h in a.net_arch.split(","))
    if a.child:
        return child(a.envs, a.child, a.steps, hidden)
    if a.parent_root:
        a.parent_root = os.path.abspath(a.parent_root)
    lib = os.path.join(ROOT, "gym_auv_amd", "csrc", "libauv_hip.so")
    print("library sha256 %s" % hashlib.sha256(open(lib, "rb").read()).hexdigest(), flush=True)
    shared, pops = [], {16: [], 64: []}
    env = {k: v for k, v in os.environ.items() if k != "AUV_HIP_LIB"}
    for p in range(a.passes):
        if a.parent_root:
            out = subprocess.run([sys.executable, os.path.join(a.parent_root, "tools", "policy_bench.py"), str(a.envs), "--quick"], cwd=a.parent_root,
                                 env=env, check=True, capture_output=True, text=True, timeout=600).stdout
            m = re.search(r"policy \+ env step ([0-9.]+) us per step = ([0-9.]+) M env-steps/s", out)
            shared.append(float(m.group(2)))
            print("pass %d parent shared policy: %s us per step, %s M env-steps/s" % (p, m.group(1), m.group(2)), flush=True)
        for rows in (16, 64):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(rows), "--envs", str(a.envs), "--steps", str(a.steps),
                                  "--net-arch", a.net_arch], cwd=ROOT, env=env, check=True, capture_output=True, text=True, timeout=600).stdout
            r = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
            pops[rows].append(r)
            print("pass %d population %d x %d: %.1f us per step, %.2f M env-steps/s (host %.1f us); k11_population_act %.1f us, k9_policy_eval %.1f us"
                  % (p, r["members"], rows, r["us_per_step"], r["m_env_steps_s"], r["host_us_per_step"], r["k11_population_act_us"],
                     r["k9_policy_eval_us"]), flush=True)
    med = lambda xs: statistics.median(xs) if xs else None      # noqa: E731
    res = dict(hidden=list(hidden), parent_shared_m_env_steps_s=med(shared))
    for rows in (16, 64):
        res["population_G%d_m_env_steps_s" % rows] = med([r["m_env_steps_s"] for r in pops[rows]])
        res["k11_population_act_G%d_us" % rows] = med([r["k11_population_act_us"] for r in pops[rows]])
        res["k9_policy_eval_us_G%d_rows" % rows] = med([r["k9_policy_eval_us"] for r in pops[rows]])
    res["G16_over_G64"] = res["population_G16_m_env_steps_s"] / res["population_G64_m_env_steps_s"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
