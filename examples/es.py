#!/usr/bin/env python3
"""OpenAI-ES with mirrored sampling on the reference's own actor, a population per launch (gym_auv_amd/population.py).

The task is the one examples/ppo.py --task pathfollow learns: PathFollowNoObstacles-v0 (no obstacles, LiDAR off, PathFollowRewarder;
gym_auv/__init__.py:105-121), the policy obs[6] -> [256, 128, 64] tanh -> 2 (scripts/run.py:332-357).  256 members x 16 environments
step side by side; a generation is

    perturb   theta_p = theta +- sigma eps_p            one launch, counter-based noise (nothing of it is stored)
    rollout   T x (population launch + env step)        one C call; per-member fitness = mean over its environments of the summed reward
    update    theta += lr / (P sigma) sum_p w_p eps_p   one launch, eps regenerated; w = centred ranks of the fitness

and nothing returns to the host in between except the fitness that is printed.

    python examples/es.py --generations 30 --rollout 64
    python examples/es.py --net-arch 64,64,64                  # a narrower actor: fewer parameters for the estimate, a shorter launch
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))


def train(members=256, rows=16, generations=30, rollout=64, sigma=0.02, lr=0.01, seed=0, device="cuda:0", task="pathfollow", log=print,
          net_arch=(256, 128, 64)):
    import ppo
    from gym_auv_amd.batched_env import BatchedAuvEnv
    from gym_auv_amd.config import effective_reference_config
    from gym_auv_amd.devgen import GeneratedWorlds
    from gym_auv_amd.population import PolicyPopulation
    colav = task == "colav"
    cfg = effective_reference_config(use_lidar=colav)
    n = members * rows
    nm, ns = (17, 11) if colav else (0, 0)
    env = BatchedAuvEnv(cfg, GeneratedWorlds(2 * n, nm, ns, seed=1000 * seed), n, device=device, auto_reset=True,
                        rewarder="colav" if colav else "pathfollow")
    env.reset()
    torch.manual_seed(seed)
    # --net-arch: the hidden widths of the actor, one of the triples the population kernels are compiled for
    # (gym_auv_amd._capi.POLICY_ARCHS, the list of examples/ppo.py --net-arch); PolicyPopulation reads them off the net
    net = ppo.ActorCritic(env.obs_dim, hidden=tuple(int(h) for h in net_arch)).to(device)
    # the policy's box is [-1, 1]^2 mapped onto the action space (examples/ppo.py --act-space normalized)
    low, high = torch.as_tensor(env.action_space.low), torch.as_tensor(env.action_space.high)
    pop = PolicyPopulation(env, members, rows, net=net, act_mid=(0.5 * (high + low)).tolist(), act_half=(0.5 * (high - low)).tolist(),
                           clip_lo=(-1.0, -1.0), clip_hi=(1.0, 1.0), seed=seed)
    log("es: %d members x %d environments, obs_dim %d, hidden %s, %d floats per member, T = %d, sigma %g, lr %g"
        % (pop.P, pop.G, env.obs_dim, list(pop.hidden), pop.nf, rollout, sigma, lr))
    history, seconds = [], []
    for g in range(generations):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pop.perturb(sigma, g)
        fitness, ends = pop.rollout(rollout)
        pop.update(pop.centered_ranks(fitness), lr, sigma, g)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        seconds.append(dt)
        f = fitness.cpu()
        history.append(float(f.mean()))
        log("gen %3d  fitness mean %9.3f  best %9.3f  worst %9.3f  episodes ended %5d  |grad| %.3e  %.2f M env-steps/s"
            % (g, float(f.mean()), float(f.max()), float(f.min()), int(ends.sum()), float(pop.grad.norm()), n * rollout / dt / 1e6))
    if len(seconds) > 1:                                       # (the first generation carries the one-time set-up of the launches)
        log("es: %.2f generations/s (perturb + rollout + update, generations 1..%d)" % ((len(seconds) - 1) / sum(seconds[1:]), len(seconds) - 1))
    env.close()
    return history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=256)
    ap.add_argument("--rows", type=int, default=16, help="environments per member (a multiple of 16)")
    ap.add_argument("--generations", type=int, default=30)
    ap.add_argument("--rollout", type=int, default=64, help="steps per generation")
    ap.add_argument("--sigma", type=float, default=0.02)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--task", default="pathfollow", choices=["colav", "pathfollow"])
    ap.add_argument("--net-arch", default="256,128,64", metavar="H1,H2,H3",
                    help="hidden widths of the actor: one of 256,128,64 (the reference's)  128,128,64  128,64,64  64,64,64")
    a = ap.parse_args()
    train(a.members, a.rows, a.generations, a.rollout, a.sigma, a.lr, a.seed, task=a.task, net_arch=tuple(int(h) for h in a.net_arch.split(",")))
