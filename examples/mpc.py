#!/usr/bin/env python3
"""Model-predictive control by shooting on the batched simulator: the standard non-learning baseline of collision-avoidance work.

Every real vessel branches K candidate action sequences from its current state (BatchedAuvEnv.snapshot / restore into the planner's
own batch), rolls them T steps forward in one launch, and executes the first action of the best one -- closed loop, until its
episode ends.  Prints the return of every vessel and the plans per second.

    python examples/mpc.py --scenario TestScenario1 --vessels 4 --candidates 64 --horizon 16
    python examples/mpc.py --scenario moving --vessels 16 --iterations 3          # CEM
    python examples/mpc.py --scenario moving --vessels 16 --iterations 3 --sampler device --method mppi --mppi-lambda 5 --warm-start
    python examples/mpc.py --value policy.pt --value-scale 100 --prior policy.pt  # a learned critic beyond the horizon, the actor as the mean
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gym_auv_amd import scenarios  # noqa: E402
from gym_auv_amd.batched_env import BatchedAuvEnv  # noqa: E402
from gym_auv_amd.config import effective_reference_config  # noqa: E402
from gym_auv_amd.planning import ShootingPlanner  # noqa: E402
from gym_auv_amd.world import build_world, pack_bank  # noqa: E402

SCENARIOS = {"TestScenario1": scenarios.test_scenario1, "TestScenario2": scenarios.test_scenario2, "TestScenario3": scenarios.test_scenario3,
             "TestScenario4": scenarios.test_scenario4, "TestHeadOn": scenarios.test_head_on, "TestCrossing": scenarios.test_crossing}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenario", default="TestScenario1", help="%s, or 'moving' (a different MovingObstacles world per vessel)" % ", ".join(SCENARIOS))
    ap.add_argument("--vessels", type=int, default=4)
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=1)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--max-steps", type=int, default=400)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--value", default=None, metavar="CKPT",
                    help="state_dict of examples/ppo.py's ActorCritic: its critic is the terminal value beyond the horizon (one fused launch per plan)")
    ap.add_argument("--value-scale", type=float, default=100.0, help="terminal = value * scale + shift (the critic lives in scaled-reward "
                                                                      "units: 1 / reward_scale of the training run)")
    ap.add_argument("--value-shift", type=float, default=0.0)
    ap.add_argument("--prior", default=None, metavar="CKPT", help="state_dict of an ActorCritic: its deterministic action, held over the horizon, is "
                                                                  "the mean the candidates are drawn around")
    ap.add_argument("--sampler", choices=("torch", "device"), default="torch", help="device: sample and refit in two HIP launches per iteration, "
                                                                                     "counter-based noise (reproducible on the host)")
    ap.add_argument("--method", choices=("cem", "mppi"), default="cem", help="mppi (path-integral weights over all candidates) needs --sampler device")
    ap.add_argument("--mppi-lambda", type=float, default=1.0, help="temperature of the MPPI weights, in reward units")
    ap.add_argument("--warm-start", action="store_true", help="receding horizon: start every plan from the previous one moved on one step "
                                                             "(needs --sampler device)")
    args = ap.parse_args()
    cfg = effective_reference_config(use_lidar=True)
    B = args.vessels
    if args.scenario == "moving":
        worlds = [scenarios.moving_obstacles_world(args.seed + i) for i in range(B)]
    else:
        worlds = [SCENARIOS[args.scenario]()]
    bank = pack_bank([build_world(w) for w in worlds])
    env = BatchedAuvEnv(cfg, bank, B, auto_reset=False, test_mode=True)
    env.reset()
    nets = {}

    def fused_of(ckpt):
        if ckpt and ckpt not in nets:
            from evaluate import load_policy
            from gym_auv_amd.policy import FusedActorCritic
            nets[ckpt] = FusedActorCritic(load_policy(ckpt, env.obs_dim, env.device), env, rollout=1)
        return nets.get(ckpt)
    planner = ShootingPlanner(env, candidates=args.candidates, horizon=args.horizon, gamma=args.gamma, iterations=args.iterations, seed=args.seed,
                              value=fused_of(args.value), value_scale=args.value_scale, value_shift=args.value_shift, prior=fused_of(args.prior),
                              sampler=args.sampler, method=args.method, mppi_lambda=args.mppi_lambda, warm_start=args.warm_start)
    ret = torch.zeros(B, dtype=torch.float64, device=env.device)
    running = torch.ones(B, dtype=torch.bool, device=env.device)
    torch.cuda.synchronize()
    t0, steps = time.perf_counter(), 0
    done = None
    while steps < args.max_steps:
        # (warm start: a vessel whose episode has just ended plans afresh, the others carry their plan on by one step)
        actions, _, _ = planner.plan(reset=done.contiguous() if args.warm_start and done is not None else None)
        _, reward, done, _ = env.step(actions)
        ret += torch.where(running, reward.double(), torch.zeros_like(ret))
        running &= ~done.bool()
        steps += 1
        if steps % 20 == 0 and not bool(running.any()):     # (one small read-back every 20 decisions)
            break
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    info = env.read("INFO64").cpu()
    for b in range(B):
        print("vessel %d: return %.1f  progress %.2f  collision %d  reached_goal %d" % (b, float(ret[b]), float(info[b, 3]), int(info[b, 0]),
                                                                                       int(info[b, 1])))
    print("%d decisions for %d vessels in %.2f s: %.0f plans/s (%d candidates x %d steps each, %d iteration(s))"
          % (steps, B, dt, steps / dt, args.candidates, args.horizon, args.iterations))


if __name__ == "__main__":
    main()
