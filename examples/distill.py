#!/usr/bin/env python3
"""Expert iteration on the Colav task: the shooting planner decides, the policy is trained towards its decisions, the planner plans
around the policy it is training (prior = the actor's action, terminal value = the critic).

Every decision: plan -> (observation, the planner's first action mapped into the policy's space, the plan's predicted score mapped into
the critic's units) into a DistillBuffer -> the real batch steps with the planner's action, or, per environment with probability
1 - beta, with the policy's own (DAgger's mixing).  Every `every` decisions: `epochs` passes of clone_step minibatches over the
buffer; the updater is attach()ed, so the planner's prior and value follow every step without a repack.  At the end the policy ALONE is
evaluated through examples/evaluate.py's loop and printed against the planner and against the untrained policy.

    python examples/distill.py --envs 64 --decisions 400 --every 20 --epochs 2
    python examples/distill.py --eager 1        # the same loop with the stock torch step (clone_loss_terms + Adam + refresh)

No learning result is promised: this is the loop, at the project's speed."""
import argparse
import json
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gym_auv_amd import scenarios  # noqa: E402
from gym_auv_amd.batched_env import BatchedAuvEnv  # noqa: E402
from gym_auv_amd.config import effective_reference_config  # noqa: E402
from gym_auv_amd.planning import DistillBuffer, ShootingPlanner  # noqa: E402
from gym_auv_amd.policy import FusedActorCritic  # noqa: E402
from gym_auv_amd.ppo_update import FusedPPOUpdate, clone_loss_terms  # noqa: E402
from gym_auv_amd.world import build_world, pack_bank  # noqa: E402


def metrics(log):
    """Goal rate, collision rate and mean progress of episode-log rows (BatchedAuvEnv.EPISODE_LOG_COLUMNS)."""
    k = int(log.shape[0])
    if not k:
        return dict(episodes=0)
    col = {c: log[:, i] for i, c in enumerate(BatchedAuvEnv.EPISODE_LOG_COLUMNS)}
    return dict(episodes=k, goal_rate=float((col["reached_goal"] != 0).double().mean()),
                collision_rate=float((col["collision"] != 0).double().mean()), progress_mean=float(col["progress"].mean()))


def run(envs=64, candidates=32, horizon=16, decisions=400, every=20, epochs=2, batch=256, beta=0.5, kind="nll", lr=3e-4, eager=False,
        capacity=65536, reward_scale=0.01, eval_episodes=1, eval_steps=2000, seed=0, device="cuda:0", log=print,
        net_arch=(256, 128, 64)):
    from evaluate import evaluate, load_policy
    cfg = effective_reference_config(use_lidar=True)
    bank = pack_bank([build_world(scenarios.moving_obstacles_world(seed + i)) for i in range(2 * envs)])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = BatchedAuvEnv(cfg, bank, envs, device=device, rewarder="colav", auto_reset=True)
    env.reset()
    net = load_policy(None, env.obs_dim, device, seed, hidden=tuple(int(h) for h in net_arch)).train()
    lo, hi = env.action_space.low, env.action_space.high              # the policy speaks [-1, 1]^2
    fused = FusedActorCritic(net, env, rollout=1, act_mid=((lo + hi) / 2).tolist(), act_half=((hi - lo) / 2).tolist(),
                             clip_lo=[-1.0, -1.0], clip_hi=[1.0, 1.0], seed=seed)
    res = dict(envs=envs, candidates=candidates, horizon=horizon, decisions=decisions, every=every, epochs=epochs, batch=batch, beta=beta,
               kind=kind, step="eager" if eager else "fused")
    res["untrained"] = metrics(evaluate(env, fused, eval_episodes, eval_steps)[0])
    if eager:
        upd, opt = None, torch.optim.Adam(net.parameters(), lr=lr)
    else:
        upd = FusedPPOUpdate(net, lr=lr, vf_coef=0.5, ent_coef=0.01, max_batch=batch)
        upd.attach(fused)
    # the critic lives in scaled-reward units (examples/ppo.py): terminal = value / reward_scale
    planner = ShootingPlanner(env, candidates=candidates, horizon=horizon, seed=seed, prior=fused, value=fused, value_scale=1.0 / reward_scale)
    buf = DistillBuffer(capacity, env.obs_dim, env.device)
    gen = torch.Generator(device=env.device).manual_seed(seed + 1)
    env.reset()
    env.episode_log()
    n_updates = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for d in range(decisions):
        actions, _, predicted = planner.plan()
        buf.add(env.obs, *DistillBuffer.targets_from_plan(planner, actions, predicted))
        if beta < 1.0:
            own = fused.predict()                                     # the policy's deterministic action, into fused.actions
            take = torch.rand((envs, 1), generator=gen, device=env.device) < beta
            actions = torch.where(take, actions, own)
        env.step(actions.contiguous())
        if (d + 1) % every == 0:
            for _ in range(epochs * max(1, buf.size // batch)):
                idx = buf.sample(batch, gen)
                if eager:
                    opt.zero_grad()
                    clone_loss_terms(net, buf.O[idx], buf.A[idx], buf.RET[idx], buf.W[idx], kind, 0.5, 0.01)[0].backward()
                    opt.step()
                    fused.refresh()
                else:
                    upd.clone_step(buf.O, buf.A, buf.RET, buf.W, idx, kind=kind)
                n_updates += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res.update(loop_seconds=dt, decisions_per_s=decisions * envs / dt, clone_steps=n_updates, mixed=metrics(env.episode_log()))
    if upd is not None and n_updates:
        last = upd.log[(upd.n_steps - 1) % upd.LOG_ROWS].tolist()
        res.update(last_loss=last[0], last_bc=last[1], last_vf=last[2], nonfinite_inputs=float(upd.log[:min(upd.n_steps, upd.LOG_ROWS), 5].sum()))
    # the planner alone (around the trained policy), then the policy alone
    env.reset()
    env.episode_log()
    for _ in range(min(eval_steps, 400)):
        env.step(planner.plan()[0])
    res["planner"] = metrics(env.episode_log())
    env.reset()
    res["policy"] = metrics(evaluate(env, fused, eval_episodes, eval_steps)[0])
    for name in ("untrained", "planner", "policy"):
        log("%-9s %s" % (name, json.dumps(res[name])))
    planner.close()
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--candidates", type=int, default=32)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--decisions", type=int, default=400)
    ap.add_argument("--every", type=int, default=20, help="decisions between two rounds of clone steps")
    ap.add_argument("--epochs", type=int, default=2, help="passes over the buffer per round")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--beta", type=float, default=0.5, help="probability that an environment steps with the planner's action (else the policy's own)")
    ap.add_argument("--kind", default="nll", choices=["nll", "mse"])
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--eager", type=int, default=0, help="1: the stock torch step instead of the fused one")
    ap.add_argument("--eval-episodes", type=int, default=1)
    ap.add_argument("--eval-steps", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--net-arch", default="256,128,64", metavar="H1,H2,H3",
                    help="hidden widths of the policy and the value net: one of 256,128,64 (the reference's)  128,128,64  128,64,64  64,64,64")
    a = ap.parse_args()
    res = run(envs=a.envs, candidates=a.candidates, horizon=a.horizon, decisions=a.decisions, every=a.every, epochs=a.epochs, batch=a.batch,
              beta=a.beta, kind=a.kind, lr=a.lr, eager=bool(a.eager), eval_episodes=a.eval_episodes, eval_steps=a.eval_steps, seed=a.seed,
              device=a.device, net_arch=tuple(int(h) for h in a.net_arch.split(",")))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
