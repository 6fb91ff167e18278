#!/usr/bin/env python3
"""Time one PPO minibatch step three ways in one process, on the same random rows: the eager `minibatch_step` of examples/ppo.py on
rows already gathered, that step behind its five gathers, and the fused step (gym_auv_amd/ppo_update.py).  B = 16384 rows of 131072
stored ones, obs_dim 186 and 15; HIP events around every step, warm-up, the median of `--reps` steps.  With --train it then runs
examples/ppo.py for a few updates with --fused-update off and on and reports `sps`.  One JSON line per measurement goes to --out.
--arch H1,H2,H3[:H1,H2,H3...]: hidden widths of the nets (gym_auv_amd.ppo_update.SUPPORTED_HIDDEN); several, separated by ':', are
measured one after the other in the same session, `--passes` times round (alternating passes show the spread between them).

    python tools/ppo_update_bench.py --out profiles/ppo_update/ppo_update_bench.jsonl --train 1
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return dict(median_ms=statistics.median(ms), min_ms=ms[0], p90_ms=ms[int(0.9 * (len(ms) - 1))], reps=reps)


def bench_width(obs_dim, B, n_rows, warmup, reps, device, arch=(256, 128, 64)):
    import ppo
    from gym_auv_amd.ppo_update import FusedPPOUpdate
    torch.manual_seed(0)
    clip, ent_coef = 0.2, 0.01
    net = ppo.ActorCritic(obs_dim, hidden=arch).to(device)
    twin = ppo.ActorCritic(obs_dim, hidden=arch).to(device)
    twin.load_state_dict(net.state_dict())
    O, A = torch.randn(n_rows, obs_dim, device=device), torch.randn(n_rows, 2, device=device) * 0.5
    with torch.no_grad():
        LP = net.log_prob(net.pi(O), A) + 0.05 * torch.randn(n_rows, device=device)
    ADV, RET = torch.randn(n_rows, device=device), torch.randn(n_rows, device=device)
    params = list(twin.parameters())
    pi_params, v_params = list(twin.pi.parameters()) + [twin.log_std], list(twin.v.parameters())
    opt = torch.optim.Adam(params, lr=2e-4)
    diag_row = torch.zeros((1, 8), device=device)

    def eager(o, a, lp, advn, retn):
        # minibatch_step of examples/ppo.py (single rank, no graph capture), with its diagnostics row
        mu = twin.pi(o)
        ratio = (twin.log_prob(mu, a) - lp).exp()
        pg = -torch.min(ratio * advn, ratio.clamp(1 - clip, 1 + clip) * advn).mean()
        vf = 0.5 * (twin.v(o).squeeze(-1) - retn).pow(2).mean()
        loss = pg + 0.5 * vf - ent_coef * twin.entropy()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        bad_in = torch.zeros((), device=device)
        for x in (o, a, lp, advn, retn):
            bad_in = bad_in + (~torch.isfinite(x)).sum(dtype=torch.float32)
        bad_g = torch.zeros((), device=device)
        for q in params:
            bad_g = bad_g + (~torch.isfinite(q.grad)).sum(dtype=torch.float32)
        n_pi, n_v = ppo.clip_grad_norm(pi_params, 0.5), ppo.clip_grad_norm(v_params, 0.5)
        for j, x in enumerate((n_pi, n_v, loss.detach(), advn.abs().max(), ratio.detach().max(), bad_in, bad_g)):
            diag_row[0, j].copy_(x)
        opt.step()

    idx = torch.randperm(n_rows, device=device)[:B].contiguous()
    rows = (O[idx], A[idx], LP[idx], ADV[idx], RET[idx])
    upd = FusedPPOUpdate(net, lr=2e-4, clip=clip, vf_coef=0.5, ent_coef=ent_coef, max_batch=B)
    out = dict(obs_dim=obs_dim, B=B, n_rows=n_rows, arch=list(arch))
    out["eager"] = timed(lambda: eager(*rows), warmup, reps)
    out["eager_with_gathers"] = timed(lambda: eager(O[idx], A[idx], LP[idx], ADV[idx], RET[idx]), warmup, reps)
    out["fused"] = timed(lambda: upd.step(O, A, LP, ADV, RET, idx), warmup, reps)
    out["fused_grad_only"] = timed(lambda: upd.grad(O, A, LP, ADV, RET, idx), warmup, reps)
    # the same step for a tanh-squashed policy (auv_ppo_grad_squash), on a net of its own, in the same session
    sq_net = ppo.ActorCritic(obs_dim, hidden=arch).to(device)
    sq_net.load_state_dict(twin.state_dict())
    sq = FusedPPOUpdate(sq_net, lr=2e-4, clip=clip, vf_coef=0.5, ent_coef=ent_coef, max_batch=B, squash=True)
    out["fused_squash"] = timed(lambda: sq.step(O, A, LP, ADV, RET, idx), warmup, reps)
    out["fused_again"] = timed(lambda: upd.step(O, A, LP, ADV, RET, idx), warmup, reps)
    out["speedup_vs_eager"] = out["eager"]["median_ms"] / out["fused"]["median_ms"]
    out["speedup_vs_eager_with_gathers"] = out["eager_with_gathers"]["median_ms"] / out["fused"]["median_ms"]
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_update", "ppo_update_bench.jsonl"))
    ap.add_argument("--B", type=int, default=16384)
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--train", type=int, default=0, help="1: also run examples/ppo.py with --fused-update 0 and 1")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rollout", type=int, default=128)
    ap.add_argument("--updates", type=int, default=4)
    ap.add_argument("--arch", default="256,128,64", metavar="H1,H2,H3[:H1,H2,H3...]", help="hidden widths; several separated by ':'")
    ap.add_argument("--obs-dims", default="186,15", help="observation widths, separated by ','")
    ap.add_argument("--passes", type=int, default=1, help="times the list of widths is gone through")
    a = ap.parse_args()
    archs = [tuple(int(x) for x in s.split(",")) for s in a.arch.split(":")]
    from gym_auv_amd import _capi
    sha = hashlib.sha256(open(_capi.LIB_PATH, "rb").read()).hexdigest()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        def emit(rec):
            rec["lib_sha256"] = sha
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        for k in range(a.passes):
            for arch in archs:
                for D in (int(x) for x in a.obs_dims.split(",")):
                    emit(dict(kind="minibatch_step", device=torch.cuda.get_device_name(0), **{"pass": k},
                              **bench_width(D, a.B, a.rows, a.warmup, a.reps, "cuda:0", arch)))
        if a.train:
            import ppo
            for arch, flag in ((h, f) for h in archs for f in (0, 1)):
                hist = ppo.train(envs=a.envs, updates=a.updates, rollout=a.rollout, log=lambda *_: None, fused_update=bool(flag), net_arch=arch)
                tail = hist[1:] or hist                          # (the first update pays for allocations and start-up)
                emit(dict(kind="train", fused_update=flag, arch=list(arch), envs=a.envs, rollout=a.rollout, updates=a.updates,
                          sps=[h["sps"] for h in hist], sps_median_after_first=statistics.median(h["sps"] for h in tail),
                          rollout_sps_median=statistics.median(h["rollout_sps"] for h in tail),
                          nonfinite_steps=sum(h["minibatch_steps_nonfinite"] for h in hist)))
