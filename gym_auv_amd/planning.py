"""Planning by shooting on the batched simulator: model-predictive control with random shooting or the cross-entropy method.

For each of the B real environments the planner branches K candidate action sequences from the environment's CURRENT state,
rolls all B * K of them T steps forward in one open-loop launch (`step_multi` with a reward record), scores them on the device
(`auv_plan_score`) and returns the first action of the best one -- the standard non-learning baseline a collision-avoidance
agent is compared against.  What makes it possible is snapshot / restore (BatchedAuvEnv.snapshot, .restore): the real batch's
state is copied K-fold into a second batch the planner owns; the real environments are never stepped by a plan.

A plan enqueues work on the caller's current stream and returns device tensors: no host synchronisation.
"""
import ctypes as C
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch


# ---- index maps: planner environment e = b * K + k is candidate k of real environment (group) b -------------------------------
def candidate_env(b, k, K: int):
    """Planner environment of candidate k of real environment b."""
    return b * K + k


def env_group(e, K: int):
    """(real environment, candidate) of planner environment e."""
    return e // K, e % K


def fork_rows(B: int, K: int) -> torch.Tensor:
    """[B * K] int32: the snapshot row (= real environment) every planner environment is restored from: 0 x K, 1 x K, ..."""
    return torch.arange(B, dtype=torch.int32).repeat_interleave(K)


def reference_plan_score(reward, done, group: int, gamma: float) -> Tuple[np.ndarray, np.ndarray]:
    """auv_plan_score's contract as a plain float32 loop (tests check the kernel against it, bit for bit):
    score[e] = sum_t disc_t * reward[t][e] up to and including the first t with done[t][e], disc_0 = 1, disc_{t+1} = disc_t * gamma,
    every product and sum rounded to float32 in increasing t; best[g] = index within group g of its largest score, the lowest
    index wins a tie, a NaN never wins (all NaN: 0).  reward [T, n] float32, done [T, n]; returns (score [n] f32, best [n / group] i32)."""
    reward = np.asarray(reward, dtype=np.float32)
    done = np.asarray(done) != 0
    T, n = reward.shape
    if n % group:
        raise ValueError("n = %d is not a multiple of group = %d" % (n, group))
    score = np.zeros(n, dtype=np.float32)
    g32 = np.float32(gamma)
    with np.errstate(all="ignore"):
        for e in range(n):
            s, disc = np.float32(0.0), np.float32(1.0)
            for t in range(T):
                s = np.float32(s + np.float32(disc * reward[t, e]))
                if done[t, e]:
                    break
                disc = np.float32(disc * g32)
            score[e] = s
    best = np.zeros(n // group, dtype=np.int32)
    for g in range(n // group):
        have, bs = False, np.float32(0.0)
        for k in range(group):
            s = score[g * group + k]
            if s != s:
                continue
            if not have or s > bs:
                have, bs, best[g] = True, s, k
    return score, best


def reference_plan_score_terminal(reward, done, group: int, gamma: float, terminal) -> Tuple[np.ndarray, np.ndarray]:
    """auv_plan_score_v's contract as a plain float32 loop: reference_plan_score, and in addition an environment with NO done in
    [0, T) adds float32(disc_T * terminal[e]), disc_T the same running product after T multiplications -- one more rounded product
    and one more rounded sum, last in order.  An environment that saw a done never reads its terminal value.  terminal [n] float32."""
    reward = np.asarray(reward, dtype=np.float32)
    done = np.asarray(done) != 0
    terminal = np.asarray(terminal, dtype=np.float32).reshape(-1)
    T, n = reward.shape
    if n % group:
        raise ValueError("n = %d is not a multiple of group = %d" % (n, group))
    if terminal.shape[0] != n:
        raise ValueError("terminal has %d entries, n = %d" % (terminal.shape[0], n))
    score = np.zeros(n, dtype=np.float32)
    g32 = np.float32(gamma)
    with np.errstate(all="ignore"):
        for e in range(n):
            s, disc, ended = np.float32(0.0), np.float32(1.0), False
            for t in range(T):
                s = np.float32(s + np.float32(disc * reward[t, e]))
                if done[t, e]:
                    ended = True
                    break
                disc = np.float32(disc * g32)
            if not ended:
                s = np.float32(s + np.float32(disc * terminal[e]))
            score[e] = s
    best = np.zeros(n // group, dtype=np.int32)
    for g in range(n // group):
        have, bs = False, np.float32(0.0)
        for k in range(group):
            s = score[g * group + k]
            if s != s:
                continue
            if not have or s > bs:
                have, bs, best[g] = True, s, k
    return score, best


def plan_score(env, reward: torch.Tensor, done: torch.Tensor, group: int, gamma: float,
               terminal: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """auv_plan_score on the caller's current stream: (score [n] float32, best [n / group] int32) of a [T, n] reward / done record.
    `terminal` [n] float32: auv_plan_score_v -- a candidate without a done adds disc_T * terminal[e] (reference_plan_score_terminal)."""
    from . import batched_env as be
    if reward.dim() != 2 or reward.dtype != torch.float32 or done.dtype != torch.uint8 or tuple(done.shape) != tuple(reward.shape) \
            or not reward.is_contiguous() or not done.is_contiguous() or reward.device != env.device or done.device != env.device:
        raise ValueError("reward must be a contiguous [T, n] float32 tensor and done a uint8 tensor of the same shape, on %s" % env.device)
    T, n = int(reward.shape[0]), int(reward.shape[1])
    if group < 1 or n % group:
        raise ValueError("n = %d is not a multiple of group = %d" % (n, group))
    if terminal is not None and (terminal.dtype != torch.float32 or tuple(terminal.shape) != (n,) or not terminal.is_contiguous()
                                 or terminal.device != env.device):
        raise ValueError("terminal must be a contiguous [%d] float32 tensor on %s" % (n, env.device))
    with torch.cuda.device(env.device):
        score = torch.empty((n,), dtype=torch.float32, device=env.device)
        best = torch.empty((n // group,), dtype=torch.int32, device=env.device)
    if terminal is not None:
        be._check(be._LIB.auv_plan_score_v(env._h, C.c_void_p(reward.data_ptr()), C.c_void_p(done.data_ptr()), T, n, int(group), C.c_float(gamma),
                                           C.c_void_p(terminal.data_ptr()), C.c_void_p(score.data_ptr()), C.c_void_p(best.data_ptr()),
                                           env._stream()), "auv_plan_score_v")
        return score, best
    be._check(be._LIB.auv_plan_score(env._h, C.c_void_p(reward.data_ptr()), C.c_void_p(done.data_ptr()), T, n, int(group), C.c_float(gamma),
                                     C.c_void_p(score.data_ptr()), C.c_void_p(best.data_ptr()), env._stream()), "auv_plan_score")
    return score, best


# ---- the sampler and the refit on the device (csrc/k15_plan.hip): their contracts in NumPy, and the calls -------------------------
PLAN_METHODS = {"cem": 0, "mppi": 1}            # (AUV_PLAN_CEM, AUV_PLAN_MPPI)
PLAN_MAX_CANDIDATES = 1024                      # (AUV_PLAN_MAX_GROUP)


def _rank_order(score: np.ndarray) -> np.ndarray:
    """Candidate indices of one group in the total order of the scorer's argmax: larger score first, lower index on a tie; a NaN ranks
    below every number, NaNs among themselves by index."""
    nan = score != score
    return np.array(sorted(range(score.shape[0]), key=lambda k: (bool(nan[k]), 0.0 if nan[k] else -float(score[k]), k)), dtype=np.int64)


def reference_plan_sample(mean, sigma, K: int, lo, hi, seed: int, draw: int, shift: int = 0, reset=None, mean0=None, sigma0=None) -> np.ndarray:
    """auv_plan_sample's contract (the kernel is held to it bit for bit): the ring [T, B * K, 2] float32 with
    ring[t, b * K + k, j] = clip(m + s * eps) -- a rounded product, a rounded sum, fmax(fmin(., hi[j]), lo[j]) -- where m, s are row
    min(t + shift, T - 1) of mean, sigma [T, B, 2] for group b, eps = population.es_noise(seed, draw, pair = b * K + k, idx = 2 t + j),
    and candidate 0 is clip(m).  A group with reset[b] != 0 reads row t (no shift) of mean0 / sigma0 instead."""
    from .population import es_noise
    mean, sigma = np.asarray(mean, dtype=np.float32), np.asarray(sigma, dtype=np.float32)
    T, B = mean.shape[0], mean.shape[1]
    if mean.shape != (T, B, 2) or sigma.shape != (T, B, 2) or int(shift) not in (0, 1) or int(K) < 1:
        raise ValueError("reference_plan_sample: mean and sigma are [T, B, 2], shift is 0 or 1, K >= 1")
    rows = np.minimum(np.arange(T) + int(shift), T - 1)
    m, s = mean[rows].copy(), sigma[rows].copy()
    if reset is not None:
        fresh = np.asarray(reset).reshape(B) != 0
        m[:, fresh] = np.asarray(mean0, dtype=np.float32)[:, fresh]
        s[:, fresh] = np.asarray(sigma0, dtype=np.float32)[:, fresh]
    n = B * int(K)
    b = np.arange(n) // int(K)
    m, s = m[:, b, :], s[:, b, :]                                          # [T, n, 2]
    idx = 2 * np.arange(T)[:, None, None] + np.arange(2)[None, None, :]
    eps = es_noise(seed, draw, np.arange(n)[None, :, None], idx)
    with np.errstate(all="ignore"):
        v = (m + (s * eps).astype(np.float32)).astype(np.float32)
        v[:, ::int(K), :] = m[:, ::int(K), :]
        return np.fmax(np.fmin(v, np.asarray(hi, dtype=np.float32)), np.asarray(lo, dtype=np.float32)).astype(np.float32)


def reference_plan_refit(ring, score, best, K: int, method: str = "cem", n_elite: int = 1, sigma_min: float = 0.0, lam: float = 1.0,
                         mean_in=None, sigma_in=None, mppi_dtype=np.float64):
    """auv_plan_refit's contract: (mean [T, B, 2], sigma [T, B, 2], chosen [T, B, 2], predicted [B]) from the ring [T, B * K, 2], the
    scores [B * K] and the winners best [B].  chosen / predicted are plain gathers (float32).
    "cem": float32, bit for bit the kernel -- the elite are the first n_elite candidates of a group in the scorer's order (a NaN
        last, ties by index); over them in ascending index, s = the sequential sum of a, mean = s / n_elite, q = the sequential sum
        of (a - mean) * (a - mean), sigma = fmax(sqrt(q / n_elite), sigma_min), every operation rounded to float32.
    "mppi": FLOAT64 (the kernel's expf is not reproducible on a host; tests hold it to a recorded bound) -- w_k = 1 at the group's
        largest valid score, else exp((score_k - max) / lam) with the float32-rounded difference and quotient the kernel forms,
        0 for a NaN; mean = sum w a / sum w over all k; sigma = sigma_in; a group without a valid score keeps mean_in.
        mppi_dtype=np.float32: the same statement with every operation rounded to float32 in the kernel's order and correctly
        rounded weights -- what the recorded bound is derived from (its distance to the float64 result)."""
    ring = np.asarray(ring, dtype=np.float32)
    score = np.asarray(score, dtype=np.float32).reshape(-1)
    T, n, K = ring.shape[0], ring.shape[1], int(K)
    if ring.shape != (T, n, 2) or score.shape[0] != n or K < 1 or n % K or method not in PLAN_METHODS:
        raise ValueError("reference_plan_refit: ring [T, n, 2], score [n], n a multiple of K, method one of %s" % sorted(PLAN_METHODS))
    B = n // K
    bl = np.clip(np.asarray(best, dtype=np.int64).reshape(B), 0, K - 1)
    cand = ring.reshape(T, B, K, 2)
    chosen = cand[:, np.arange(B), bl, :].copy()
    predicted = score.reshape(B, K)[np.arange(B), bl].copy()
    f = np.float32
    with np.errstate(all="ignore"):
        if method == "cem":
            E = int(n_elite)
            if not 1 <= E <= K:
                raise ValueError("reference_plan_refit: n_elite = %d must be in [1, K = %d]" % (E, K))
            mean, sigma = np.zeros((T, B, 2), dtype=f), np.zeros((T, B, 2), dtype=f)
            for b in range(B):
                elite = np.sort(_rank_order(score[b * K:(b + 1) * K])[:E])
                s = np.zeros((T, 2), dtype=f)
                for k in elite:
                    s = (s + cand[:, b, k, :]).astype(f)
                mu = (s / f(E)).astype(f)
                q = np.zeros((T, 2), dtype=f)
                for k in elite:
                    d = (cand[:, b, k, :] - mu).astype(f)
                    q = (q + (d * d).astype(f)).astype(f)
                mean[:, b, :] = mu
                sigma[:, b, :] = np.fmax(np.sqrt((q / f(E)).astype(f)).astype(f), f(sigma_min))
            return mean, sigma, chosen, predicted
        dt = np.dtype(mppi_dtype).type
        mean = np.asarray(mean_in, dtype=np.float32).astype(dt)
        sigma = np.asarray(sigma_in, dtype=np.float32).copy()
        for b in range(B):
            w = mppi_weights(score[b * K:(b + 1) * K], lam, dt)
            if w is None:
                continue
            num, den = np.zeros((T, 2), dtype=dt), dt(0)
            for k in range(K):
                num = (num + (w[k] * cand[:, b, k, :].astype(dt)).astype(dt)).astype(dt)
                den = dt(den + w[k])
            mean[:, b, :] = (num / den).astype(dt)
    return mean, sigma, chosen, predicted


def mppi_weights(score, lam: float, dtype=np.float64):
    """The path-integral weights of one group as auv_plan_refit forms them, or None where no score is valid: 1 at the largest valid
    score, 0 for a NaN, else exp(float32((float32(score_k - max)) / float32(lam))), evaluated in float64 and rounded to `dtype`."""
    score = np.asarray(score, dtype=np.float32)
    valid = score == score
    if not valid.any():
        return None
    with np.errstate(all="ignore"):
        smax = score[valid].max()
        arg = ((score - smax).astype(np.float32) / np.float32(lam)).astype(np.float32)
        w = np.exp(arg.astype(np.float64)).astype(dtype)
    w[score == smax] = 1
    w[~valid] = 0
    return w


def reference_plan_iterations(mean0, sigma0, K: int, lo, hi, seed: int, draw0: int, records, gamma: float, method: str = "cem",
                              n_elite: int = 1, sigma_min: float = 0.0, lam: float = 1.0, shift: int = 0, reset=None, mean_start=None,
                              terminals=None):
    """The device sampler's loop over the iterations of one plan, composed of the mirrors above: iteration i samples with draw0 + i
    around the current (mean, sigma), scores the recorded (reward, done) of that iteration -- `records[i]`, each [T, B * K] -- with
    reference_plan_score (reference_plan_score_terminal with `terminals[i]`) and refits.  Iteration 0 samples around `mean_start`
    (default mean0) with sigma0 and `shift` / `reset` as given (a warm start: mean_start = the previous plan's refitted mean, shift = 1);
    later iterations use shift 0 and no mask.  A refit follows every record, so pass one record fewer than rings are wanted -- or all
    of them, for the mean a warm start carries on.  Returns (rings, mean, sigma): the rings of iterations 0 .. len(records) (the last
    one only when its distribution is float32, i.e. for "cem", or when no refit preceded it)."""
    mean = np.asarray(mean0 if mean_start is None else mean_start, dtype=np.float32)
    sigma = np.asarray(sigma0, dtype=np.float32)
    rings = [reference_plan_sample(mean, sigma, K, lo, hi, seed, draw0, shift, reset, mean0, sigma0)]
    for i, (reward, done) in enumerate(records):
        if terminals is not None and terminals[i] is not None:
            score, best = reference_plan_score_terminal(reward, done, K, gamma, terminals[i])
        else:
            score, best = reference_plan_score(reward, done, K, gamma)
        mean, sigma, _, _ = reference_plan_refit(rings[-1], score, best, K, method, n_elite, sigma_min, lam, mean, sigma)
        if method == "cem":
            rings.append(reference_plan_sample(mean, sigma, K, lo, hi, seed, draw0 + i + 1))
    return rings, mean, sigma


def _dev_f32(env, t, shape, name):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != env.device:
        raise ValueError("%s must be a contiguous %s float32 tensor on %s" % (name, list(shape), env.device))
    return C.c_void_p(t.data_ptr())


def plan_sample(env, mean: torch.Tensor, sigma: torch.Tensor, K: int, lo, hi, seed: int, draw: int, shift: int = 0,
                reset: Optional[torch.Tensor] = None, mean0: Optional[torch.Tensor] = None, sigma0: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """auv_plan_sample on the caller's current stream: the ring [T, B * K, 2] float32 around mean / sigma [T, B, 2] (device tensors;
    reference_plan_sample is the contract).  lo, hi: two floats each, on the host.  reset: a [B] uint8 device tensor or None."""
    from . import batched_env as be
    if mean.dim() != 3:
        raise ValueError("mean must be [T, B, 2]")
    T, B, K = int(mean.shape[0]), int(mean.shape[1]), int(K)
    ptr = [_dev_f32(env, mean, (T, B, 2), "mean"), _dev_f32(env, sigma, (T, B, 2), "sigma"), None, None, None]
    if reset is not None:
        if reset.dtype != torch.uint8 or tuple(reset.shape) != (B,) or not reset.is_contiguous() or reset.device != env.device:
            raise ValueError("reset must be a contiguous [%d] uint8 tensor on %s" % (B, env.device))
        ptr[2:] = [_dev_f32(env, mean0, (T, B, 2), "mean0"), _dev_f32(env, sigma0, (T, B, 2), "sigma0"), C.c_void_p(reset.data_ptr())]
    if out is None:
        with torch.cuda.device(env.device):
            out = torch.empty((T, B * K, 2), dtype=torch.float32, device=env.device)
    lo_c, hi_c = (C.c_float * 2)(float(lo[0]), float(lo[1])), (C.c_float * 2)(float(hi[0]), float(hi[1]))
    be._check(be._LIB.auv_plan_sample(env._h, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], T, B * K, K, int(shift), lo_c, hi_c,
                                      C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint64(int(draw) & 0xFFFFFFFFFFFFFFFF),
                                      _dev_f32(env, out, (T, B * K, 2), "out"), env._stream()), "auv_plan_sample")
    return out


def plan_refit(env, ring: torch.Tensor, score: torch.Tensor, best: torch.Tensor, K: int, method: str = "cem", n_elite: int = 1,
               sigma_min: float = 0.0, lam: float = 1.0, mean_in: Optional[torch.Tensor] = None, sigma_in: Optional[torch.Tensor] = None,
               mean_out: Optional[torch.Tensor] = None, sigma_out: Optional[torch.Tensor] = None, refit: bool = True):
    """auv_plan_refit on the caller's current stream: (mean, sigma, chosen [T, B, 2], predicted [B]) of a ring [T, B * K, 2] with its
    scores [B * K] and winners [B] (reference_plan_refit is the contract).  refit=False: only chosen and predicted, mean and sigma
    come back None.  mean_out / sigma_out: the caller's output tensors (allocated when None)."""
    from . import batched_env as be
    if method not in PLAN_METHODS:
        raise ValueError("method must be one of %s" % sorted(PLAN_METHODS))
    if ring.dim() != 3:
        raise ValueError("ring must be [T, n, 2]")
    T, n, K = int(ring.shape[0]), int(ring.shape[1]), int(K)
    if K < 1 or n % K:
        raise ValueError("n = %d is not a multiple of K = %d" % (n, K))
    B = n // K
    if best.dtype != torch.int32 or tuple(best.shape) != (B,) or not best.is_contiguous() or best.device != env.device:
        raise ValueError("best must be a contiguous [%d] int32 tensor on %s" % (B, env.device))
    with torch.cuda.device(env.device):
        chosen = torch.empty((T, B, 2), dtype=torch.float32, device=env.device)
        predicted = torch.empty((B,), dtype=torch.float32, device=env.device)
        if refit and mean_out is None:
            mean_out = torch.empty((T, B, 2), dtype=torch.float32, device=env.device)
        if refit and sigma_out is None:
            sigma_out = torch.empty((T, B, 2), dtype=torch.float32, device=env.device)
    if not refit:
        mean_out = sigma_out = None
    opt = lambda t, name: None if t is None else _dev_f32(env, t, (T, B, 2), name)       # noqa: E731
    be._check(be._LIB.auv_plan_refit(env._h, _dev_f32(env, ring, (T, n, 2), "ring"), _dev_f32(env, score, (n,), "score"),
                                     C.c_void_p(best.data_ptr()), T, n, K, PLAN_METHODS[method], int(n_elite), C.c_float(sigma_min),
                                     C.c_float(lam), opt(mean_in, "mean_in"), opt(sigma_in, "sigma_in"), opt(mean_out, "mean_out"),
                                     opt(sigma_out, "sigma_out"), C.c_void_p(chosen.data_ptr()), C.c_void_p(predicted.data_ptr()),
                                     env._stream()), "auv_plan_refit")
    return mean_out, sigma_out, chosen, predicted


def check_planner_options(candidates: int, sampler: str = "torch", method: str = "cem", mppi_lambda: float = 1.0, warm_start: bool = False):
    """What ShootingPlanner refuses of its sampler options, before it touches a device (ValueError)."""
    if sampler not in ("torch", "device"):
        raise ValueError("ShootingPlanner: sampler must be \"torch\" or \"device\", not %r" % (sampler,))
    if method not in PLAN_METHODS:
        raise ValueError("ShootingPlanner: method must be one of %s, not %r" % (sorted(PLAN_METHODS), method))
    if sampler == "torch" and (method != "cem" or warm_start):
        raise ValueError("ShootingPlanner: method=\"mppi\" and warm_start=True need sampler=\"device\"")
    if sampler == "device" and int(candidates) > PLAN_MAX_CANDIDATES:
        raise ValueError("ShootingPlanner: sampler=\"device\" takes at most %d candidates, not %d" % (PLAN_MAX_CANDIDATES, int(candidates)))
    if method == "mppi" and not (np.isfinite(float(mppi_lambda)) and float(mppi_lambda) > 0.0):
        raise ValueError("ShootingPlanner: mppi_lambda must be finite and > 0, not %r" % (mppi_lambda,))


class ShootingPlanner:
    """Random shooting (iterations = 1) or the cross-entropy method (iterations > 1) over `candidates` action sequences of
    `horizon` steps per real environment.

    The planner owns a second BatchedAuvEnv of B * K environments on the real batch's config and world bank (`worlds`: the bank,
    when the real batch cannot name its own).  plan():
        snapshot of the B real environments -> restored K-fold into the planner's batch (environment b * K + k = real b)
        -> [T, B * K, 2] action ring: candidate 0 of every group is the mean sequence, the others Gaussian around it
           (per-dimension `sigma`), clipped to the action space
        -> step_multi(ring, 0, T, record="reward") -> auv_plan_score (auv_plan_score_v with a terminal `value`)
        -> (CEM) mean and sigma refitted from the best `elite_frac` of every group, again from the restore
    and returns (first actions [B, 2], chosen sequences [T, B, 2], their predicted scores [B]) as device tensors.  The sampler
    is a seeded torch.Generator on the device: the same seed and the same states give the same plan (`plan(seed=...)` re-seeds).
    Predictions are exact for what they cover: the simulator is bit-reproducible, so stepping the real batch with a chosen
    sequence realises the predicted rewards up to and including the first done (afterwards the two batches cycle to different
    worlds).  With auto-reset a candidate's score stops at its first done.

    sampler="device": sampling and refit run as two HIP launches per iteration (auv_plan_sample, auv_plan_refit) instead of the
    chain of torch operations -- per iteration restore, sample, step_multi, score, refit: 5 launches (torch: the same three and about 13 small ones).  The noise is
    then counter-based, a function of (seed, draw, environment, step, component) with draw = plans * iterations + iteration, and
    reference_plan_iterations reproduces a plan on the host bit for bit; `plan(seed=s)` sets the seed and puts the draw back to 0.
    The two samplers draw DIFFERENT noise: same distribution family (the device's is a bounded sum of four uniforms, |eps| <= 3.46),
    other plans.  Only with the device sampler:
        method="mppi"     the mean is refitted as the path-integral average, weights exp((score - max) / mppi_lambda) over ALL
                          candidates, and the spread stays; "cem" (default): mean and spread of the elite.
        warm_start=True   receding horizon: a refit also follows the last iteration, and the next plan() samples around that mean
                          moved on one step (its last step repeated) with the initial spread.  plan(reset=mask) -- a [B] uint8 device
                          tensor, e.g. the real batch's `done` after the step just taken -- restarts the masked groups from the
                          mid-range mean (or the prior), as the first plan does for every group.
    plan() returns the best SIMULATED candidate of the last iteration under either method, so the predictions stay exact."""

    def __init__(self, real_env, candidates: int = 64, horizon: int = 16, gamma: float = 0.99, iterations: int = 1,
                 elite_frac: float = 0.125, sigma: Union[float, Sequence[float], None] = None, seed: int = 0, worlds=None,
                 sigma_min: float = 1e-3, value=None, value_scale: float = 1.0, value_shift: float = 0.0, prior=None,
                 sampler: str = "torch", method: str = "cem", mppi_lambda: float = 1.0, warm_start: bool = False):
        check_planner_options(candidates, sampler, method, mppi_lambda, warm_start)
        from .batched_env import BatchedAuvEnv
        from .devgen import FreshWorlds
        K, T = int(candidates), int(horizon)
        if K < 1 or T < 1 or int(iterations) < 1:
            raise ValueError("candidates, horizon and iterations must be >= 1")
        if not 0.0 < float(elite_frac) <= 1.0:
            raise ValueError("elite_frac must be in (0, 1]")
        self.sampler, self.method, self.mppi_lambda, self.warm_start = sampler, method, float(mppi_lambda), bool(warm_start)
        if worlds is None:
            worlds = getattr(real_env, "_worlds_arg", None)
        if worlds is None or isinstance(worlds, FreshWorlds) or real_env._fresh is not None:
            raise ValueError("ShootingPlanner needs the real batch's world bank (not FreshWorlds: a snapshot names its world by bank index)")
        self.real = real_env
        self.B, self.K, self.T = real_env.n_envs, K, T
        self.gamma, self.iterations = float(gamma), int(iterations)
        self.n_elite = max(1, min(K, int(round(float(elite_frac) * K))))
        self.device = real_env.device
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")      # (worlds per environment: the planner's batch never outlives a horizon in them)
            self.sim = BatchedAuvEnv(real_env.config, worlds, self.B * K, device=self.device, **real_env._ctor_args)
        if self.sim.snapshot_layout != real_env.snapshot_layout:
            raise ValueError("the planner's batch does not have the real batch's snapshot layout (another bank?)")
        # one chain on the caller's stream: restore, launch and scoring are then ordered by the stream alone
        with torch.cuda.device(self.device):
            self.sim.set_sub_batches(1, probe_streams=False, inline_first=True)
            lo = torch.as_tensor(real_env.action_space.low, dtype=torch.float32, device=self.device)
            hi = torch.as_tensor(real_env.action_space.high, dtype=torch.float32, device=self.device)
            self._lo, self._hi = lo, hi
            if sigma is None:
                sigma = ((hi - lo) / 4).tolist()          # a quarter of the action range per dimension
            sg = torch.as_tensor(sigma, dtype=torch.float32, device=self.device).reshape(-1)
            self._sigma0 = (sg if sg.numel() == 2 else sg.expand(2)).reshape(1, 1, 2).expand(T, self.B, 2).contiguous()
            self._mean0 = ((lo + hi) / 2).reshape(1, 1, 2).expand(T, self.B, 2).contiguous()
            self._rows = fork_rows(self.B, K).to(self.device)
            self._envs = torch.arange(self.B * K, dtype=torch.int32, device=self.device)
            self._groups = torch.arange(self.B, device=self.device)
            self._gen = torch.Generator(device=self.device)
        self._sigma_min = float(sigma_min)
        self.seed = int(seed)
        self._gen.manual_seed(self.seed)
        self.last = None
        self.plans = 0
        # the device sampler: its draw counter, the action bounds as host floats, two (mean, sigma) pairs written in turn (a refit
        # never writes what its iteration's sampler read) and the mean a warm start carries into the next plan
        self._dev_seed, self._draw = self.seed, 0
        self._lo_host = [float(x) for x in np.asarray(real_env.action_space.low, dtype=np.float32).reshape(-1)]
        self._hi_host = [float(x) for x in np.asarray(real_env.action_space.high, dtype=np.float32).reshape(-1)]
        self._fit = None
        self._warm_mean = None
        if sampler == "device":
            with torch.cuda.device(self.device):
                self._fit = [tuple(torch.empty((T, self.B, 2), dtype=torch.float32, device=self.device) for _ in range(2)) for _ in range(2)]
        for name, f in (("value", value), ("prior", prior)):
            if f is not None and hasattr(f, "params") and f.env.obs_dim != real_env.obs_dim:
                raise ValueError("ShootingPlanner: %s was built for observations of %d columns, the planner's have %d" % (name, f.env.obs_dim, real_env.obs_dim))
        if value is not None and not (hasattr(value, "params") or callable(value)):
            raise ValueError("ShootingPlanner: value must be a FusedActorCritic or a callable obs [n, D] -> [n]")
        if prior is not None and not hasattr(prior, "params"):
            raise ValueError("ShootingPlanner: prior must be a FusedActorCritic")
        self.value, self.prior = value, prior
        self.value_scale, self.value_shift = float(value_scale), float(value_shift)

    def _terminal(self) -> torch.Tensor:
        """value(sim.obs) * value_scale + value_shift of the planner's batch after the launch, [B * K] float32."""
        from .policy import policy_eval
        obs = self.sim.obs
        if hasattr(self.value, "params"):
            v = policy_eval(self.value.params, self.sim.obs_dim, obs, want=("value",))["value"]
        else:
            v = self.value(obs)
            if not isinstance(v, torch.Tensor) or v.numel() != obs.shape[0] or v.device != obs.device:
                raise ValueError("ShootingPlanner: value(obs) must return %d values on %s" % (obs.shape[0], obs.device))
            v = v.reshape(-1).to(torch.float32)
        if self.value_scale != 1.0 or self.value_shift != 0.0:
            v = v * self.value_scale + self.value_shift
        return v.contiguous()

    def _plan_device(self, reset: Optional[torch.Tensor]):
        """plan() with sampler="device": per iteration restore, auv_plan_sample, step_multi, the scorer, auv_plan_refit."""
        B, K, T, sim = self.B, self.K, self.T, self.sim
        snap = self.real.snapshot()
        terminal = None
        history = []
        with torch.cuda.device(self.device):
            mean0 = self._mean0
            if self.prior is not None:
                from .policy import policy_eval
                a0 = policy_eval(self.prior.params, self.real.obs_dim, self.real.obs, want=("action",), action_map=self.prior.action_map)["action"]
                mean0 = a0.reshape(1, B, 2).expand(T, B, 2).contiguous()
            mean, sigma, shift = mean0, self._sigma0, 0
            if self._warm_mean is not None:
                mean, shift = self._warm_mean, 1                       # (masked groups: mean0, unshifted)
            else:
                reset = None                                              # (the first plan: every group starts from mean0 anyway)
            for it in range(self.iterations):
                sim.restore(snap, rows=self._rows, envs=self._envs, validate=False)
                ring = plan_sample(sim, mean, sigma, K, self._lo_host, self._hi_host, self._dev_seed, self._draw, shift,
                                   reset if it == 0 else None, mean0, self._sigma0)
                self._draw += 1
                _, rew, done = sim.step_multi(ring, 0, T, record="reward")
                sim._join_chains()
                if self.value is not None:
                    terminal = self._terminal()
                score, best = plan_score(sim, rew, done, K, self.gamma, terminal)
                refit = it + 1 < self.iterations or self.warm_start
                out = self._fit[0]
                new_mean, new_sigma, chosen, predicted = plan_refit(sim, ring, score, best, K, self.method, self.n_elite, self._sigma_min,
                                                                    self.mppi_lambda, mean, sigma, out[0], out[1], refit=refit)
                history.append(dict(ring=ring, reward=rew, done=done, score=score, best=best, terminal=terminal))
                if refit:
                    mean, sigma, shift = new_mean, new_sigma, 0
                    self._fit.reverse()                                   # the next refit writes the other pair
            if self.warm_start:
                self._warm_mean = mean
        self.last = dict(ring=ring, reward=rew, done=done, score=score, best=best, iterations=history, mean=mean, sigma=sigma)
        if terminal is not None:
            self.last["terminal"] = terminal
        self.plans += 1
        return chosen[0], chosen, predicted

    def plan(self, seed: Optional[int] = None, reset: Optional[torch.Tensor] = None):
        """One decision for every real environment: (actions [B, 2], sequences [T, B, 2], predicted scores [B]).  `self.last` keeps
        the last iteration's ring, reward / done record, scores and winners (device tensors) for inspection; with the device
        sampler also every iteration's (`iterations`) and the distribution the plan ended with (`mean`, `sigma`: views of buffers
        the next plan overwrites).  `reset`: only with warm_start=True, a [B] uint8 device tensor -- groups that start afresh."""
        if reset is not None and not self.warm_start:
            raise ValueError("ShootingPlanner.plan: reset is for warm_start=True (no other plan carries anything over)")
        if reset is not None and (not isinstance(reset, torch.Tensor) or reset.dtype != torch.uint8 or tuple(reset.shape) != (self.B,)
                                  or not reset.is_contiguous() or reset.device != self.device):
            raise ValueError("ShootingPlanner.plan: reset must be a contiguous [%d] uint8 tensor on %s" % (self.B, self.device))
        if seed is not None:
            self._dev_seed, self._draw = int(seed), 0
            self._gen.manual_seed(int(seed))
        if self.sampler == "device":
            return self._plan_device(reset)
        B, K, T, sim = self.B, self.K, self.T, self.sim
        snap = self.real.snapshot()
        mean, sigma = self._mean0, self._sigma0
        terminal = None
        with torch.cuda.device(self.device):
            if self.prior is not None:
                # the policy's deterministic action at the real observation, held over the horizon
                from .policy import policy_eval
                a0 = policy_eval(self.prior.params, self.real.obs_dim, self.real.obs, want=("action",), action_map=self.prior.action_map)["action"]
                mean = a0.reshape(1, B, 2).expand(T, B, 2).contiguous()
            for it in range(self.iterations):
                sim.restore(snap, rows=self._rows, envs=self._envs, validate=False)
                noise = torch.randn((T, B, K, 2), generator=self._gen, device=self.device, dtype=torch.float32)
                cand = mean[:, :, None, :] + sigma[:, :, None, :] * noise
                cand[:, :, 0, :] = mean                                   # candidate 0: the mean sequence itself
                cand = torch.maximum(torch.minimum(cand, self._hi), self._lo)
                ring = cand.reshape(T, B * K, 2)
                _, rew, done = sim.step_multi(ring, 0, T, record="reward")
                sim._join_chains()
                if self.value is not None:
                    terminal = self._terminal()
                score, best = plan_score(sim, rew, done, K, self.gamma, terminal)
                if it + 1 < self.iterations:
                    # cross-entropy refit: mean and spread of the elite sequences of every group
                    elite = torch.nan_to_num(score, nan=float("-inf")).view(B, K).topk(self.n_elite, dim=1).indices      # [B, E]
                    seqs = torch.gather(cand, 2, elite[None, :, :, None].expand(T, B, self.n_elite, 2))
                    mean = seqs.mean(dim=2)
                    sigma = seqs.std(dim=2, unbiased=False).clamp_min(self._sigma_min)
            bl = best.long()
            chosen = cand[:, self._groups, bl, :].contiguous()                # [T, B, 2]
            predicted = score.view(B, K).gather(1, bl[:, None]).squeeze(1)
        self.last = dict(ring=ring, reward=rew, done=done, score=score, best=best)
        if terminal is not None:
            self.last["terminal"] = terminal                              # (only with a `value`: the last iteration's terminal values)
        self.plans += 1
        return chosen[0], chosen, predicted

    def close(self):
        self.sim.close()


class DistillBuffer:
    """A ring of supervised targets on the device: O [capacity, obs_dim], A [capacity, 2] (target actions in the POLICY's own space),
    RET [capacity] (value targets), W [capacity] (row weights) -- the stored rows FusedPPOUpdate.clone_step gathers from.

        buf = DistillBuffer(65536, env.obs_dim, env.device)
        a, _, predicted = planner.plan()
        buf.add(env.obs, *DistillBuffer.targets_from_plan(planner, a, predicted))
        upd.clone_step(buf.O, buf.A, buf.RET, buf.W, buf.sample(256, gen))

    add() writes with index_copy_ at positions that follow from the batch's size alone: nothing synchronises with the host."""

    def __init__(self, capacity: int, obs_dim: int, device):
        if int(capacity) < 1 or int(obs_dim) < 1:
            raise ValueError("DistillBuffer: capacity and obs_dim must be >= 1")
        self.capacity, self.obs_dim, self.device = int(capacity), int(obs_dim), torch.device(device)
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=self.device)   # noqa: E731
        self.O, self.A, self.RET, self.W = z(self.capacity, self.obs_dim), z(self.capacity, 2), z(self.capacity), z(self.capacity)
        self.head = 0                                             # the next row to write
        self.size = 0                                             # filled rows: 0 .. capacity

    def add(self, obs: torch.Tensor, actions: torch.Tensor, ret: torch.Tensor, w: Optional[torch.Tensor] = None):
        """Append n rows (the oldest are overwritten once the ring is full; of a batch longer than the ring the last `capacity` rows
        stay).  obs [n, obs_dim], actions [n, 2], ret [n], w [n] or None (all one)."""
        n = int(obs.shape[0])
        if tuple(obs.shape) != (n, self.obs_dim) or tuple(actions.shape) != (n, 2) or tuple(ret.shape) != (n,) \
                or (w is not None and tuple(w.shape) != (n,)):
            raise ValueError("DistillBuffer.add: expected obs [n, %d], actions [n, 2], ret [n] and w [n] or None" % self.obs_dim)
        if n == 0:
            return
        if w is None:
            w = torch.ones((n,), dtype=torch.float32, device=self.device)
        cols = [x.detach().to(device=self.device, dtype=torch.float32) for x in (obs, actions, ret, w)]
        if n > self.capacity:
            self.head = (self.head + n - self.capacity) % self.capacity
            cols, n = [x[-self.capacity:] for x in cols], self.capacity
        pos = (torch.arange(n, dtype=torch.int64, device=self.device) + self.head) % self.capacity
        for dst, src in zip((self.O, self.A, self.RET, self.W), cols):
            dst.index_copy_(0, pos, src)
        self.head = (self.head + n) % self.capacity
        self.size = min(self.capacity, self.size + n)

    def sample(self, B: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """[B] int64 on the device: rows drawn uniformly, with replacement, from the filled part."""
        if self.size < 1:
            raise ValueError("DistillBuffer.sample: the buffer is empty")
        return torch.randint(0, self.size, (int(B),), generator=generator, device=self.device, dtype=torch.int64)

    @staticmethod
    def targets_from_plan(planner, first_actions: torch.Tensor, predicted: torch.Tensor):
        """A plan's outputs as the policy's targets: (mu* [B, 2], ret [B]).  The planner decides in ENVIRONMENT actions; the policy's
        mean reaches the environment through the prior's affine map action = mid + half * clip(mu), so mu* = (a - mid) / half.  The
        predicted scores are in the planner's reward units, value * value_scale + value_shift: ret = (predicted - shift) / scale."""
        prior = planner.prior
        mid, half = (0.0, 0.0), (1.0, 1.0)
        if prior is not None and getattr(prior, "action_map", None) is not None:
            mid, half = prior.action_map[0], prior.action_map[1]
        if any(float(h) == 0.0 for h in half):
            raise ValueError("DistillBuffer.targets_from_plan: the action map's half-range %s has a zero: it cannot be inverted" % (tuple(half),))
        if planner.value_scale == 0.0:
            raise ValueError("DistillBuffer.targets_from_plan: value_scale is 0: the scores cannot be mapped back")
        mid_t = torch.as_tensor(mid, dtype=first_actions.dtype, device=first_actions.device)
        half_t = torch.as_tensor(half, dtype=first_actions.dtype, device=first_actions.device)
        mu = (first_actions - mid_t) / half_t
        ret = predicted if planner.value_scale == 1.0 and planner.value_shift == 0.0 else (predicted - planner.value_shift) / planner.value_scale
        return mu.contiguous(), ret.contiguous()
