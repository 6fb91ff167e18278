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
    worlds).  With auto-reset a candidate's score stops at its first done."""

    def __init__(self, real_env, candidates: int = 64, horizon: int = 16, gamma: float = 0.99, iterations: int = 1,
                 elite_frac: float = 0.125, sigma: Union[float, Sequence[float], None] = None, seed: int = 0, worlds=None,
                 sigma_min: float = 1e-3, value=None, value_scale: float = 1.0, value_shift: float = 0.0, prior=None):
        from .batched_env import BatchedAuvEnv
        from .devgen import FreshWorlds
        K, T = int(candidates), int(horizon)
        if K < 1 or T < 1 or int(iterations) < 1:
            raise ValueError("candidates, horizon and iterations must be >= 1")
        if not 0.0 < float(elite_frac) <= 1.0:
            raise ValueError("elite_frac must be in (0, 1]")
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

    def plan(self, seed: Optional[int] = None):
        """One decision for every real environment: (actions [B, 2], sequences [T, B, 2], predicted scores [B]).  `self.last` keeps
        the last iteration's ring, reward / done record, scores and winners (device tensors) for inspection."""
        if seed is not None:
            self._gen.manual_seed(int(seed))
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
