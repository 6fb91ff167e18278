"""RunningNorm -- running observation and reward normalisation for the fused rollout (csrc/k16_policy_norm.hip): what stable-baselines
ships as VecNormalize.  Running mean and variance of the observations, applied inside the policy launch; rewards divided by the running
deviation of the discounted return.

    norm = RunningNorm(env.obs_dim, gamma=0.999)
    fused = FusedActorCritic(net, env, rollout=T, normalize=norm)
    fused.begin_rollout(); fused.rollout(T)          # the launches normalise with a frozen table and leave per-tile moments
    ...                                              # order the caller's stream behind the chains (wait_stream), as for gae()
    norm.fold()                                      # the rollout's raw rows into the running moments, the table rewritten
    norm.returns(fused.R, fused.Dn)                  # discounted returns into their moments, R scaled in place
    fused.predict() / value() / evaluate()           # see normalised rows: normalize() in front of auv_policy_eval

DEVIATION from stable-baselines (include/auv_hip.h): its statistics move at every step_wait, before that step's batch is
normalised.  Here they are FROZEN while launches run and FOLDED between rollouts -- a per-step update would be a reduction over all
environments between the environment's and the policy's launch of every step, a barrier across chains that are not ordered against each
other.  The first rollout therefore runs on the initial table (mean 0, variance 1); a rollout's rewards are scaled by a deviation that
holds all of that rollout's returns.  `training = False` is VecNormalize.training: the table is used, nothing is folded, `ret` stands still.

The NumPy functions below restate the kernels operation for operation (float32 where the kernel computes in f32, float64 where it computes
in fp64, the same association and the same merge order); tests/test_gpu_normalize.py compares bits.
"""
import ctypes as C
from typing import Optional, Sequence

import numpy as np

INIT_COUNT = 1e-4      # stable-baselines' RunningMeanStd: mean 0, variance 1, count 1e-4
TILE = 16              # rows of a policy workgroup's tile (csrc/auv_policy_mfma.h, POL_ROWS)
WAVE = 64


# ------------------------------------------------------------------------------ the mirrors
def norm_rows(x, table, clip_obs):
    """min(max((x - mean) * inv_std, -clip), clip) in float32, three separately rounded operations: the act launch's tile step and
    auv_norm_rows.  x [..., D] float32, table [D, 2] float32."""
    x = np.asarray(x, dtype=np.float32)
    table = np.asarray(table, dtype=np.float32)
    c = np.float32(clip_obs)
    y = (x - table[:, 0]) * table[:, 1]
    return np.minimum(np.maximum(y, -c), c).astype(np.float32)


def tile_moments(rows):
    """(m, M2), float32 [D] each, of the rows [n <= 16, D] of one tile: m = s / n of the sequential sum s over rows 0 .. n - 1, M2 the
    sequential sum of (x_r - m)^2."""
    rows = np.asarray(rows, dtype=np.float32)
    n = rows.shape[0]
    if n < 1 or n > TILE:
        raise ValueError("tile_moments: a tile has 1 .. %d rows, got %d" % (TILE, n))
    s = np.zeros(rows.shape[1], dtype=np.float32)
    for r in range(n):
        s = s + rows[r]
    m = (s / np.float32(n)).astype(np.float32)
    M2 = np.zeros(rows.shape[1], dtype=np.float32)
    for r in range(n):
        d = rows[r] - m
        M2 = M2 + d * d
    return m, M2


def slice_partials(obs, bounds):
    """The (part [slots, 2, D], pcnt [slots]) one launch position leaves for the raw rows obs [N, D] cut into the slices
    [bounds[i], bounds[i + 1]): every slice's tiles in order, the last one of a slice ragged."""
    obs = np.asarray(obs, dtype=np.float32)
    part, cnt = [], []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        for r0 in range(lo, hi, TILE):
            rows = obs[r0:min(r0 + TILE, hi)]
            part.append(np.stack(tile_moments(rows)))
            cnt.append(rows.shape[0])
    return np.stack(part), np.asarray(cnt, dtype=np.int32)


def _merge(a, b):
    """Chan's pairwise merge, vectorised over leading axes: a, b = (n, mean, M2) float64 arrays.  b.n == 0 gives a, a.n == 0 gives b."""
    an, am, aM = a
    bn, bm, bM = b
    with np.errstate(invalid="ignore", divide="ignore"):
        tot = an + bn
        delta = bm - am
        mean = am + (delta * bn) / tot
        M2 = (aM + bM) + (((delta * delta) * an) * bn) / tot
    take_a, take_b = bn == 0.0, (an == 0.0) & (bn != 0.0)
    n = np.where(take_a, an, np.where(take_b, bn, tot))
    mean = np.where(take_a, am, np.where(take_b, bm, mean))
    M2 = np.where(take_a, aM, np.where(take_b, bM, M2))
    return n, mean, M2


def _merge_lanes(n, mean, M2):
    """n, mean, M2 [S, ...] -- S sets in order -> one set: lane l merges sets l, l + 64, ... in that order, then the tree for
    o = 32 .. 1: lane l < o becomes merge(lane l, lane l + o)."""
    S = n.shape[0]
    shape = (WAVE,) + n.shape[1:]
    a = tuple(np.zeros(shape, dtype=np.float64) for _ in range(3))
    for s0 in range(0, S, WAVE):
        k = min(WAVE, S - s0)
        b = []
        for x in (n, mean, M2):
            y = np.zeros(shape, dtype=np.float64)
            y[:k] = x[s0:s0 + k]
            b.append(y)
        a = _merge(a, tuple(b))
    o = WAVE // 2
    while o >= 1:
        lo = _merge(tuple(x[:o] for x in a), tuple(x[o:2 * o] for x in a))
        a = lo
        o //= 2
    return tuple(x[0] for x in a)


def fold_moments(part, pcnt, mom, eps):
    """auv_norm_fold: part [S, 2, D] float32 and pcnt [S] int32 merged into mom [D, 3] float64 = (count, mean, M2).  Returns
    (mom', table') with table' [D, 2] float32 = (mean, 1 / sqrt(M2 / count + eps))."""
    part = np.asarray(part, dtype=np.float32)
    pcnt = np.asarray(pcnt, dtype=np.int32)
    mom = np.asarray(mom, dtype=np.float64)
    D = part.shape[2]
    n = np.repeat(np.where(pcnt > 0, pcnt, 0).astype(np.float64)[:, None], D, axis=1)
    batch = _merge_lanes(n, part[:, 0].astype(np.float64), part[:, 1].astype(np.float64))
    rn, rm, rM = _merge((mom[:, 0], mom[:, 1], mom[:, 2]), batch)
    out = np.stack([rn, rm, rM], axis=1)
    inv = 1.0 / np.sqrt(rM / rn + np.float64(eps))
    return out, np.stack([rm.astype(np.float32), inv.astype(np.float32)], axis=1)


def return_pass(R, Dn, ret, rmom, gamma, eps, clip_reward, update=True):
    """auv_norm_returns: R, Dn [T, N] float32, ret [N] float64, rmom [3] float64 = (count, mean, M2).  Returns (ret', rmom', R')."""
    R = np.asarray(R, dtype=np.float32)
    Dn = np.asarray(Dn, dtype=np.float32)
    g = np.array(ret, dtype=np.float64)
    rmom = np.array(rmom, dtype=np.float64)
    T, N = R.shape
    if update:
        mean, M2 = np.zeros(N), np.zeros(N)
        gam = np.float64(gamma)
        for t in range(T):
            g = g * gam + R[t].astype(np.float64)
            d = g - mean
            mean = mean + d / np.float64(t + 1)
            M2 = M2 + d * (g - mean)
            g = np.where(Dn[t] != 0.0, 0.0, g)
        batch = _merge_lanes(np.full(N, float(T)), mean, M2)
        rmom = np.array(_merge((rmom[0], rmom[1], rmom[2]), batch), dtype=np.float64)
    sd = np.float32(np.sqrt(rmom[2] / rmom[0] + np.float64(eps)))
    c = np.float32(clip_reward)
    return g, rmom, np.minimum(np.maximum(R / sd, -c), c).astype(np.float32)


# ------------------------------------------------------------------------------ the device state
class RunningNorm:
    """The state of the normalisation and the launches that move it on.  The statistics live in torch tensors (on the CPU until `bind`
    or `to` moves them): table [D, 2] f32, obs_mom [D, 3] f64, ret_mom [3] f64, and -- once bound to a batch -- ret [N] f64 and the
    launches' partial buffers part [T * part_ld, 2, D] f32 / pcnt [T * part_ld] i32, part_base[i] the prefix sum of ceil(ne_i / 16)."""

    def __init__(self, obs_dim: int, gamma: float, norm_obs: bool = True, norm_reward: bool = True, clip_obs: float = 10.0,
                 clip_reward: float = 10.0, eps: float = 1e-8, device="cpu"):
        import torch
        self.obs_dim, self.gamma = int(obs_dim), float(gamma)
        if self.obs_dim < 1:
            raise ValueError("RunningNorm: obs_dim must be >= 1")
        if not (clip_obs > 0 and clip_reward > 0):
            raise ValueError("RunningNorm: clip_obs and clip_reward must be > 0")
        if not (eps >= 0 and np.isfinite(eps) and np.isfinite(gamma)):
            raise ValueError("RunningNorm: eps must be finite and >= 0, gamma finite")
        self.norm_obs, self.norm_reward = bool(norm_obs), bool(norm_reward)
        self.clip_obs, self.clip_reward, self.eps = float(clip_obs), float(clip_reward), float(eps)
        self.training = True
        self.device = torch.device(device)
        D = self.obs_dim
        self.obs_mom = torch.zeros((D, 3), dtype=torch.float64)
        self.obs_mom[:, 0], self.obs_mom[:, 2] = INIT_COUNT, INIT_COUNT              # variance 1: M2 = count
        self.ret_mom = torch.tensor([INIT_COUNT, 0.0, INIT_COUNT], dtype=torch.float64)
        self.table = torch.zeros((D, 2), dtype=torch.float32)
        self.table[:, 1] = float(np.float32(1.0 / np.sqrt(1.0 + np.float64(self.eps))))
        self.ret = None
        self.part = self.pcnt = self.rpart = None
        self.part_base, self.part_ld, self.T, self.n = [], 0, 0, 0
        self.to(self.device)

    def to(self, device):
        import torch
        self.device = torch.device(device)
        for name in ("obs_mom", "ret_mom", "table", "ret", "part", "pcnt", "rpart"):
            t = getattr(self, name)
            if t is not None:
                setattr(self, name, t.to(self.device))
        return self

    def bind(self, n_envs: int, T: int, slices: Sequence, device):
        """Size the per-batch buffers for rollouts of T steps over `slices` = [(lo, cnt), ...] (FusedActorCritic calls this)."""
        import torch
        self.to(device)
        self.n, self.T = int(n_envs), int(T)
        tiles = [-(-int(cnt) // TILE) for _, cnt in slices]
        self.part_base = [int(x) for x in np.concatenate([[0], np.cumsum(tiles)[:-1]])]
        self.part_ld = int(sum(tiles))
        slots = self.T * self.part_ld
        self.part = torch.zeros((slots, 2, self.obs_dim), dtype=torch.float32, device=self.device)
        self.pcnt = torch.zeros(slots, dtype=torch.int32, device=self.device)
        self.ret = torch.zeros(self.n, dtype=torch.float64, device=self.device)
        self.rpart = torch.zeros((self.n, 2), dtype=torch.float64, device=self.device)
        return self

    # ---- launches (on the caller's current stream; the caller orders them against the chains, as for gae()) ----
    def _dev(self):
        import torch
        return self.device.index if self.device.index is not None else torch.cuda.current_device()

    def fold(self):
        """The partials the launches since the last fold have left -> the running observation moments, the table rewritten (auv_norm_fold);
        the slots are then emptied.  Nothing happens with training == False or norm_obs == False."""
        import torch
        if not (self.training and self.norm_obs):
            return
        if self.part is None:
            raise RuntimeError("RunningNorm.fold: not bound to a batch (FusedActorCritic(normalize=...) binds it)")
        from .batched_env import _check, _LIB
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream(self.device)
            _check(_LIB.auv_norm_fold(self._dev(), C.c_void_p(self.part.data_ptr()), C.c_void_p(self.pcnt.data_ptr()), int(self.pcnt.numel()),
                                      self.obs_dim, self.eps, C.c_void_p(self.obs_mom.data_ptr()), C.c_void_p(self.table.data_ptr()),
                                      C.c_void_p(st.cuda_stream)), "auv_norm_fold")
            self.pcnt.zero_()

    def returns(self, R, Dn, out=None):
        """The reward pass over a stored rollout R, Dn [T, N] (auv_norm_returns): with training, the discounted returns into their running
        moments; then R scaled by the updated deviation and clipped, in place (or into `out`).  Returns the scaled tensor.  Nothing happens
        with norm_reward == False."""
        import torch
        if not self.norm_reward:
            return R
        out = R if out is None else out
        T, N = int(R.shape[0]), int(R.shape[1])
        for name, t in (("R", R), ("Dn", Dn), ("out", out)):
            if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (T, N) or t.device != self.device:
                raise ValueError("RunningNorm.returns: %s must be a contiguous float32 [T, N] tensor on %s" % (name, self.device))
        upd = bool(self.training)
        if upd and (self.ret is None or N != self.n):
            raise ValueError("RunningNorm.returns: N = %d, bound to %d environments" % (N, self.n))
        from .batched_env import _check, _LIB
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream(self.device)
            _check(_LIB.auv_norm_returns(self._dev(), C.c_void_p(R.data_ptr()), C.c_void_p(Dn.data_ptr()), C.c_void_p(out.data_ptr()), T, N,
                                         self.gamma, self.clip_reward, self.eps, C.c_void_p(self.ret.data_ptr()) if upd else None,
                                         C.c_void_p(self.rpart.data_ptr()) if upd else None, C.c_void_p(self.ret_mom.data_ptr()),
                                         int(upd), C.c_void_p(st.cuda_stream)), "auv_norm_returns")
        return out

    def normalize(self, rows, idx=None, out=None):
        """[M, obs_dim] raw rows (rows may be strided) -> normalised rows with the current table (auv_norm_rows): the bits the act launch
        stores in O.  norm_obs == False: the rows as they are."""
        import torch
        if not self.norm_obs:
            return rows if idx is None else rows[idx]
        if rows.dtype != torch.float32 or rows.dim() != 2 or rows.shape[1] != self.obs_dim or rows.device != self.device:
            raise ValueError("RunningNorm.normalize: rows must be a float32 [M, %d] tensor on %s" % (self.obs_dim, self.device))
        if rows.shape[0] > 0 and rows.stride(1) != 1:
            raise ValueError("RunningNorm.normalize: the columns of rows must be contiguous")
        if idx is not None and (idx.dtype != torch.int64 or not idx.is_contiguous() or idx.device != self.device):
            raise ValueError("RunningNorm.normalize: idx must be a contiguous int64 tensor on %s" % self.device)
        M = int(rows.shape[0] if idx is None else idx.numel())
        if out is None:
            out = torch.empty((M, self.obs_dim), dtype=torch.float32, device=self.device)
        elif out.dtype != torch.float32 or tuple(out.shape) != (M, self.obs_dim) or not out.is_contiguous() or out.device != self.device:
            raise ValueError("RunningNorm.normalize: out must be a contiguous float32 [%d, %d] tensor" % (M, self.obs_dim))
        if M == 0:
            return out
        from .batched_env import _check, _LIB
        ldx = int(rows.stride(0)) if rows.shape[0] > 1 else self.obs_dim
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream(self.device)
            _check(_LIB.auv_norm_rows(self._dev(), C.c_void_p(rows.data_ptr()), C.c_void_p(idx.data_ptr()) if idx is not None else None, ldx,
                                      C.c_void_p(self.table.data_ptr()), self.clip_obs, C.c_void_p(out.data_ptr()), self.obs_dim, M,
                                      self.obs_dim, C.c_void_p(st.cuda_stream)), "auv_norm_rows")
        return out

    # ---- state ----
    _STATE = ("obs_mom", "ret_mom", "table", "ret")

    def state_dict(self):
        """Every statistic as a CPU copy (ret: None until bound), and the settings they were gathered under."""
        d = {k: (None if getattr(self, k) is None else getattr(self, k).detach().cpu().clone()) for k in self._STATE}
        d["settings"] = dict(obs_dim=self.obs_dim, gamma=self.gamma, clip_obs=self.clip_obs, clip_reward=self.clip_reward, eps=self.eps,
                             norm_obs=self.norm_obs, norm_reward=self.norm_reward)
        return d

    def load_state_dict(self, d):
        if int(d["settings"]["obs_dim"]) != self.obs_dim:
            raise ValueError("RunningNorm.load_state_dict: statistics of %d columns, this one has %d" % (d["settings"]["obs_dim"], self.obs_dim))
        for k in self._STATE:
            src, cur = d[k], getattr(self, k)
            if src is None:
                continue
            if cur is None:
                setattr(self, k, src.clone().to(self.device))
            else:
                if tuple(cur.shape) != tuple(src.shape):
                    raise ValueError("RunningNorm.load_state_dict: %s has shape %s, expected %s" % (k, tuple(src.shape), tuple(cur.shape)))
                cur.copy_(src)                          # (in place: the launches' io blocks hold the table's address)
