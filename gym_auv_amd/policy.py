"""FusedActorCritic -- the PPO policy in the loop as ONE HIP launch per sub-batch and step (csrc/k6_policy.hip).

The reference trains PPO2 with `MlpPolicy`, net_arch [256, 128, 64] for policy and value function
(/root/reference/scripts/run.py:332-357), stepping its environments through a VecEnv (run.py:293-296).  With thousands of
environments per GPU stepping in ~30 us, evaluating the two small MLPs with stock tensor operations (eight GEMMs and a
dozen element-wise launches per step) is what bounds a rollout.  This class keeps the torch modules as the owner of the
weights -- the optimiser updates them as usual -- and evaluates them during rollouts with `auv_policy_act`: observation
rows -> actor and critic on the matrix cores in f32 -> sampled action into the environment's action buffer, log-probability
and value into the rollout buffers; reward / done of the previous step are stored by the same launch.

    fused = FusedActorCritic(net, env, rollout=T, reward_scale=0.01)     # net.pi / net.v: Linear-Tanh x 3 + Linear, net.log_std
    fused.refresh()                                # after every optimiser step: repack the weights (device-side copies)
    fused.begin_rollout()                          # t = 0 on every chain
    fused.rollout(T)                               # T steps of every sub-batch chain, policy + env.step, one C call
    O, A, LP, V, R, Dn = fused.buffers()           # [T, N, ...] views for the update

Frame stacking (what stable-baselines ships as VecFrameStack; csrc/k12_policy_stacked.hip): `FusedActorCritic(net, env, T, frames=k)` with a
net whose first layers take k * obs_dim columns evaluates every environment on its last k observations, NEWEST FIRST (columns [j * obs_dim,
(j + 1) * obs_dim) = the observation of j steps ago; a column permutation of stable-baselines' newest-last order), zeros where the episode
is younger than j steps.  The history lives on the device (`fused.stack`: gym_auv_amd/framestack.py) and is moved on by the policy launch
itself; O is then [T, N, k * obs_dim] and everything behind the first layer -- FusedPPOUpdate, policy_eval, the planner -- takes those rows
as they are.  Call `fused.reset_frames()` behind an `env.reset()`.

Running normalisation (what stable-baselines ships as VecNormalize; gym_auv_amd/normalize.py, csrc/k16_policy_norm.hip):
`FusedActorCritic(net, env, T, normalize=RunningNorm(env.obs_dim, gamma))` sends rollouts through the normalising launch -- O then holds the
NORMALISED rows, so the fused update, gae() and the clone step take them as they are -- and predict / value / evaluate normalise the rows
they are given.  The statistics are frozen during a rollout and folded behind it (`normalize.fold()`, `normalize.returns(R, Dn)`).  Not
together with frames > 1 or bf16.

Tanh-squashed actions (what stable-baselines3 calls squash_output; csrc/k17_policy_squash.hip): `FusedActorCritic(net, env, T, squash=True)`
hands the environment act_mid + act_half * tanh(u) of the sample u = mu + sigma eps -- a bounded action whose entropy the update can see
(FusedPPOUpdate(..., squash=True)) -- in the place of the clipped affine map; clip_lo / clip_hi are not consulted.  A holds u itself and LP
its Gaussian log-density, exactly as without the option (the PPO ratio needs no Jacobian), so everything behind the rollout takes the
buffers as they are; predict() gives act_mid + act_half * tanh(mu), and evaluate() takes PRE-SQUASH actions (rows of A).  Not together
with frames > 1, normalize, bf16 or a PolicyPopulation: those launches have no squashed variant.

Hidden widths: read off `net.pi` / `net.v` (both the same triple), one of SUPPORTED_HIDDEN -- the reference's [256, 128, 64] and the
narrower [128, 128, 64], [128, 64, 64], [64, 64, 64] the launches are also compiled for (csrc/auv_policy_mfma.h, POL_ARCH_LIST; the
auv_policy_*_arch entries).  Anything else raises ValueError; bf16 exists for the reference's widths only.
"""
import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from . import _capi
from .batched_env import BatchedAuvEnv, _check, _LIB
from .population import _GEN_MUL, _U64, _mix

HIDDEN = (256, 128, 64)                 # the reference's hidden widths: the default, evaluated by the entries without _arch
SUPPORTED_HIDDEN = _capi.POLICY_ARCHS   # the closed list the forward launches are compiled for (csrc/auv_policy_mfma.h, POL_ARCH_LIST)


def _pad16(x: int) -> int:
    return (x + 31) & ~31          # (rows are padded to the kernel's k-step of 32 columns)


def check_hidden(hidden, who: str) -> tuple:
    """`hidden` as a tuple of three ints if the fused forward launches are compiled for it; ValueError with the list otherwise."""
    try:
        h = tuple(int(x) for x in hidden)
    except (TypeError, ValueError):
        h = None
    if h is None or len(h) != 3:
        raise ValueError("%s: the fused kernels evaluate three hidden tanh layers (another depth is not compiled in), one of %s; got %r"
                         % (who, list(SUPPORTED_HIDDEN), hidden))
    if h not in SUPPORTED_HIDDEN:
        raise ValueError("%s: hidden widths %s are not compiled in: the fused kernels evaluate one of %s" % (who, list(h), list(SUPPORTED_HIDDEN)))
    return h


def _arch_arg(hidden) -> "_capi.AuvPolicyArch":
    return _capi.AuvPolicyArch(int(hidden[0]), int(hidden[1]), int(hidden[2]))


# ------------------------------------------------------------------------------ NumPy mirrors of the act launch's epilogue and of k6_gae
# (csrc/auv_policy_forward.h: pol_gauss, pol_act_sample, pol_logp, pol_act_map; csrc/k6_policy.hip: k6_gae.)  `dtype` = float64 is the
# reference the tests hold the kernels to; float32 restates the kernel's own operations in its order, every operation rounded once
# (log / cos / exp are evaluated in float64 and rounded, so that the restatement does not depend on the host's float32 libm) and
# nothing contracted: what tests/policy_epilogue_cases.py derives its bounds from.  They need no device.
def chain_seed(seed: int, i: int) -> int:
    """The generator seed of sub-batch chain `i` of a FusedActorCritic made with `seed` (auv_policy_io::seed)."""
    return (int(seed) * 0x9E3779B97F4A7C15 + int(i)) & _U64


def _rounded(fn, x, dtype):
    return fn(np.asarray(x, dtype=np.float64)).astype(dtype)


def policy_noise_hash(seed: int, step, env, comp) -> np.ndarray:
    """The 64 bits pol_gauss draws from for (chain seed, generator step, GLOBAL environment index, component), uint64:
    mix(mix(seed ^ step * 0xd1342543de82ef95) ^ (env << 1 | comp)).  `step`, `env` and `comp` broadcast against each other."""
    step, env, comp = (np.asarray(x).astype(np.uint64) for x in (step, env, comp))
    shape = np.broadcast(step, env, comp).shape
    key = _mix(np.uint64(int(seed) & _U64) ^ (np.atleast_1d(step) * np.uint64(_GEN_MUL)))
    return _mix(key ^ ((np.atleast_1d(env) << np.uint64(1)) | np.atleast_1d(comp))).reshape(shape)


def hash_fields(h):
    """(u1, u2), float32, as pol_gauss forms them from the hash: u1 = min(((h >> 40) + 0.5) 2^-24, 1 - 2^-24) in (0, 1), u2 =
    ((h >> 8) & 0xffffff) 2^-24 in [0, 1).  u2 is exact.  u1 is exact below 2^23; from there on field + 0.5 is a tie that float32 rounds
    to even (one rounding, the same on every IEEE machine), which the top field would take to 1: hence the min."""
    h = np.atleast_1d(np.asarray(h).astype(np.uint64))
    scale = np.float32(1.0 / 16777216.0)
    u1 = np.minimum(((h >> np.uint64(40)).astype(np.float32) + np.float32(0.5)) * scale, np.float32(1.0 - 1.0 / 16777216.0))
    u2 = ((h >> np.uint64(8)) & np.uint64(0xffffff)).astype(np.float32) * scale
    return u1.reshape(np.shape(h)), u2.reshape(np.shape(h))


def policy_noise_fields(seed: int, step, env, comp):
    """(u1, u2), float32, of the draw pol_gauss makes: hash_fields(policy_noise_hash(...))."""
    h = policy_noise_hash(seed, step, env, comp)
    u1, u2 = hash_fields(h)
    return u1.reshape(h.shape), u2.reshape(h.shape)


def box_muller(u1, u2, dtype=np.float64):
    """sqrt(-2 ln u1) cos(2 pi u2) in `dtype`, in pol_gauss' order of operations (2 pi rounded to `dtype` first, as the kernel's literal)."""
    u1, u2 = np.asarray(u1).astype(dtype), np.asarray(u2).astype(dtype)
    r = np.sqrt(dtype(-2.0) * _rounded(np.log, u1, dtype))
    return r * _rounded(np.cos, dtype(2.0 * np.pi) * u2, dtype)


def policy_noise(seed: int, step, env, comp, dtype=np.float64):
    """eps of pol_gauss: Box-Muller on policy_noise_fields in `dtype`."""
    return box_muller(*policy_noise_fields(seed, step, env, comp), dtype=dtype)


def sample_reference(mu, log_std, eps, dtype=np.float64):
    """a = mu + exp(log_std) * eps in `dtype` (pol_act_sample); mu, eps [..., 2], log_std [2]."""
    sigma = _rounded(np.exp, np.asarray(log_std).astype(dtype), dtype)
    return np.asarray(mu).astype(dtype) + sigma * np.asarray(eps).astype(dtype)


def logp_reference(a, mu, log_std, dtype=np.float64):
    """log pi(a) of the diagonal Gaussian, the two components summed, in `dtype` and pol_logp's order: z = (a - mu) / exp(ls),
    (-0.5 z) z - ls - log sqrt(2 pi); a, mu [..., 2] -> [...]."""
    ls = np.asarray(log_std).astype(dtype)
    z = (np.asarray(a).astype(dtype) - np.asarray(mu).astype(dtype)) / _rounded(np.exp, ls, dtype)
    lp = dtype(-0.5) * z * z - ls - dtype(0.5 * np.log(2.0 * np.pi))
    return lp[..., 0] + lp[..., 1]


def action_map_reference(a, mid, half, lo, hi):
    """mid + half * clamp(a, lo, hi) per component in float32 (PolActMap): what an act launch leaves in the environment's action buffer."""
    f = np.float32
    mid, half, lo, hi = (np.asarray(x, dtype=f) for x in (mid, half, lo, hi))
    return mid + half * np.minimum(np.maximum(np.asarray(a, dtype=f), lo), hi)


def squash_map_reference(u, mid, half, dtype=np.float64):
    """mid + half * tanh(u) per component in `dtype`, as PolSquashMap forms it: t = exp(-2 |u|), tanh = copysign((1 - t) / (1 + t), u) --
    odd bit for bit, exactly +-1 once t drops below half an ulp of 1, never NaN for a finite u.  mid and half are rounded to float32
    first: the launch takes them as floats.  float64: the reference the tests hold actions_out to; float32: the kernel's own operations."""
    u = np.asarray(u).astype(dtype)
    mid, half = (np.asarray(x, dtype=np.float32).astype(dtype) for x in (mid, half))
    t = _rounded(np.exp, dtype(-2.0) * np.abs(u), dtype)
    return mid + half * np.copysign((dtype(1.0) - t) / (dtype(1.0) + t), u)


def gae_reference(R, V, Dn, last_v, gamma: float, lam: float, dtype=np.float64):
    """(adv, ret) [T, N] of k6_gae's backward recursion in `dtype` and in its order: delta = R + (gamma nv) (1 - Dn) - V,
    adv = delta + ((gamma lam) (1 - Dn)) adv', ret = adv + V.  gamma and lam are rounded to float32 first: the kernel takes them as
    float, and the caller's rounding is not the kernel's error."""
    R, V, Dn = (np.asarray(x).astype(dtype) for x in (R, V, Dn))
    g, l = dtype(np.float32(gamma)), dtype(np.float32(lam))
    nv, gae = np.asarray(last_v).astype(dtype), np.zeros(R.shape[1], dtype=dtype)
    adv = np.empty_like(R)
    for t in range(R.shape[0] - 1, -1, -1):
        nd = dtype(1.0) - Dn[t]
        delta = R[t] + g * nv * nd - V[t]
        gae = delta + g * l * nd * gae
        adv[t] = gae
        nv = V[t]
    return adv, adv + V


def policy_param_floats(obs_dim: int, hidden=HIDDEN) -> int:
    """Floats of the packed buffer (auv_policy_io::params) of a net with `hidden` widths on `obs_dim` input columns."""
    hidden = check_hidden(hidden, "policy_param_floats")
    if hidden == HIDDEN:
        return int(_LIB.auv_policy_param_floats(int(obs_dim)))
    return int(_LIB.auv_policy_param_floats_arch(int(obs_dim), C.byref(_arch_arg(hidden))))


def pack_linear(weight: torch.Tensor, out_pad: int, in_pad: int) -> torch.Tensor:
    """A Linear.weight [out, in] zero-padded to [out_pad, in_pad] (multiples of 16 / 32) and laid out in MFMA fragment order
    (include/auv_hip.h, auv_policy_io): [n-tile][k-step J][half h][group g][row n][4 floats] -- lane 16 g + n of a wave holds
    k = 32 J + 8 g + 4 h + (0..3) of row n of the tile, and each load instruction of the kernel reads 1 KB contiguously."""
    w = torch.zeros((out_pad, in_pad), dtype=torch.float32, device=weight.device)
    w[:weight.shape[0], :weight.shape[1]].copy_(weight)
    return w.view(out_pad // 16, 16, in_pad // 32, 4, 2, 4).permute(0, 2, 4, 3, 1, 5).contiguous().view(-1)


def pack_linear_bf16(weight: torch.Tensor, out_pad: int, in_pad: int) -> torch.Tensor:
    """The same matrix as bf16 fragments for v_mfma_f32_16x16x32_bf16 (auv_policy_io::params_bf16): [n-tile][k-step J][group g]
    [row n][8 bf16] -- lane 16 g + n holds k = 32 J + 8 g + (0..7) of row n, 16 bytes."""
    w = torch.zeros((out_pad, in_pad), dtype=torch.float32, device=weight.device)
    w[:weight.shape[0], :weight.shape[1]].copy_(weight)
    return w.view(out_pad // 16, 16, in_pad // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous().view(-1).to(torch.bfloat16)


@torch.no_grad()
def pack_policy_params(net: nn.Module, obs_dim: int, out: Optional[torch.Tensor] = None, hidden=HIDDEN) -> torch.Tensor:
    """The packed f32 weight buffer of auv_policy_io::params for `net` (net.pi / net.v: Linear-Tanh x 3 + Linear, net.log_std) without
    an environment: what FusedActorCritic.refresh() writes into `self.params`.  For policy_eval on rows that come from elsewhere.
    `hidden`: the hidden widths of both nets, one of SUPPORTED_HIDDEN."""
    hidden = check_hidden(hidden, "pack_policy_params")
    k0p = _pad16(int(obs_dim))
    dev = net.log_std.device
    n_float = policy_param_floats(obs_dim, hidden)
    p = torch.zeros(n_float, dtype=torch.float32, device=dev) if out is None else out
    off = 0
    for seq, n_out in ((net.pi, 2), (net.v, 1)):
        lin = [m for m in seq if isinstance(m, nn.Linear)]
        if tuple(l.out_features for l in lin[:-1]) != hidden or lin[-1].out_features != n_out or lin[0].in_features != int(obs_dim):
            raise ValueError("pack_policy_params: the fused kernels evaluate obs[%d] -> %s tanh -> %d" % (int(obs_dim), list(hidden), n_out))
        for j, l in enumerate(lin):
            out_p = l.out_features if j < 3 else 16
            in_p = k0p if j == 0 else l.in_features
            p[off:off + out_p * in_p].copy_(pack_linear(l.weight, out_p, in_p))
            off += out_p * in_p
            p[off:off + out_p].zero_()
            p[off:off + l.out_features].copy_(l.bias)
            off += out_p
    p[off:off + 2].copy_(net.log_std)
    assert off + 4 == p.numel()
    return p


_EVAL_OUTPUTS = ("mu", "action", "value", "logp")


def _eval_check(name: str, t, device, shape_tail, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != device:
        raise ValueError("policy_eval: %s must be a %s tensor on %s" % (name, str(dtype).replace("torch.", ""), device))
    if t.dim() != 1 + len(shape_tail) or tuple(t.shape[1:]) != tuple(shape_tail):
        raise ValueError("policy_eval: %s must have shape [M%s], got %s" % (name, "".join(", %d" % x for x in shape_tail), tuple(t.shape)))


def policy_eval(params: torch.Tensor, obs_dim: int, X: torch.Tensor, idx: Optional[torch.Tensor] = None,
                actions: Optional[torch.Tensor] = None, want: Sequence[str] = ("mu", "value"), action_map=None,
                out: Optional[Dict[str, torch.Tensor]] = None, hidden=HIDDEN, arch_entry: Optional[bool] = None,
                squash: bool = False) -> Dict[str, torch.Tensor]:
    """auv_policy_eval (csrc/k9_policy_eval.hip) on the caller's current stream: M observation rows through the policy net, the
    value net, or both, in ONE launch -- no environment, no rollout position, no sampling.

    params      a packed weight buffer (FusedActorCritic.params, or the buffer a FusedPPOUpdate is attached to)
    X           [R, obs_dim] float32; rows may be strided (a column window of a wider buffer), columns may not
    idx         [M] int64 rows of X to evaluate, repeats allowed (None: all R rows, M = R); an index outside [0, R) is the
                caller's error: it is not checked (as auv_ppo_batch::idx)
    actions     [M, 2] float32, contiguous: needed for "logp"
    want        any of "mu" [M, 2], "action" [M, 2], "value" [M], "logp" [M]; only the nets they need are launched
    action_map  (act_mid, act_half, clip_lo, clip_hi), each two floats: action = mid + half * clip(mu, lo, hi); None: the identity
                map without clipping
    out         tensors to write into instead of new ones, by name; "action" may be a row-strided [M, 2] view (rows of an
                environment's action buffer)
    hidden      the hidden widths `params` was packed for, one of SUPPORTED_HIDDEN
    arch_entry  None: the default widths go through auv_policy_eval, any other through auv_policy_eval_arch; True: the _arch entry also
                for the default widths (it dispatches to the same kernel)
    squash      True: auv_policy_eval_squash -- action = mid + half * tanh(mu), lo and hi are not read; mu, value and logp are the same
                either way, and `actions` are PRE-SQUASH actions (rows of a rollout's A)
    Returns a dict of the tensors asked for.  Raises ValueError for anything the launch would refuse."""
    want = tuple(want)
    out = dict(out or {})
    hidden = check_hidden(hidden, "policy_eval")
    n_params = policy_param_floats(obs_dim, hidden) if int(obs_dim) >= 1 else 0
    for w in want:
        if w not in _EVAL_OUTPUTS:
            raise ValueError("policy_eval: unknown output %r (one of %s)" % (w, ", ".join(_EVAL_OUTPUTS)))
    for w in out:
        if w not in want:
            raise ValueError("policy_eval: out[%r] given but %r is not in want" % (w, w))
    if not want:
        raise ValueError("policy_eval: no output asked for")
    obs_dim = int(obs_dim)
    if obs_dim < 1:
        raise ValueError("policy_eval: obs_dim must be >= 1")
    if not isinstance(params, torch.Tensor) or params.dtype != torch.float32 or not params.is_cuda or not params.is_contiguous() \
            or params.numel() != n_params or params.data_ptr() % 16:
        raise ValueError("policy_eval: params must be a contiguous, 16-byte aligned float32 device tensor of auv_policy_param_floats(%d) = %d "
                         "elements%s" % (obs_dim, n_params, "" if hidden == HIDDEN else " (hidden widths %s)" % list(hidden)))
    dev = params.device
    _eval_check("X", X, dev, (obs_dim,))
    if X.stride(1) != 1 and X.shape[0] > 0:
        raise ValueError("policy_eval: the columns of X must be contiguous (rows may be strided)")
    ldx = int(X.stride(0)) if X.shape[0] > 1 else obs_dim
    if ldx < obs_dim:
        raise ValueError("policy_eval: row stride of X %d < obs_dim %d" % (ldx, obs_dim))
    if idx is not None:
        _eval_check("idx", idx, dev, (), torch.int64)
        if not idx.is_contiguous():
            raise ValueError("policy_eval: idx must be contiguous")
        if idx.numel() and X.shape[0] == 0:
            raise ValueError("policy_eval: idx names rows of an empty X")
    M = int(X.shape[0] if idx is None else idx.numel())
    if "logp" in want and actions is None:
        raise ValueError("policy_eval: logp needs the actions")
    if actions is not None:
        _eval_check("actions", actions, dev, (2,))
        if actions.shape[0] != M or not actions.is_contiguous():
            raise ValueError("policy_eval: actions must be a contiguous [%d, 2] tensor" % M)
    ev = _capi.AuvPolicyEval()
    res = {}
    with torch.cuda.device(dev):
        for w in want:
            tail = (2,) if w in ("mu", "action") else ()
            t = out.get(w)
            if t is None:
                t = torch.empty((M,) + tail, dtype=torch.float32, device=dev)
            else:
                _eval_check("out[%r]" % w, t, dev, tail)
                if t.shape[0] != M:
                    raise ValueError("policy_eval: out[%r] has %d rows, M = %d" % (w, t.shape[0], M))
                if w == "action":
                    if M > 0 and (t.stride(1) != 1 or (M > 1 and t.stride(0) < 2)):
                        raise ValueError("policy_eval: out['action'] must have contiguous columns and a row stride >= 2")
                elif not t.is_contiguous():
                    raise ValueError("policy_eval: out[%r] must be contiguous" % w)
            res[w] = t
            setattr(ev, w, t.data_ptr() if M else None)
        if M == 0:
            return res
        ev.params, ev.X, ev.ldx = params.data_ptr(), X.data_ptr(), ldx
        ev.idx = idx.data_ptr() if idx is not None else None
        ev.A = actions.data_ptr() if actions is not None else None
        ev.action_ld = int(res["action"].stride(0)) if "action" in res and M > 1 else 2
        ev.obs_dim, ev.M = obs_dim, M
        mid, half, lo, hi = ((0.0, 0.0), (1.0, 1.0), (float("-inf"),) * 2, (float("inf"),) * 2) if action_map is None else action_map
        for k in range(2):
            ev.act_mid[k], ev.act_half[k], ev.clip_lo[k], ev.clip_hi[k] = float(mid[k]), float(half[k]), float(lo[k]), float(hi[k])
        st = torch.cuda.current_stream(dev)
        dev_i = dev.index if dev.index is not None else torch.cuda.current_device()
        name = "auv_policy_eval_squash" if squash else "auv_policy_eval"
        if hidden != HIDDEN or arch_entry:
            _check(getattr(_LIB, name + "_arch")(dev_i, C.byref(ev), C.byref(_arch_arg(hidden)), C.c_void_p(st.cuda_stream)), name + "_arch")
        else:
            _check(getattr(_LIB, name)(dev_i, C.byref(ev), C.c_void_p(st.cuda_stream)), name)
    return res


class FusedActorCritic:
    def __init__(self, net: nn.Module, env: BatchedAuvEnv, rollout: int, reward_scale: float = 1.0, reward_clip: float = 0.0,
                 act_mid=None, act_half=None, clip_lo=None, clip_hi=None, seed: int = 0, store_obs: bool = True, debug: bool = False,
                 bf16: bool = False, frames: int = 1, arch_entry: Optional[bool] = None, normalize=None, squash: bool = False):
        # squash: the environment receives act_mid + act_half * tanh(u) (module docstring); the plain, exact-f32 launches only
        self.squash = bool(squash)
        if self.squash:
            for bad, what in ((int(frames) > 1, "frames = %d" % int(frames)), (normalize is not None, "normalize"), (bool(bf16), "bf16 = True")):
                if bad:
                    raise ValueError("FusedActorCritic: squash = True together with %s -- the stacked, normalising and bf16 launches have no "
                                     "squashed variant" % what)
        self.net, self.env, self.T = net, env, int(rollout)
        self.device = env.device
        # frames > 1: every environment is evaluated on its last `frames` observations (module docstring); 1: the plain launch
        self.frames = int(frames)
        if self.frames < 1 or self.frames > _capi.MAX_FRAMES:
            raise ValueError("FusedActorCritic: frames = %d outside [1, %d]" % (self.frames, _capi.MAX_FRAMES))
        if self.frames > 1 and bf16:
            raise ValueError("FusedActorCritic: frames = %d with bf16 = True -- stacked rows are evaluated in exact f32 only" % self.frames)
        # normalize: a RunningNorm (gym_auv_amd/normalize.py); None: the plain launches, nothing below touches them
        self.normalize = normalize
        if normalize is not None:
            if self.frames > 1:
                raise ValueError("FusedActorCritic: frames = %d together with normalize -- frame stacking and normalisation are not combined" % self.frames)
            if bf16:
                raise ValueError("FusedActorCritic: bf16 = True together with normalize -- normalised rows are evaluated in exact f32 only")
            if normalize.obs_dim != env.obs_dim:
                raise ValueError("FusedActorCritic: normalize was made for %d columns, the environment's observation has %d"
                                 % (normalize.obs_dim, env.obs_dim))
        self.in_dim = self.frames * env.obs_dim                                        # the nets' input width
        self._lin = []
        # the hidden widths are read off the modules: both nets the same triple, one of SUPPORTED_HIDDEN
        self.hidden = None
        for seq, out in ((net.pi, 2), (net.v, 1)):
            lin = [m for m in seq if isinstance(m, nn.Linear)]
            act = [m for m in seq if not isinstance(m, nn.Linear)]
            dims = tuple(l.out_features for l in lin[:-1])
            if lin and lin[0].in_features != self.in_dim:                              # the width, with both numbers (one frame or several)
                raise ValueError("FusedActorCritic: frames = %d of %d columns need a first Linear with in_features == %d, got %d"
                                 % (self.frames, env.obs_dim, self.in_dim, lin[0].in_features))
            if dims not in SUPPORTED_HIDDEN or lin[-1].out_features != out or not all(isinstance(a, nn.Tanh) for a in act):
                raise ValueError("FusedActorCritic evaluates obs -> [h1, h2, h3] tanh -> %d with three hidden layers (another depth is not "
                                 "compiled in) and [h1, h2, h3] one of %s (the reference's architecture, scripts/run.py:332-357, is the "
                                 "first); got %s -> %d" % (out, list(SUPPORTED_HIDDEN), list(dims), lin[-1].out_features))
            if self.hidden is not None and dims != self.hidden:
                raise ValueError("FusedActorCritic: net.pi has the hidden widths %s, net.v %s -- one launch evaluates both nets with the same "
                                 "widths, one of %s" % (list(self.hidden), list(dims), list(SUPPORTED_HIDDEN)))
            self.hidden = dims
            self._lin.append(lin)
        if bf16 and self.hidden != HIDDEN:
            raise ValueError("FusedActorCritic: hidden widths %s with bf16 = True -- only %s has a bf16 path, the other widths are evaluated "
                             "in exact f32 only" % (list(self.hidden), list(HIDDEN)))
        # the default widths go through the entries without _arch (unless arch_entry: the _arch entries then dispatch to the same kernels)
        self._arch = _arch_arg(self.hidden) if (self.hidden != HIDDEN or arch_entry) else None
        self.k0p = _pad16(self.in_dim)
        n_float = policy_param_floats(self.in_dim, self.hidden)
        self.params = torch.zeros(n_float, dtype=torch.float32, device=self.device)
        assert self.params.data_ptr() % 16 == 0
        # bf16 = True: the weights also as bf16 fragments, and the launch multiplies on v_mfma_f32_16x16x32_bf16 (one MFMA where
        # the exact path issues eight; ~1e-2 on the means -- NOT the reference's arithmetic; default off)
        self.bf16 = bool(bf16)
        n_w = (n_float - 4) // 2 - (sum(self.hidden) + 16)                                  # weight elements of one net
        self.params_bf16 = torch.zeros(2 * n_w, dtype=torch.bfloat16, device=self.device) if self.bf16 else None
        if env._slices is None:
            env.set_sub_batches(1)
        self.slices = list(env._slices)
        D = env.obs_dim
        lo_t = torch.as_tensor(env.action_space.low, dtype=torch.float32)
        hi_t = torch.as_tensor(env.action_space.high, dtype=torch.float32)
        # default: raw units clipped to the action space (what stable-baselines does with a Box)
        mid = [0.0, 0.0] if act_mid is None else [float(x) for x in act_mid]
        half = [1.0, 1.0] if act_half is None else [float(x) for x in act_half]
        clo = lo_t.tolist() if clip_lo is None else [float(x) for x in clip_lo]
        chi = hi_t.tolist() if clip_hi is None else [float(x) for x in clip_hi]
        self.actions = torch.zeros((env.n_envs, 2), dtype=torch.float32, device=self.device)
        self.action_map = (tuple(mid), tuple(half), tuple(clo), tuple(chi))            # (what predict() maps the mean through, too)
        N = env.n_envs
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=self.device)   # noqa: E731
        # ONE set of rollout buffers [T, N, ...] for the whole batch: every chain writes its own columns, nothing is
        # concatenated afterwards
        self.O = z(self.T, N, self.in_dim) if store_obs else None
        self.A, self.LP, self.V, self.R, self.Dn = z(self.T, N, 2), z(self.T, N), z(self.T, N), z(self.T, N), z(self.T, N)
        self.mu = z(N, 2) if debug else None
        self.eps = z(N, 2) if debug else None
        self.buf: List[dict] = []
        self._ios = (_capi.AuvPolicyIO * len(self.slices))()
        for i, (lo, cnt) in enumerate(self.slices):
            b = dict(ctr=torch.zeros(4, dtype=torch.int64, device=self.device))
            self.buf.append(b)
            io = self._ios[i]
            io.obs, io.params, io.ctr = env.obs.data_ptr(), self.params.data_ptr(), b["ctr"].data_ptr()
            io.reward_in, io.done_in, io.actions_out = env.reward.data_ptr(), env.done.data_ptr(), self.actions.data_ptr()
            io.O = self.O.data_ptr() if store_obs else None
            io.A, io.LP, io.V, io.R, io.Dn = (x.data_ptr() for x in (self.A, self.LP, self.V, self.R, self.Dn))
            io.mu_out = self.mu[lo:].data_ptr() if debug else None       # ([ne][2] views of the slice's rows)
            io.eps_out = self.eps[lo:].data_ptr() if debug else None
            io.seed = chain_seed(seed, i)
            io.obs_dim, io.T, io.ld, io.env_base = D, self.T, N, 0
            io.params_bf16 = self.params_bf16.data_ptr() if self.bf16 else None
            for k in range(2):
                io.act_mid[k], io.act_half[k], io.clip_lo[k], io.clip_hi[k] = mid[k], half[k], clo[k], chi[k]
            io.reward_scale, io.reward_clip = float(reward_scale), float(reward_clip)
        # host mirror of every chain's rollout position and generator step (the device copies in `ctr` stay in step with them):
        # rollout() names them to the launches, which then need no count-off
        self._t = [0] * len(self.slices)
        self._g = [0] * len(self.slices)
        self.stack = None
        if self.frames > 1:
            # the history of every environment (indexed by global environment: the chains advance their own rows) and the launches'
            # io blocks: the plain ones with hist, stk and frames behind them
            from .framestack import FrameStack
            self.stack = FrameStack(env, self.frames)
            self._sios = (_capi.AuvPolicyStack * len(self.slices))()
            for i in range(len(self.slices)):
                s = self._sios[i]
                s.io = self._ios[i]
                s.hist, s.stk, s.frames = self.stack.hist.data_ptr(), self.stack.stk.data_ptr(), self.frames
        self._nios = None
        if normalize is not None:
            normalize.bind(N, self.T, self.slices, self.device)
            if normalize.norm_obs:
                # the launches' io blocks: the plain ones with the table and the partial buffers behind them
                self._nios = (_capi.AuvPolicyNorm * len(self.slices))()
                for i in range(len(self.slices)):
                    s = self._nios[i]
                    s.io = self._ios[i]
                    s.table, s.part, s.pcnt = normalize.table.data_ptr(), normalize.part.data_ptr(), normalize.pcnt.data_ptr()
                    s.part_ld, s.part_base, s.clip_obs = normalize.part_ld, normalize.part_base[i], normalize.clip_obs
        # the entries act() and rollout() call, resolved once: squash first, then norm, then stacked, then plain; the _arch entries
        # (with the widths as one more argument behind the io block) only for other widths than the default, or on request
        variant, self._io = (("_squash", self._ios) if self.squash else ("_norm", self._nios) if self._nios is not None
                             else ("_stacked", self._sios) if self.frames > 1 else ("", self._ios))
        suffix = variant + ("_arch" if self._arch is not None else "")
        self._act_name, self._rollout_name = "auv_policy_act" + suffix, "auv_policy_rollout" + suffix
        self._act_fn, self._rollout_fn = getattr(_LIB, self._act_name), getattr(_LIB, self._rollout_name)
        self._arch_arg = () if self._arch is None else (C.byref(self._arch),)
        self.refresh()

    # ------------------------------------------------------------------------------ weights
    @torch.no_grad()
    def refresh(self):
        """Repack the modules' weights into the kernel's layout (rows padded to a multiple of 16 columns, the last layer to 16
        rows): device-side copies on the current stream, no host synchronisation.  Call after every optimiser step that
        precedes a rollout."""
        off = off16 = 0
        p = self.params
        for lin in self._lin:
            for j, l in enumerate(lin):
                out_p = l.out_features if j < 3 else 16
                in_p = self.k0p if j == 0 else l.in_features
                p[off:off + out_p * in_p].copy_(pack_linear(l.weight, out_p, in_p))
                if self.bf16:
                    self.params_bf16[off16:off16 + out_p * in_p].copy_(pack_linear_bf16(l.weight, out_p, in_p))
                    off16 += out_p * in_p
                off += out_p * in_p
                p[off:off + l.out_features].copy_(l.bias)
                off += out_p
        p[off:off + 2].copy_(self.net.log_std)
        assert off + 4 == p.numel()

    # ------------------------------------------------------------------------------ rollouts
    def begin_rollout(self):
        """t = 0 on every chain (enqueued on each chain's stream, behind whatever the chain did last)."""
        for i, b in enumerate(self.buf):
            with torch.cuda.stream(self.env._sub_streams[i]):
                b["ctr"][0] = 0
            self._t[i] = 0

    def act(self, i: int, stream: Optional[torch.cuda.Stream] = None):
        """The policy launch of sub-batch i alone (auv_policy_act) on `stream` (default: the sub-batch's): writes the
        slice's rows of `self.actions` and the transition at the chain's position t, then moves t on."""
        lo, cnt = self.slices[i]
        st = self.env._sub_streams[i] if stream is None else stream
        _check(self._act_fn(self.env._h, lo, cnt, C.byref(self._io[i]), *self._arch_arg, C.c_void_p(st.cuda_stream)), self._act_name)
        self._t[i] = min(self._t[i] + 1, self.T + 1)
        self._g[i] += 1

    def rollout(self, n_steps: int, flush: bool = True):
        """`n_steps` transitions of every sub-batch: per step and chain the policy launch and the environment's step of that
        slice, back to back on the chain's stream -- one C call (auv_policy_rollout), nothing returns to Python in between.
        `flush`: a final policy call stores reward / done of the last step.  The chains are not ordered against the caller's
        stream: order them yourself (wait_stream) around the call."""
        env = self.env
        k = len(self.slices)
        t0, g0 = (C.c_int64 * k)(*self._t), (C.c_int64 * k)(*self._g)
        _check(self._rollout_fn(env._h, env.sub_batches, env._bounds_c, env._streams_c, self._io, *self._arch_arg,
                                C.c_void_p(env.obs.data_ptr()), C.c_void_p(env.reward.data_ptr()), C.c_void_p(env.done.data_ptr()),
                                int(n_steps), int(bool(flush)), t0, g0), self._rollout_name)
        n_launch = int(n_steps) + int(bool(flush))
        for i in range(k):
            self._t[i] = min(self._t[i] + n_launch, self.T + 1)
            self._g[i] += n_launch

    def buffers(self):
        """(O, A, LP, V, R, Dn) of the whole batch, [T, N, ...] (written in place by the chains: no copy).  With frames > 1 O holds the
        stacked rows, [T, N, frames * obs_dim]."""
        return self.O, self.A, self.LP, self.V, self.R, self.Dn

    def gae(self, V: torch.Tensor, last_v: torch.Tensor, gamma: float, lam: float):
        """Generalised advantage estimation of the stored rollout (auv_gae, one launch on the current stream): returns
        (adv, ret), [T, N].  `V` [T, N] and `last_v` [N] in the units of the stored rewards (pass `self.V` or a rescaled copy)."""
        adv, ret = torch.empty_like(self.R), torch.empty_like(self.R)
        V, last_v = V.contiguous(), last_v.contiguous()
        st = torch.cuda.current_stream(self.device)
        _check(_LIB.auv_gae(self.env._h, C.c_void_p(self.R.data_ptr()), C.c_void_p(V.data_ptr()), C.c_void_p(self.Dn.data_ptr()),
                            C.c_void_p(last_v.data_ptr()), float(gamma), float(lam), C.c_void_p(adv.data_ptr()),
                            C.c_void_p(ret.data_ptr()), self.T, self.env.n_envs, C.c_void_p(st.cuda_stream)), "auv_gae")
        return adv, ret

    # ------------------------------------------------------------------------------ evaluation outside a rollout
    def _eval_kw(self):
        return dict(hidden=self.hidden, arch_entry=self._arch is not None, squash=self.squash)

    def _rows(self, obs):
        if obs is None and self.frames > 1:
            # the row the next policy launch would form: a peek, the history is not moved on
            return self.stack.peek(self.env.obs, self.env.done)
        X = self.env.obs if obs is None else obs
        if self._nios is not None:
            # raw rows -> the rows the normalising launch would feed the nets (auv_norm_rows, the current table)
            return self.normalize.normalize(X)
        return X

    def reset_frames(self, envs: Optional[torch.Tensor] = None):
        """Empty the history of the environments `envs` (indices or a boolean mask; None: all) on the current stream: their next row
        holds the current observation and zeros.  Call it behind env.reset() -- an episode that ends inside a rollout resets its history
        itself, through the done flag.  Nothing to do with frames == 1."""
        if self.stack is not None:
            self.stack.reset(envs)

    def predict(self, obs: Optional[torch.Tensor] = None, deterministic: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The deterministic action of the policy -- the reference's agent.predict(obs, deterministic=True) of its enjoy / play /
        test modes (scripts/run.py:175, 273, 567): act_mid + act_half * clip(mu(obs)) (squash: act_mid + act_half * tanh(mu(obs))), one launch (auv_policy_eval) on the caller's
        current stream, written into `out` (default: `self.actions`, which env.step takes as is).  obs = None: the environment's
        observation buffer (with frames > 1: the stacked row of it, peeked; rows passed in are stacked rows already).  Reads `self.params`: refresh() after optimiser steps, as for rollouts.  Touches no rollout buffer and
        no counter."""
        if not deterministic:
            raise ValueError("predict(deterministic=False): sampling lives where its counters are -- use act(i) / rollout()")
        X = self._rows(obs)
        if out is None:
            if X.dim() != 2 or X.shape[0] != self.env.n_envs:
                raise ValueError("predict: %s rows do not fit self.actions [%d, 2]; pass out=" % (tuple(X.shape[:1]), self.env.n_envs))
            out = self.actions
        return policy_eval(self.params, self.in_dim, X, want=("action",), action_map=self.action_map, out={"action": out}, **self._eval_kw())["action"]

    def value(self, obs: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The critic's value of every row of `obs` (None: the environment's observation buffer), [M] float32 in the units the
        critic was trained in (scaled rewards): one launch of the value net alone, on the caller's current stream."""
        return policy_eval(self.params, self.in_dim, self._rows(obs), want=("value",), **self._eval_kw())["value"]

    def evaluate(self, obs: torch.Tensor, actions: torch.Tensor):
        """(log pi(actions | obs) [M], value [M], mu [M, 2]) in one launch on the caller's current stream.  With `normalize`, obs are RAW
        rows (the rows stored in O are normalised already: evaluate those with policy_eval).  With `squash`, `actions` are PRE-SQUASH actions:
        rows of A, not what the environment received."""
        r = policy_eval(self.params, self.in_dim, self._rows(obs), actions=actions, want=("logp", "value", "mu"), **self._eval_kw())
        return r["logp"], r["value"], r["mu"]
