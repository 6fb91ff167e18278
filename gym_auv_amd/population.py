"""PolicyPopulation -- a policy per group of environments in ONE launch, made and folded back on the device (csrc/k11_population.hip).

Every other rollout path of the package evaluates one parameter block for the whole batch.  Here row j of the batch is evaluated with
the weights of member j // G: 4096 environments are 256 tiles of 16 rows, and with G = 16 that is a population of 256 MLP policies
-- the reference's own actor, obs -> [256, 128, 64] tanh -> 2 (scripts/run.py:332-357) -- stepping side by side.  What evolution
strategies, ARS on that actor or "evaluate these checkpoints side by side" need:

    pop = PolicyPopulation(env, members=256, net=net, seed=1)      # theta = net.pi, packed; G = env.n_envs // 256
    for g in range(generations):
        pop.perturb(sigma, g)                                      # theta_p = theta +- sigma eps_p   (mirrored pairs, on the device)
        fitness, ends = pop.rollout(T)                             # T x (population launch + env step), one C call
        pop.update(pop.centered_ranks(fitness), lr, sigma, g)      # ES gradient estimate, eps regenerated from its counters
    pop.base_state_into(fused)                                     # theta into a FusedActorCritic's policy half: predict(), evaluate.py

The NumPy functions below -- es_noise, padding_mask, perturb_reference, es_update_reference -- are the CONTRACT of the two kernels that
make and fold a population: the kernels are held to them bit for bit (tests/test_gpu_population.py).  They need no device.

Hidden widths: the reference's [256, 128, 64] unless named -- `hidden=` on the functions, read off the net by PolicyPopulation -- and
then one of the triples the fused policy launches are compiled for (_capi.POLICY_ARCHS; the auv_population_*_arch entries,
csrc/k14_population_arch.hip; tests/test_gpu_population_arch.py).
"""
import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np

HIDDEN = (256, 128, 64)
_GEN_MUL = 0xd1342543de82ef95
_U64 = 0xFFFFFFFFFFFFFFFF
# eps = (S - 131070) * c, S the sum of four uniform 16-bit fields: variance of S = 4 (65536^2 - 1) / 12
EPS_SCALE = np.float32(1.0 / np.sqrt(4.0 * (65536.0 * 65536.0 - 1.0) / 12.0))


def _hidden(hidden, who: str) -> tuple:
    """`hidden` as a tuple of three ints, one of the triples the population kernels are compiled for (_capi.POLICY_ARCHS; the list of
    the fused policy launches); ValueError otherwise.  Needs no device and no library."""
    from ._capi import POLICY_ARCHS
    try:
        h = tuple(int(x) for x in hidden)
    except (TypeError, ValueError):
        h = None
    if h is None or h not in POLICY_ARCHS:
        raise ValueError("%s: hidden widths %r are not compiled in: the population kernels evaluate one of %s" % (who, hidden, list(POLICY_ARCHS)))
    return h


def member_floats(obs_dim: int, hidden=HIDDEN) -> int:
    """Floats of one member: the packed policy net of auv_policy_io::params (auv_population_member_floats, _arch for other `hidden`
    widths than the reference's)."""
    h1, h2, h3 = _hidden(hidden, "member_floats")
    k0p = (int(obs_dim) + 31) & ~31
    n = h1 * k0p + h1 + h2 * h1 + h2 + h3 * h2 + h3 + 16 * h3 + 16
    return (n + 3) & ~3


# ------------------------------------------------------------------------------------------------------------------ the contract
def _mix(z: np.ndarray) -> np.ndarray:
    """splitmix64 finaliser (csrc/auv_noise.h: pol_mix) on uint64 arrays: 64-bit wrap-around arithmetic."""
    z = z + np.uint64(0x9e3779b97f4a7c15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def es_noise(seed: int, generation: int, pair, idx) -> np.ndarray:
    """eps(seed, generation, pair, idx), float32: h = mix(mix(mix(seed ^ generation * 0xd1342543de82ef95) ^ pair) ^ idx), S = the sum
    of the four 16-bit fields of h, eps = float32(S - 131070) * EPS_SCALE -- one rounded product (|S - 131070| < 2^24 converts
    exactly).  Symmetric, unit variance, |eps| <= 3.4642.  `pair` and `idx` broadcast against each other."""
    key0 = np.array([(int(seed) ^ ((int(generation) * _GEN_MUL) & _U64)) & _U64], dtype=np.uint64)
    pair = np.atleast_1d(np.asarray(pair)).astype(np.uint64)
    idx = np.atleast_1d(np.asarray(idx)).astype(np.uint64)
    h = _mix(_mix(_mix(key0) ^ pair) ^ idx)
    m = np.uint64(0xffff)
    S = (h & m) + ((h >> np.uint64(16)) & m) + ((h >> np.uint64(32)) & m) + (h >> np.uint64(48))
    return (S.astype(np.int64) - 131070).astype(np.float32) * EPS_SCALE


def padding_mask(obs_dim: int, hidden=HIDDEN) -> np.ndarray:
    """[member_floats(obs_dim, hidden)] bool: True where an element of the packed block is PADDING -- a column of W1 beyond obs_dim, a
    row 2..15 of W4, an entry 2..15 of b4, the tail -- and so carries no noise and no gradient.  Found by packing all-ones weights with
    the packing routine itself (policy.pack_linear), not from a second copy of the index formula."""
    import torch
    from .policy import pack_linear
    h1, h2, h3 = _hidden(hidden, "padding_mask")
    obs_dim = int(obs_dim)
    if obs_dim < 1:
        raise ValueError("padding_mask: obs_dim must be >= 1")
    k0p = (obs_dim + 31) & ~31
    parts = []
    for n_in, n_out, in_p, out_p in ((obs_dim, h1, k0p, h1), (h1, h2, h1, h2), (h2, h3, h2, h3), (h3, 2, h3, 16)):
        parts.append(pack_linear(torch.ones((n_out, n_in)), out_p, in_p).numpy())
        b = np.zeros(out_p, dtype=np.float32)
        b[:n_out] = 1.0
        parts.append(b)
    live = np.concatenate(parts)
    mask = np.ones(member_floats(obs_dim, hidden), dtype=bool)
    mask[:live.size] = live == 0.0
    return mask


def perturb_reference(theta: np.ndarray, P: int, obs_dim: int, sigma: float, seed: int, generation: int, stride: Optional[int] = None,
                      hidden=HIDDEN) -> np.ndarray:
    """What auv_population_perturb writes, [P, stride] float32: member p = theta + s_p * (sigma * eps(seed, generation, p // 2, i)),
    s_p = +1 for even p and -1 for odd p, two rounded float32 operations; padding keeps theta's value, the tail behind the block is 0.
    `hidden`: the widths of the packed net (they decide what is padding; the noise does not depend on them)."""
    nf = member_floats(obs_dim, hidden)
    stride = nf if stride is None else int(stride)
    theta = np.asarray(theta, dtype=np.float32)
    assert theta.shape == (nf,) and stride >= nf
    live = ~padding_mask(obs_dim, hidden)
    idx = np.arange(nf, dtype=np.uint64)
    out = np.zeros((int(P), stride), dtype=np.float32)
    for p in range(int(P)):
        d = np.float32(sigma) * es_noise(seed, generation, p // 2, idx)
        m = theta + (-d if p & 1 else d)
        out[p, :nf] = np.where(live, m, theta)
    return out


def es_update_reference(theta: np.ndarray, w: np.ndarray, obs_dim: int, sigma: float, lr: float, seed: int, generation: int, hidden=HIDDEN):
    """What auv_population_update writes, (grad, theta_new): grad[i] = acc_i * float32(1 / (P sigma)), acc_i the float32 sum over pairs
    in increasing order of (w[2 pair] - w[2 pair + 1]) * eps(seed, generation, pair, i) -- a rounded difference, a rounded product and
    a rounded add per pair; padding gets exactly 0.  theta_new = theta + lr * grad (two rounded operations) where lr != 0.
    `hidden`: the widths of the packed net, as in perturb_reference."""
    nf = member_floats(obs_dim, hidden)
    theta = np.asarray(theta, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32)
    P = int(w.size)
    assert theta.shape == (nf,) and P >= 2 and P % 2 == 0
    live = ~padding_mask(obs_dim, hidden)
    idx = np.arange(nf, dtype=np.uint64)
    acc = np.zeros(nf, dtype=np.float32)
    for pair in range(P // 2):
        d = np.float32(w[2 * pair] - w[2 * pair + 1])
        acc = acc + d * es_noise(seed, generation, pair, idx)
    scale = np.float32(1.0 / (float(P) * float(np.float32(sigma))))
    grad = np.where(live, acc * scale, np.float32(0.0)).astype(np.float32)
    theta_new = theta.copy()
    if np.float32(lr) != 0:
        theta_new = np.where(live, theta + np.float32(lr) * grad, theta).astype(np.float32)
    return grad, theta_new


def population_geometry(n_envs: int, members: int, rows_per_member: Optional[int] = None):
    """(P, G) of a population over a batch: P members of G consecutive environments each, G a multiple of 16 (a 16-row tile of the
    launch never straddles two members) and P * G == n_envs.  Raises ValueError otherwise."""
    n, P = int(n_envs), int(members)
    if P < 1:
        raise ValueError("PolicyPopulation: members must be >= 1, got %d" % P)
    G = n // P if rows_per_member is None else int(rows_per_member)
    if G < 16 or G % 16:
        raise ValueError("PolicyPopulation: %d rows per member -- must be a positive multiple of 16 (%d environments, %d members)" % (G, n, P))
    if P * G != n:
        raise ValueError("PolicyPopulation: %d members x %d rows do not cover %d environments" % (P, G, n))
    return P, G


# ------------------------------------------------------------------------------------------------------------------ the device side
def _lib():
    from .batched_env import _LIB, _check
    return _LIB, _check


def _arch_arg(hidden):
    from . import _capi
    return _capi.AuvPolicyArch(int(hidden[0]), int(hidden[1]), int(hidden[2]))


def net_hidden(pi) -> tuple:
    """The hidden widths of a policy net `pi` (a Sequential of Linear and activation modules): the out_features of every Linear but
    the last, as FusedActorCritic reads them."""
    import torch.nn as nn
    lin = [m for m in pi if isinstance(m, nn.Linear)]
    return tuple(int(l.out_features) for l in lin[:-1])


def pack_member(pi, obs_dim: int, out=None, hidden=HIDDEN):
    """One member block from a policy net `pi` (Linear-Tanh x 3 + Linear: obs -> `hidden` -> 2; the reference's [256, 128, 64] unless
    named): what pack_policy_params writes for the first net.  Device-side copies on the current stream."""
    import torch
    import torch.nn as nn
    from .policy import pack_linear
    hidden = _hidden(hidden, "pack_member")
    lin = [m for m in pi if isinstance(m, nn.Linear)]
    act = [m for m in pi if not isinstance(m, nn.Linear)]
    if tuple(l.out_features for l in lin[:-1]) != hidden or lin[-1].out_features != 2 or lin[0].in_features != int(obs_dim) \
            or not all(isinstance(a, nn.Tanh) for a in act):
        raise ValueError("pack_member: the population kernel evaluates obs[%d] -> %s tanh -> 2" % (int(obs_dim), list(hidden)))
    nf = member_floats(obs_dim, hidden)
    with torch.no_grad():
        p = torch.zeros(nf, dtype=torch.float32, device=lin[0].weight.device) if out is None else out
        off = 0
        for j, l in enumerate(lin):
            out_p = l.out_features if j < 3 else 16
            in_p = ((int(obs_dim) + 31) & ~31) if j == 0 else l.in_features
            p[off:off + out_p * in_p].copy_(pack_linear(l.weight, out_p, in_p))
            off += out_p * in_p
            p[off:off + out_p].zero_()
            p[off:off + l.out_features].copy_(l.bias)
            off += out_p
        p[off:].zero_()
    return p


_ACT_OUTPUTS = ("mu", "action")


def population_act(members, obs_dim: int, G: int, X, want: Sequence[str] = ("mu",), action_map=None, out: Optional[Dict] = None,
                   hidden=HIDDEN, arch_entry: Optional[bool] = None):
    """auv_population_act on the caller's current stream: row j of X through the policy net of member j // G, ONE launch.

    members     [P, stride] float32 device tensor, rows contiguous and 16-byte aligned, stride >= member_floats(obs_dim, hidden) and a
                multiple of 4; P * G >= the number of rows
    hidden      the hidden widths the members were packed for, one of _capi.POLICY_ARCHS
    arch_entry  None: the default widths go through auv_population_act, any other through auv_population_act_arch; True: the _arch
                entry also for the default widths (it runs the same kernel)
    X           [M, obs_dim] float32; rows may be strided, columns may not
    want        any of "mu" [M, 2], "action" [M, 2]
    action_map  (act_mid, act_half, clip_lo, clip_hi), each two floats; None: the identity map without clipping
    out         tensors to write into, by name; "action" may be a row-strided [M, 2] view (rows of an environment's action buffer)
    For the same row and the same block the mean has the bits policy.policy_eval gives.  Raises ValueError for what the launch refuses."""
    import torch
    from . import _capi
    LIB, check = _lib()
    want, out = tuple(want), dict(out or {})
    obs_dim, G = int(obs_dim), int(G)
    hidden = _hidden(hidden, "population_act")
    if not want or any(w not in _ACT_OUTPUTS for w in want) or any(w not in want for w in out):
        raise ValueError("population_act: want must name some of %s, and out only what is wanted" % (_ACT_OUTPUTS,))
    if G < 16 or G % 16:
        raise ValueError("population_act: G = %d must be a positive multiple of 16" % G)
    if obs_dim < 1:
        raise ValueError("population_act: obs_dim must be >= 1")
    nf = member_floats(obs_dim, hidden)
    if not isinstance(members, torch.Tensor) or members.dtype != torch.float32 or not members.is_cuda or members.dim() != 2 \
            or members.stride(1) != 1 or members.shape[1] < nf or members.data_ptr() % 16:
        raise ValueError("population_act: members must be a 16-byte aligned [P, >= %d] float32 device tensor with contiguous rows" % nf)
    stride = int(members.stride(0)) if members.shape[0] > 1 else int(members.shape[1])
    if stride % 4 or stride < nf:
        raise ValueError("population_act: member stride %d must be a multiple of 4 and >= %d" % (stride, nf))
    dev = members.device
    if not isinstance(X, torch.Tensor) or X.dtype != torch.float32 or X.device != dev or X.dim() != 2 or X.shape[1] != obs_dim:
        raise ValueError("population_act: X must be an [M, %d] float32 tensor on %s" % (obs_dim, dev))
    M = int(X.shape[0])
    if M > 1 and X.stride(1) != 1:
        raise ValueError("population_act: the columns of X must be contiguous (rows may be strided)")
    ldx = int(X.stride(0)) if M > 1 else obs_dim
    if ldx < obs_dim:
        raise ValueError("population_act: row stride of X %d < obs_dim %d" % (ldx, obs_dim))
    if M > members.shape[0] * G:
        raise ValueError("population_act: %d rows need %d members of %d rows, got %d" % (M, -(-M // G), G, members.shape[0]))
    io = _capi.AuvPopulationIO()
    res = {}
    with torch.cuda.device(dev):
        for w in want:
            t = out.get(w)
            if t is None:
                t = torch.empty((M, 2), dtype=torch.float32, device=dev)
            elif not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev or tuple(t.shape) != (M, 2):
                raise ValueError("population_act: out[%r] must be an [%d, 2] float32 tensor on %s" % (w, M, dev))
            elif w == "action":
                if M > 0 and (t.stride(1) != 1 or (M > 1 and t.stride(0) < 2)):
                    raise ValueError("population_act: out['action'] must have contiguous columns and a row stride >= 2")
            elif not t.is_contiguous():
                raise ValueError("population_act: out[%r] must be contiguous" % w)
            res[w] = t
            setattr(io, w, t.data_ptr() if M else None)
        if M == 0:
            return res
        io.members, io.stride, io.G = members.data_ptr(), stride, G
        io.X, io.ldx, io.M, io.obs_dim = X.data_ptr(), ldx, M, obs_dim
        io.action_ld = int(res["action"].stride(0)) if "action" in res and M > 1 else 2
        io.accumulate, io.act = 0, 1
        _set_action_map(io, action_map)
        st = torch.cuda.current_stream(dev)
        dev_i = dev.index if dev.index is not None else torch.cuda.current_device()
        if hidden != HIDDEN or arch_entry:
            check(LIB.auv_population_act_arch(dev_i, C.byref(io), C.byref(_arch_arg(hidden)), C.c_void_p(st.cuda_stream)), "auv_population_act_arch")
        else:
            check(LIB.auv_population_act(dev_i, C.byref(io), C.c_void_p(st.cuda_stream)), "auv_population_act")
    return res


def _set_action_map(io, action_map):
    mid, half, lo, hi = ((0.0, 0.0), (1.0, 1.0), (float("-inf"),) * 2, (float("inf"),) * 2) if action_map is None else action_map
    for k in range(2):
        io.act_mid[k], io.act_half[k], io.clip_lo[k], io.clip_hi[k] = float(mid[k]), float(half[k]), float(lo[k]), float(hi[k])


class PolicyPopulation:
    """P policies over the environments of `env`, member p driving environments [p G, (p + 1) G).

    env               a BatchedAuvEnv (n_envs == members * rows_per_member)
    members           P; perturb / update use mirrored pairs (2 j, 2 j + 1) and want it even
    rows_per_member   G, a multiple of 16; default env.n_envs // members
    net               a module with a policy net `net.pi` (or the Sequential itself) to take the base block from; None: zeros
    hidden            the hidden widths, one of _capi.POLICY_ARCHS: read off `net` where there is one, else this, else [256, 128, 64];
                      ValueError for any other triple (csrc/k14_population_arch.hip holds the kernels of the non-default ones)
    action map        as FusedActorCritic: action = act_mid + act_half * clip(mu, clip_lo, clip_hi); default: raw units clipped to the
                      action space
    seed              keys the noise of perturb / update together with their `generation`

    Owns `theta` [member_floats] (the base block), `members` [P, stride], `grad` [member_floats], `fit` [N] float32 (sum of rewards of
    the last rollout window), `ends` [N] int32 (episodes ended in it) and `actions` [N, 2].  No method synchronises with the host."""

    @staticmethod
    def resolve_hidden(net=None, hidden=None) -> tuple:
        """The hidden widths of a population: read off `net.pi` (or `net`, a Sequential) as FusedActorCritic reads them off its
        modules, else `hidden`, else the reference's.  ValueError for a triple that is not compiled in, or a `hidden` that
        contradicts `net`.  Touches no device."""
        if net is None:
            return _hidden(HIDDEN if hidden is None else hidden, "PolicyPopulation")
        h = _hidden(net_hidden(getattr(net, "pi", net)), "PolicyPopulation")
        if hidden is not None and tuple(int(x) for x in hidden) != h:
            raise ValueError("PolicyPopulation: hidden = %s, the net has the hidden widths %s" % (list(hidden), list(h)))
        return h

    def __init__(self, env, members: int, rows_per_member: Optional[int] = None, net=None, act_mid=None, act_half=None, clip_lo=None,
                 clip_hi=None, seed: int = 0, hidden=None, squash: bool = False):
        if squash:
            raise ValueError("PolicyPopulation: squash = True -- the population launches have no tanh-squashed variant (FusedActorCritic's "
                             "plain launches do)")
        self.P, self.G = population_geometry(env.n_envs, members, rows_per_member)
        self.hidden = self.resolve_hidden(net, hidden)
        import torch
        from . import _capi
        self.env, self.device, self.obs_dim = env, env.device, int(env.obs_dim)
        self.seed = int(seed) & _U64
        LIB, _ = _lib()
        # the default widths go through the entries without _arch (FusedActorCritic's rule)
        self._arch = _arch_arg(self.hidden) if self.hidden != HIDDEN else None
        self.nf = int(LIB.auv_population_member_floats_arch(self.obs_dim, C.byref(_arch_arg(self.hidden))))
        assert self.nf == member_floats(self.obs_dim, self.hidden)
        self.stride = self.nf
        N = env.n_envs
        with torch.cuda.device(self.device):
            self.theta = torch.zeros(self.nf, dtype=torch.float32, device=self.device)
            self.grad = torch.zeros(self.nf, dtype=torch.float32, device=self.device)
            self.members = torch.zeros((self.P, self.stride), dtype=torch.float32, device=self.device)
            self.fit = torch.zeros(N, dtype=torch.float32, device=self.device)
            self.ends = torch.zeros(N, dtype=torch.int32, device=self.device)
            self.actions = torch.zeros((N, 2), dtype=torch.float32, device=self.device)
        lo_t, hi_t = [float(x) for x in env.action_space.low], [float(x) for x in env.action_space.high]
        self.action_map = (tuple([0.0, 0.0] if act_mid is None else [float(x) for x in act_mid]),
                           tuple([1.0, 1.0] if act_half is None else [float(x) for x in act_half]),
                           tuple(lo_t if clip_lo is None else [float(x) for x in clip_lo]),
                           tuple(hi_t if clip_hi is None else [float(x) for x in clip_hi]))
        self._io_type = _capi.AuvPopulationIO
        self._streams = []                                    # rollout(bounds=...): the chains' streams
        if net is not None:
            self.load(net)

    def _dev_index(self):
        import torch
        return self.device.index if self.device.index is not None else torch.cuda.current_device()

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device)

    # ------------------------------------------------------------------------------ weights
    def load(self, net):
        """The base block from `net.pi` (or from `net` itself, a Sequential), and every member a copy of it."""
        pack_member(getattr(net, "pi", net), self.obs_dim, out=self.theta, hidden=self.hidden)
        self.members.copy_(self.theta.unsqueeze(0).expand(self.P, self.stride))

    def base_state_into(self, fused):
        """`theta` into the policy half of a FusedActorCritic's packed buffer (a slice copy): the champion can then be run through
        fused.predict() / examples/evaluate.py.  The torch modules of `fused` are not touched: do not refresh() afterwards."""
        if getattr(fused, "squash", False):
            raise ValueError("base_state_into: the policy was made with squash = True -- the population's members act through the clipped "
                             "affine map, a squashed predict() would run another policy")
        if int(fused.env.obs_dim) != self.obs_dim:
            raise ValueError("base_state_into: obs_dim %d, the population has %d" % (int(fused.env.obs_dim), self.obs_dim))
        if tuple(getattr(fused, "hidden", HIDDEN)) != self.hidden:
            raise ValueError("base_state_into: the policy has the hidden widths %s, the population %s"
                             % (list(getattr(fused, "hidden", HIDDEN)), list(self.hidden)))
        fused.params[:self.nf].copy_(self.theta)

    def perturb(self, sigma: float, generation: int):
        """members[p] = theta +- sigma eps(seed, generation, p // 2, .) for every member, one launch (auv_population_perturb)."""
        LIB, check = _lib()
        head = (self._dev_index(), C.c_void_p(self.theta.data_ptr()), C.c_void_p(self.members.data_ptr()), self.stride, self.P, self.obs_dim,
                float(sigma), self.seed, int(generation))
        st = C.c_void_p(self._stream().cuda_stream)
        if self._arch is not None:
            check(LIB.auv_population_perturb_arch(*head, C.byref(self._arch), st), "auv_population_perturb_arch")
        else:
            check(LIB.auv_population_perturb(*head, st), "auv_population_perturb")

    def update(self, weights, lr: float, sigma: float, generation: int):
        """The ES gradient estimate of generation `generation` from the shaped fitness `weights` [P] into `grad`, and theta += lr * grad
        (lr = 0: the estimate only): one launch (auv_population_update), the noise regenerated from its counters."""
        import torch
        if self.P % 2:
            raise ValueError("update: mirrored pairs need an even number of members, got %d" % self.P)
        if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or weights.device != self.device or tuple(weights.shape) != (self.P,) \
                or not weights.is_contiguous():
            raise ValueError("update: weights must be a contiguous [%d] float32 tensor on %s" % (self.P, self.device))
        LIB, check = _lib()
        head = (self._dev_index(), C.c_void_p(self.theta.data_ptr()), C.c_void_p(weights.data_ptr()), C.c_void_p(self.grad.data_ptr()), self.P,
                self.obs_dim, float(sigma), float(lr), self.seed, int(generation))
        st = C.c_void_p(self._stream().cuda_stream)
        if self._arch is not None:
            check(LIB.auv_population_update_arch(*head, C.byref(self._arch), st), "auv_population_update_arch")
        else:
            check(LIB.auv_population_update(*head, st), "auv_population_update")
        return self.grad

    @staticmethod
    def centered_ranks(fitness):
        """Rank-shaped fitness in [-0.5, 0.5] (the best member 0.5), [P] float32: what OpenAI-ES feeds its estimate.  torch ops."""
        import torch
        P = fitness.numel()
        ranks = torch.empty(P, dtype=torch.float32, device=fitness.device)
        ranks[torch.argsort(fitness)] = torch.arange(P, dtype=torch.float32, device=fitness.device)
        return ranks / max(P - 1, 1) - 0.5

    # ------------------------------------------------------------------------------ acting
    def act(self, obs=None, out=None):
        """The deterministic action of every environment's member for the rows `obs` (None: the environment's observation buffer)
        into `out` (default `self.actions`, which env.step takes as is): one launch on the caller's current stream."""
        X = self.env.obs if obs is None else obs
        out = self.actions if out is None else out
        return population_act(self.members, self.obs_dim, self.G, X, want=("action",), action_map=self.action_map, out={"action": out},
                              hidden=self.hidden)["action"]

    def _io(self):
        io = self._io_type()
        io.members, io.stride, io.G = self.members.data_ptr(), self.stride, self.G
        io.M, io.obs_dim, io.action_ld = self.env.n_envs, self.obs_dim, 2
        io.action, io.fit, io.ends = self.actions.data_ptr(), self.fit.data_ptr(), self.ends.data_ptr()
        _set_action_map(io, self.action_map)
        return io

    def rollout(self, n_steps: int, bounds: Optional[Sequence[int]] = None):
        """A window of `n_steps` steps of every environment under its member: per step the population launch and the environment's
        step back to back, one C call (auv_population_rollout), and a last launch that adds the last step's reward.  Returns
        (fitness [P], ends [P]): per member the MEAN over its environments of the rewards summed over the window, and the number of
        episodes that ended in it; `self.fit` / `self.ends` hold the per-environment numbers.  Runs as one chain on the caller's
        current stream -- or, if the environment is split into sub-batches (env.set_sub_batches) whose bounds are multiples of G,
        as their chains; `bounds` (first environments of the chains, multiples of G, starting with 0) names a split of the caller's
        own instead.  Chains are ordered behind the caller's stream and the caller's stream behind them, on the device."""
        env = self.env
        LIB, check = _lib()
        cur = self._stream()
        self.fit.zero_()
        self.ends.zero_()
        N = env.n_envs
        if bounds is not None:
            # the caller's own split: chains on streams of the population's own (kept: a stream must outlive its work)
            import torch
            los = [int(b) for b in bounds]
            if not los or los[0] != 0 or any(b <= a for a, b in zip(los, los[1:])) or los[-1] >= N or any(lo % self.G for lo in los):
                raise ValueError("rollout: bounds must start at 0, increase, stay below %d and be multiples of G = %d, got %s" % (N, self.G, los))
            while len(self._streams) < len(los):
                self._streams.append(torch.cuda.Stream(device=self.device))
            k, subs = len(los), self._streams[:len(los)]
            bounds, streams = (C.c_int32 * (k + 1))(*(los + [N])), (C.c_void_p * k)(*[st.cuda_stream for st in subs])
        elif env._slices is not None and env.sub_batches > 1 and all(lo % self.G == 0 for lo, _ in env._slices):
            k, bounds, streams, subs = env.sub_batches, env._bounds_c, env._streams_c, env._sub_streams
        else:
            k, bounds, streams, subs = 1, (C.c_int32 * 2)(0, N), (C.c_void_p * 1)(cur.cuda_stream), []
        for st in subs:
            st.wait_stream(cur)
        ios = (self._io_type * k)(*[self._io() for _ in range(k)])
        tail = (C.c_void_p(env.obs.data_ptr()), C.c_void_p(env.reward.data_ptr()), C.c_void_p(env.done.data_ptr()), int(n_steps), 1)
        if self._arch is not None:
            check(LIB.auv_population_rollout_arch(env._h, k, bounds, streams, ios, C.byref(self._arch), *tail), "auv_population_rollout_arch")
        else:
            check(LIB.auv_population_rollout(env._h, k, bounds, streams, ios, *tail), "auv_population_rollout")
        for st in subs:
            cur.wait_stream(st)
        return self.fit.view(self.P, self.G).mean(dim=1), self.ends.view(self.P, self.G).sum(dim=1)
