"""FusedPPOUpdate -- one PPO minibatch step of examples/ppo.py as a few HIP launches (csrc/k8_ppo_update.hip, k13_ppo_update_arch.hip,
auv_ppo_*).

The reference trains PPO2 with `MlpPolicy`, net_arch [256, 128, 64] for policy and value function, tanh, a diagonal Gaussian with a
free log_std (the reference's scripts/run.py:332-357).  `minibatch_step` of examples/ppo.py evaluates that update with stock tensor
operations: two MLPs forward and backward, the loss, two global-norm clips, a diagnostics row and Adam -- more than a hundred small
launches behind five gathers.  This class runs the same arithmetic as five launches: the row pass (gather, forward, backward through
the activations), the weight-gradient pass, the fixed-order reduction, the norm and clip + Adam, which also scatters every updated
weight into the packed buffer of an attached FusedActorCritic (so `refresh()` is not needed between update and rollout).

    upd = FusedPPOUpdate(net, lr=2e-4, clip=0.2, vf_coef=0.5, ent_coef=0.01, max_batch=16384)
    upd.attach(fused)                              # optional: the rollout policy's packed weights follow every step
    stats = upd.step(O, A, LP, ADV, RET, idx)      # [10]: loss, pg, vf, max |adv|, max ratio, non-finite inputs, clipped fraction, 0,
                                                   #       |g_pi|, |g_v| before clipping -- a device tensor, nothing synchronises
    g, stats = upd.grad(O, A, LP, ADV, RET, idx)   # or in two halves, e.g. around an all-reduce of g
    upd.apply(g)

The same updater also takes supervised steps (k8_clone: the same row pass with another head): the policy towards target actions, the
value net towards target values -- a planner's decisions (planning.DistillBuffer), an autopilot's, a warm start for PPO:

    stats = upd.clone_step(O, A, RET, W, idx, kind="nll")   # [10]: loss, bc, vf, max |a - mu|, sum of weights, non-finite inputs, 0, 0,
                                                            #       |g_pi|, |g_v|;  kind "mse": squared error of the mean instead
    g, stats = upd.clone_grad(O, A, RET)                    # the two halves, as above

A tanh-squashed policy (policy.FusedActorCritic(..., squash=True)) is trained by an updater made with the CONSTRUCTOR flag
`FusedPPOUpdate(net, ..., squash=True)` -- one flag per updater, not per call, because it belongs to the policy the rows came from: grad()
and step() then go through auv_ppo_grad_squash, whose entropy term is the squashed distribution's, estimated on the stored actions
(squash_loss_terms below is the same loss in stock tensor operations); slot 7 of the record is then the mean entropy.  A holds PRE-SQUASH
actions and LP their Gaussian log-density, as the squash launches store them.  The clone steps do not look at the flag.

Hidden widths: read off `net.pi` / `net.v` (both the same triple), one of SUPPORTED_HIDDEN -- the reference's [256, 128, 64] and the
narrower nets the fused forward launches evaluate (policy.SUPPORTED_HIDDEN); anything else raises ValueError.  `upd.hidden` is the triple.

The module's parameters become views of ONE flat tensor (`upd.theta`, torch layout: pi W1 b1 .. W4 b4, v W1 .. b4, log_std); the torch
modules stay usable and stay the owners -- `net.v(obs)` sees every step.  Deterministic: the same inputs give the same bits.
"""
import ctypes as C
import math
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import _capi, policy

HIDDEN = (256, 128, 64)                      # the reference's hidden widths: the default, through the entries without _arch
SUPPORTED_HIDDEN = policy.SUPPORTED_HIDDEN   # the closed list the update is compiled for: the forward launches' (POL_ARCH_LIST)
CLONE_KINDS = {"nll": 0, "mse": 1}
_LIB = _capi.load_library()


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, _LIB.auv_last_error().decode()))


def clone_loss_terms(net, o, a, ret, w=None, kind="nll", vf_coef=0.5, ent_coef=0.0):
    """The loss of auv_ppo_grad_clone in stock tensor operations, on any device and dtype: (loss, bc, vf).  `net`: pi, v, log_std as
    examples/ppo.ActorCritic holds them; o [B, D], a [B, 2] target actions in the policy's own space, ret [B], w [B] >= 0 or None.
        nll: bc = mean_i w_i sum_k (0.5 z_ik^2 + log_std_k + log sqrt(2 pi)), z = (a - mu) / exp(log_std);  mse: mean_i w_i sum_k 0.5 (a - mu)^2
        vf = mean_i w_i 0.5 (v_i - ret_i)^2;  loss = bc + vf_coef vf - ent_coef sum_k (0.5 + log sqrt(2 pi) + log_std_k)
    The means are over all B rows, whatever their weights."""
    if kind not in CLONE_KINDS:
        raise ValueError("kind must be one of %s, got %r" % (sorted(CLONE_KINDS), kind))
    w = torch.ones_like(ret) if w is None else w
    mu, log_std = net.pi(o), net.log_std
    c = 0.5 * math.log(2.0 * math.pi)
    if kind == "nll":
        z = (a - mu) / log_std.exp()
        per_row = (0.5 * z * z + log_std + c).sum(-1)
    else:
        per_row = (0.5 * (a - mu) ** 2).sum(-1)
    bc = (w * per_row).mean()
    vf = (w * 0.5 * (net.v(o).squeeze(-1) - ret) ** 2).mean()
    loss = bc + vf_coef * vf - ent_coef * (0.5 + c + log_std).sum()
    return loss, bc, vf


def squash_loss_terms(net, o, a, lp, adv, ret, clip, vf_coef, ent_coef):
    """The loss of auv_ppo_grad_squash in stock tensor operations, on any device and dtype: (loss, pg, vf, ent).  `net`: pi, v, log_std as
    examples/ppo.ActorCritic holds them; o [B, D], a [B, 2] STORED (pre-squash) actions, lp [B] their Gaussian log-density under the
    collecting policy, adv and ret [B].
        pg, vf: minibatch_step's of examples/ppo.py -- ratio = exp(log N(a; mu, sigma) - lp), the clipped surrogate, 0.5 mean (v - ret)^2
        ent = mean_i sum_k [0.5 + log sqrt(2 pi) + log_std_k + log(1 - tanh^2 u_ik)],   u = mu + sigma * ((a - mu) / sigma).detach()
        loss = pg + vf_coef vf - ent_coef ent
    u has the value of the stored action and the gradient of a reparameterised sample: the noise is held, mu and sigma move it.
    log(1 - tanh^2 u) = 2 (log 2 - |u| - log1p(exp(-2 |u|))), finite for every finite u."""
    mu, log_std = net.pi(o), net.log_std
    sigma = log_std.exp()
    c = 0.5 * math.log(2.0 * math.pi)
    z = (a - mu) / sigma
    logp = (-0.5 * z * z - log_std - c).sum(-1)
    ratio = (logp - lp).exp()
    pg = -torch.min(ratio * adv, ratio.clamp(1 - clip, 1 + clip) * adv).mean()
    vf = 0.5 * ((net.v(o).squeeze(-1) - ret) ** 2).mean()
    u = mu + sigma * z.detach()
    au = u.abs()
    ent = (0.5 + c + log_std + 2.0 * (math.log(2.0) - au - torch.log1p(torch.exp(-2.0 * au)))).sum(-1).mean()
    loss = pg + vf_coef * vf - ent_coef * ent
    return loss, pg, vf, ent


class FusedPPOUpdate:
    LOG_ROWS = 8192

    def __init__(self, net: nn.Module, lr: float = 2e-4, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, clip: float = 0.2,
                 vf_coef: float = 0.5, ent_coef: float = 0.01, max_norm_pi: float = 0.5, max_norm_v: float = 0.5, max_batch: int = 16384,
                 arch_entry: Optional[bool] = None, squash: bool = False):
        """squash      True: grad() / step() train a tanh-squashed policy (auv_ppo_grad_squash; module docstring)
        arch_entry  None: the default widths go through auv_ppo_create, any other through auv_ppo_create_arch; True: the _arch entries
                    also for the default widths (they dispatch to the same kernels: tests compare the two)."""
        tensors = []
        # the hidden widths are read off the modules: both nets the same triple, one of SUPPORTED_HIDDEN
        self.hidden = None
        for seq, out in ((net.pi, 2), (net.v, 1)):
            lin = [m for m in seq if isinstance(m, nn.Linear)]
            act = [m for m in seq if not isinstance(m, nn.Linear)]
            dims = tuple(l.out_features for l in lin[:-1])
            if (dims not in SUPPORTED_HIDDEN or lin[-1].out_features != out or lin[0].in_features != net.pi[0].in_features
                    or not all(isinstance(a, nn.Tanh) for a in act) or any(l.bias is None for l in lin)):
                raise ValueError("FusedPPOUpdate trains obs -> [h1, h2, h3] tanh -> %d with three hidden layers and biases (another depth "
                                 "is not compiled in), [h1, h2, h3] one of %s (the reference's scripts/run.py:332-357 first); got %s -> %d"
                                 % (out, list(SUPPORTED_HIDDEN), list(dims), lin[-1].out_features))
            if self.hidden is not None and dims != self.hidden:
                raise ValueError("FusedPPOUpdate: net.pi has the hidden widths %s, net.v %s -- one updater trains both nets with the same "
                                 "widths, one of %s" % (list(self.hidden), list(dims), list(SUPPORTED_HIDDEN)))
            self.hidden = dims
            for l in lin:
                tensors += [l.weight, l.bias]
        if tuple(net.log_std.shape) != (2,):
            raise ValueError("FusedPPOUpdate: log_std must have two elements")
        tensors.append(net.log_std)
        self.net, self.obs_dim = net, int(net.pi[0].in_features)
        self.device = tensors[0].device
        if self.device.type != "cuda" or any(t.device != self.device or t.dtype != torch.float32 for t in tensors):
            raise ValueError("FusedPPOUpdate: the module must hold float32 parameters on one GPU")
        # the default widths go through the entries without _arch (unless arch_entry: the _arch entries then dispatch to the same kernels)
        self._arch = policy._arch_arg(self.hidden) if (self.hidden != HIDDEN or arch_entry) else None
        if self._arch is None:
            n = int(_LIB.auv_ppo_param_floats(self.obs_dim))
        else:
            n = int(_LIB.auv_ppo_param_floats_arch(self.obs_dim, C.byref(self._arch)))
        assert n == sum(t.numel() for t in tensors)
        # ONE flat tensor; every parameter becomes a view of it (the modules stay the owners of the weights)
        self.theta = torch.empty(n, dtype=torch.float32, device=self.device)
        off = 0
        with torch.no_grad():
            for t in tensors:
                view = self.theta[off:off + t.numel()].view_as(t)
                view.copy_(t)
                t.data = view
                off += t.numel()
        self.m, self.v = torch.zeros_like(self.theta), torch.zeros_like(self.theta)
        self.g = torch.zeros_like(self.theta)
        self.t = 0                                                  # Adam's step count
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.clip, self.vf_coef, self.ent_coef = float(clip), float(vf_coef), float(ent_coef)
        self.max_norm_pi, self.max_norm_v = float(max_norm_pi), float(max_norm_v)
        self.max_batch = int(max_batch)
        self.squash = bool(squash)
        # the record of every step, written by the launches themselves: row = stats[8] + the two norms; read it once per update
        self.log = torch.zeros((self.LOG_ROWS, 10), dtype=torch.float32, device=self.device)
        self.n_steps = 0
        self._fused = None
        h = C.c_void_p()
        if self._arch is None:
            _check(_LIB.auv_ppo_create(self.device.index or 0, self.obs_dim, self.max_batch, C.byref(h)), "auv_ppo_create")
        else:
            _check(_LIB.auv_ppo_create_arch(self.device.index or 0, self.obs_dim, self.max_batch, C.byref(self._arch), C.byref(h)),
                   "auv_ppo_create_arch")
        self._h = h
        self.load()

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _LIB.auv_ppo_destroy(h)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def load(self):
        """Pack the kernels' copies of the weights (and the attached policy buffer) from `theta`: after construction, and after
        anything else has written the parameters (a broadcast, a checkpoint)."""
        _check(_LIB.auv_ppo_load(self._h, C.c_void_p(self.theta.data_ptr()), self._stream()), "auv_ppo_load")

    def attach(self, fused=None):
        """Hand the packed weight buffer of a FusedActorCritic (exact f32 path) to the updater: every step then writes the updated
        weights there too, in the policy launch's layout.  None detaches."""
        if fused is None:
            _check(_LIB.auv_ppo_attach_policy(self._h, None), "auv_ppo_attach_policy")
            self._fused = None
            return
        if fused.bf16:
            raise ValueError("FusedPPOUpdate.attach: the bf16 policy keeps a second copy of the weights that only refresh() packs")
        if getattr(fused, "in_dim", fused.env.obs_dim) != self.obs_dim or fused.params.device != self.device:   # (in_dim: frames * obs_dim)
            raise ValueError("FusedPPOUpdate.attach: the policy has another observation width or device")
        if bool(getattr(fused, "squash", False)) != self.squash:
            raise ValueError("FusedPPOUpdate.attach: the policy was made with squash = %s, the updater with squash = %s"
                             % (bool(getattr(fused, "squash", False)), self.squash))
        hidden = tuple(getattr(fused, "hidden", HIDDEN))            # (the C side cannot see the buffer's length)
        if hidden != self.hidden:
            raise ValueError("FusedPPOUpdate.attach: the policy evaluates the hidden widths %s, the updater trains %s"
                             % (list(hidden), list(self.hidden)))
        _check(_LIB.auv_ppo_attach_policy(self._h, C.c_void_p(fused.params.data_ptr())), "auv_ppo_attach_policy")
        self._fused = fused                                         # (keeps the buffer alive)
        self.load()

    def _row(self):
        return self.log[self.n_steps % self.LOG_ROWS]

    def _rows(self, tensors, idx, B):
        """The argument checks of grad() and clone_grad(): `tensors` = (tensor, trailing shape) per stored column.  Returns (n_rows, B)."""
        n_rows = int(tensors[0][0].shape[0])
        for x, tail in tensors:
            shape = (n_rows,) + tail
            if tuple(x.shape) != shape or x.dtype != torch.float32 or not x.is_contiguous() or x.device != self.device:
                raise ValueError("FusedPPOUpdate: expected a contiguous float32 tensor of shape %s on %s, got %s %s"
                                 % (shape, self.device, tuple(x.shape), x.dtype))
        if idx is not None:
            if idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous() or idx.device != self.device:
                raise ValueError("FusedPPOUpdate: idx must be a contiguous int64 vector on %s" % self.device)
            B = int(idx.numel())
        elif B is None:
            B = n_rows
        return n_rows, int(B)

    def grad(self, O, A, LP, ADV, RET, idx: Optional[torch.Tensor] = None, B: Optional[int] = None):
        """The flat gradient of minibatch_step's loss over rows `idx` (int64; None: rows 0 .. B - 1, B default: all rows) of the stored
        transitions, and the statistics row (squash: of squash_loss_terms, slot 7 the mean entropy).  Returns (grad, stats): the updater's own buffers, overwritten by the next call."""
        n_rows, B = self._rows(((O, (self.obs_dim,)), (A, (2,)), (LP, ()), (ADV, ()), (RET, ())), idx, B)
        batch, entry = (_capi.AuvPpoSquashBatch, "auv_ppo_grad_squash") if self.squash else (_capi.AuvPpoBatch, "auv_ppo_grad")
        b = batch(O.data_ptr(), A.data_ptr(), LP.data_ptr(), ADV.data_ptr(), RET.data_ptr(),
                  idx.data_ptr() if idx is not None else None, int(B), n_rows, self.clip, self.vf_coef, self.ent_coef)
        row = self._row()
        _check(getattr(_LIB, entry)(self._h, C.byref(b), C.c_void_p(self.g.data_ptr()), C.c_void_p(row.data_ptr()), self._stream()), entry)
        return self.g, row[:8]

    def apply(self, grad: Optional[torch.Tensor] = None):
        """Clip per group, one Adam step, and the repack of every weight.  Returns the two norms before clipping ([2], device)."""
        g = self.g if grad is None else grad
        if g.numel() != self.theta.numel() or g.dtype != torch.float32 or not g.is_contiguous() or g.device != self.device:
            raise ValueError("FusedPPOUpdate.apply: the gradient must be a contiguous float32 vector of %d elements" % self.theta.numel())
        self.t += 1
        b1, b2 = self.betas
        a = _capi.AuvPpoAdam(self.lr, b1, b2, self.eps, 1.0 - b1 ** self.t, 1.0 - b2 ** self.t, self.max_norm_pi, self.max_norm_v)
        row = self._row()
        _check(_LIB.auv_ppo_adam(self._h, C.c_void_p(self.theta.data_ptr()), C.c_void_p(self.m.data_ptr()), C.c_void_p(self.v.data_ptr()),
                                 C.c_void_p(g.data_ptr()), C.byref(a), C.c_void_p(row[8:].data_ptr()), self._stream()), "auv_ppo_adam")
        self.n_steps += 1
        return row[8:]

    def step(self, O, A, LP, ADV, RET, idx: Optional[torch.Tensor] = None):
        """grad then apply on the current stream.  Returns the step's record [10] (see the module's docstring)."""
        row = self._row()
        self.grad(O, A, LP, ADV, RET, idx)
        self.apply()
        return row

    def clone_grad(self, O, A, RET, W: Optional[torch.Tensor] = None, idx: Optional[torch.Tensor] = None, B: Optional[int] = None,
                   kind: str = "nll", vf_coef: Optional[float] = None, ent_coef: Optional[float] = None):
        """The flat gradient of clone_loss_terms over rows `idx` of the stored rows (as grad(): int64; None: rows 0 .. B - 1, B default:
        all rows), and the statistics row: loss, bc, vf, max |a - mu| over rows of weight > 0, the sum of the weights, non-finite
        inputs, 0, 0.  A: target actions in the policy's own space; W: row weights >= 0 (None: all one); vf_coef / ent_coef default to the
        updater's.  Returns (grad, stats): the updater's own buffers, overwritten by the next call."""
        if kind not in CLONE_KINDS:
            raise ValueError("FusedPPOUpdate.clone_grad: kind must be one of %s, got %r" % (sorted(CLONE_KINDS), kind))
        cols = ((O, (self.obs_dim,)), (A, (2,)), (RET, ())) + (((W, ()),) if W is not None else ())
        n_rows, B = self._rows(cols, idx, B)
        b = _capi.AuvPpoCloneBatch(O.data_ptr(), A.data_ptr(), RET.data_ptr(), W.data_ptr() if W is not None else None,
                                   idx.data_ptr() if idx is not None else None, B, n_rows, CLONE_KINDS[kind],
                                   self.vf_coef if vf_coef is None else float(vf_coef), self.ent_coef if ent_coef is None else float(ent_coef))
        row = self._row()
        _check(_LIB.auv_ppo_grad_clone(self._h, C.byref(b), C.c_void_p(self.g.data_ptr()), C.c_void_p(row.data_ptr()), self._stream()),
               "auv_ppo_grad_clone")
        return self.g, row[:8]

    def clone_step(self, O, A, RET, W: Optional[torch.Tensor] = None, idx: Optional[torch.Tensor] = None, B: Optional[int] = None,
                   kind: str = "nll", vf_coef: Optional[float] = None, ent_coef: Optional[float] = None):
        """clone_grad then apply on the current stream.  Returns the step's record [10]: clone_grad's statistics and the two norms."""
        row = self._row()
        self.clone_grad(O, A, RET, W, idx, B, kind, vf_coef, ent_coef)
        self.apply()
        return row
