"""Frame-stacked observations: the last `frames` observations of every environment as ONE input row (what stable-baselines, which the
reference trains with, ships as VecFrameStack), kept and formed on the device (csrc/k12_policy_stacked.hip).

A row has frames * obs_dim columns, NEWEST FIRST: columns [j * obs_dim, (j + 1) * obs_dim) hold the observation of j steps ago, j = 0
the current one -- a column permutation of stable-baselines' newest-last order -- and zeros where the episode is younger than j steps
(stable-baselines zeroes the stack at a reset).  The state per environment is a ring hist[N][frames][obs_dim] and stk[N][2]:
(pos | tag << 8, age) -- pos the slot of the newest frame, age the number of valid frames; tag is the policy launch's own mark,
(generator step mod (2^23 - 1)) + 1 (include/auv_hip.h, auv_policy_stack).  One step of the history, given the observation and the done flag of the step just completed:

    age' = min((done ? 0 : age) + 1, frames);  pos' = (pos + 1) mod frames
    row  = [obs | hist[(pos' - 1) mod frames] if 1 < age' else 0 | ... ];  hist[pos'] = obs;  (pos, age) = (pos', age')

Inside rollouts `FusedActorCritic(..., frames=k)` does this in its policy launch.  This module is for the loops around it:

    fs = FrameStack(env, 4)                 # or FrameStack((n_rows, obs_dim), 4, device=...)
    rows = fs.push(env.obs, env.done)       # [N, 4 * obs_dim]: the history moves on (auv_stack_frames, one launch)
    rows = fs.peek(env.obs, env.done)       # the row push would return; nothing is stored
    fs.reset()                              # behind env.reset(): every history empty

`stack_reference` is the NumPy mirror of the same rule: pure copying, so it is exact.
"""
import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _capi

MAX_FRAMES = _capi.MAX_FRAMES


def stack_reference(obs_seq, done_seq, frames: int, state: Optional[dict] = None) -> Tuple[np.ndarray, dict]:
    """The stacked rows of T consecutive history steps, in NumPy.

    obs_seq   [T, N, D]: the observation buffer in front of each step (launch)
    done_seq  [T, N]: the done buffer in front of each step -- the flag of the environment step completed just before it
    state     None: empty histories; or what an earlier call returned, to continue from
    Returns (rows [T, N, frames * D] in obs_seq's dtype, state) with state = dict(hist [N, frames, D], pos [N], age [N]): the ring as
    the device holds it."""
    obs_seq = np.asarray(obs_seq)
    done_seq = np.asarray(done_seq).astype(bool)
    frames = int(frames)
    if obs_seq.ndim != 3 or done_seq.shape != obs_seq.shape[:2]:
        raise ValueError("stack_reference: obs_seq [T, N, D] and done_seq [T, N], got %s and %s" % (obs_seq.shape, done_seq.shape))
    if frames < 1 or frames > MAX_FRAMES:
        raise ValueError("stack_reference: frames = %d outside [1, %d]" % (frames, MAX_FRAMES))
    T, N, D = obs_seq.shape
    if state is None:
        hist = np.zeros((N, frames, D), dtype=obs_seq.dtype)
        pos, age = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    else:
        hist, pos, age = state["hist"].copy(), state["pos"].astype(np.int64), state["age"].astype(np.int64)
        if hist.shape != (N, frames, D):
            raise ValueError("stack_reference: the state holds %s, the call needs %s" % (hist.shape, (N, frames, D)))
    rows = np.zeros((T, N, frames * D), dtype=obs_seq.dtype)
    env = np.arange(N)
    for t in range(T):
        age = np.minimum(np.where(done_seq[t], 0, age) + 1, frames)
        pos = (pos + 1) % frames
        rows[t, :, :D] = obs_seq[t]
        for j in range(1, frames):
            old = hist[env, (pos - j) % frames]
            rows[t, :, j * D:(j + 1) * D] = np.where((j < age)[:, None], old, 0)
        hist[env, pos] = obs_seq[t]
    return rows, dict(hist=hist, pos=pos, age=age)


class FrameStack:
    """The history of N rows on the device and the launch that moves it on (auv_stack_frames), without a network: for loops that do
    not go through FusedActorCritic.rollout -- a deterministic evaluation loop, the planner's prior, the GAE bootstrap."""

    def __init__(self, env_or_shape, frames: int, device=None):
        import torch
        self.frames = int(frames)
        if self.frames < 1 or self.frames > MAX_FRAMES:
            raise ValueError("FrameStack: frames = %d outside [1, %d]" % (self.frames, MAX_FRAMES))
        if hasattr(env_or_shape, "n_envs"):
            self.n, self.obs_dim = int(env_or_shape.n_envs), int(env_or_shape.obs_dim)
            device = env_or_shape.device if device is None else device
        else:
            self.n, self.obs_dim = (int(x) for x in env_or_shape)
        if self.n < 1 or self.obs_dim < 1:
            raise ValueError("FrameStack: %d rows of %d columns" % (self.n, self.obs_dim))
        self.device = torch.device("cuda:0" if device is None else device)
        if self.device.type == "cuda" and self.device.index is None:           # ("cuda": tensors report their index, compare like with like)
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.width = self.frames * self.obs_dim
        self.hist = torch.zeros((self.n, self.frames, self.obs_dim), dtype=torch.float32, device=self.device)
        self.stk = torch.zeros((self.n, 2), dtype=torch.int32, device=self.device)

    @property
    def pos(self):
        """[N] int32: the ring slot of every environment's newest frame."""
        return self.stk[:, 0] & 255

    @property
    def age(self):
        """[N] int32: the number of valid frames of every environment."""
        return self.stk[:, 1]

    def reset(self, envs=None):
        """Empty the history of `envs` (indices or a boolean mask; None: all) on the current stream."""
        if envs is None:
            self.stk[:, 1].zero_()
        else:
            self.stk[:, 1][envs] = 0

    def _launch(self, obs, done, out, advance: bool):
        import torch
        from .batched_env import _check, _LIB
        if not isinstance(obs, torch.Tensor) or obs.dtype != torch.float32 or obs.device != self.device or not obs.is_contiguous() \
                or tuple(obs.shape) != (self.n, self.obs_dim):
            raise ValueError("FrameStack: obs must be a contiguous float32 [%d, %d] tensor on %s" % (self.n, self.obs_dim, self.device))
        if done is not None and (not isinstance(done, torch.Tensor) or done.dtype not in (torch.uint8, torch.bool) or done.device != self.device
                                 or not done.is_contiguous() or tuple(done.shape) != (self.n,)):
            raise ValueError("FrameStack: done must be a contiguous uint8 or bool [%d] tensor on %s" % (self.n, self.device))
        if out is None:
            out = torch.empty((self.n, self.width), dtype=torch.float32, device=self.device)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != self.device or tuple(out.shape) != (self.n, self.width) \
                or out.stride(1) != 1 or (self.n > 1 and out.stride(0) < self.width):
            raise ValueError("FrameStack: out must be a float32 [%d, %d] tensor on %s with contiguous columns" % (self.n, self.width, self.device))
        ldx = int(out.stride(0)) if self.n > 1 else self.width
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream(self.device)
            _check(_LIB.auv_stack_frames(self.device.index if self.device.index is not None else torch.cuda.current_device(),
                                         C.c_void_p(obs.data_ptr()), C.c_void_p(done.data_ptr()) if done is not None else None,
                                         C.c_void_p(self.hist.data_ptr()), C.c_void_p(self.stk.data_ptr()), C.c_void_p(out.data_ptr()), ldx,
                                         0, self.n, self.obs_dim, self.frames, int(advance), C.c_void_p(st.cuda_stream)), "auv_stack_frames")
        return out

    def push(self, obs, done=None, out=None):
        """Move every history on by `obs` [N, obs_dim] (done [N]: the flags of the step just completed; None: nobody is done) and return
        the stacked rows [N, frames * obs_dim] -- one launch on the current stream."""
        return self._launch(obs, done, out, True)

    def peek(self, obs, done=None, out=None):
        """The rows push(obs, done) would return; the history stays as it is."""
        return self._launch(obs, done, out, False)
