"""-m gpu: frame-stacked observations in the fused policy rollout (csrc/k12_policy_stacked.hip: auv_policy_act_stacked,
auv_policy_rollout_stacked, auv_stack_frames) against the NumPy mirror (gym_auv_amd/framestack.py: stack_reference), auv_policy_eval
and auv_policy_act.  Everything here is bit for bit (torch.equal): stacking is copying, and the stacked launch runs the matrix chains
and the epilogue of the plain one.

N = 40 environments (two full 16-row tiles and a ragged one of 8), max_timesteps = 5, T = 12 steps per rollout, two rollouts back to
back with a flush between them.  Odd environments are three steps into their episode when the rollouts begin, so episodes end inside
a rollout (steps 5 and 10 of the even, 2 and 7 of the odd environments) and AT its last step (step 12 of the odd ones: the first
launch of the second rollout then starts their history).  Two widths: obs_dim 6 (LiDAR off) with k = 3 -- 18 columns, no multiple of
32 -- and obs_dim 26 (2 sectors x 10 sensors) with k = 4 -- 104 columns, across three 32-column k-steps and padded to 128.

Two slices: BatchedAuvEnv cuts slices at multiples of 64 environments, which leaves 40 environments in one piece; the nearest it allows
is N = 104 cut at 64, whose second slice has the 40 environments (and the ragged tile) of the other cases."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

from gym_auv_amd.config import effective_reference_config
from gym_auv_amd.scenarios import moving_obstacles_world
from gym_auv_amd.world import build_world, pack_bank

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

DEV = "cuda:0"
N, T, MAX_T = 40, 12, 5
CASES = [(6, 3), (26, 4)]                                  # (obs_dim, frames)
AUV_EINVAL = -1


@functools.lru_cache(maxsize=None)
def _bank(lidar):
    return pack_bank([build_world(moving_obstacles_world(2000 + i) if lidar else moving_obstacles_world(2000 + i, 0, 0)) for i in range(16)])


def _cfg(n_sensors):
    """n_sensors = 0: LiDAR off (6 columns); else two sectors of n_sensors / 2 beams (6 + n_sensors columns)."""
    cfg = effective_reference_config(use_lidar=n_sensors > 0)
    cfg.episode.max_timesteps = MAX_T
    if n_sensors:
        assert n_sensors % 2 == 0
        cfg.vessel.n_sectors, cfg.vessel.n_sensors_per_sector = 2, n_sensors // 2
    return cfg


def _env(n_sensors, n=N, slices=1):
    import warnings
    from gym_auv_amd.batched_env import BatchedAuvEnv
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # (16 worlds for 40 auto-resetting environments: fine here)
        env = BatchedAuvEnv(_cfg(n_sensors), _bank(n_sensors > 0), n, device=DEV, rewarder="colav" if n_sensors else "pathfollow")
    env.reset()
    # odd environments three steps into their episode (module docstring)
    zero = torch.zeros((n, 2), dtype=torch.float32, device=DEV)
    for _ in range(3):
        env.step(zero)
    mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
    mask[0::2] = 1
    env.reset(mask)
    torch.cuda.synchronize()
    env.set_sub_batches(slices, probe_streams=False)
    assert env.sub_batches == slices
    return env


def _net(width, seed=5):
    import ppo
    torch.manual_seed(seed)
    net = ppo.ActorCritic(width).to(DEV)
    with torch.no_grad():
        net.log_std.copy_(torch.tensor([-0.5, -1.1]))
        for m in net.modules():                            # weights of ordinary size, biases that matter
            if isinstance(m, torch.nn.Linear):
                m.bias.uniform_(-0.3, 0.3)
    return net


def _fused(env, frames, seed=5, **kw):
    from gym_auv_amd.policy import FusedActorCritic
    fused = FusedActorCritic(_net(frames * env.obs_dim, seed), env, rollout=T, debug=True, seed=seed, reward_scale=0.01, reward_clip=50.0,
                             frames=frames, **kw)
    ios = fused._sios if frames > 1 else fused._ios
    for i in range(1, len(fused.slices)):                  # ONE seed for every chain: the samples are then a function of (seed, step, environment)
        if frames > 1:
            ios[i].io.seed = ios[0].io.seed
        else:
            ios[i].seed = ios[0].seed
    return fused


def _state(fused):
    torch.cuda.synchronize()
    return fused.stack.hist.clone(), fused.stack.stk.clone()


def _lib():
    from gym_auv_amd.batched_env import _LIB
    return _LIB


class Run:
    """Two rollouts of T steps through the stacked launch one step at a time (act + step_slice), with everything a step saw and gave."""

    def __init__(self, n_sensors, frames):
        self.env = env = _env(n_sensors)
        self.fused = fused = _fused(env, frames)
        self.frames, self.D = frames, env.obs_dim
        self.obs, self.done, self.mu, self.gstep, self.actions = [], [], [], [], []
        self.buffers, self.flush_state = [], []
        for rnd in range(2):
            fused.begin_rollout()
            for t in range(T):
                torch.cuda.synchronize()
                self.obs.append(env.obs.clone()), self.done.append(env.done.clone())     # the env's buffers, read before the launch
                self.gstep.append(fused._g[0])
                fused.act(0)
                torch.cuda.synchronize()
                self.mu.append(fused.mu.clone()), self.actions.append(fused.actions.clone())
                env.step_slice(0, fused.actions)
            before = _state(fused)
            fused.act(0)                                   # the flush launch
            self.flush_state.append((before, _state(fused)))
            self.buffers.append([x.clone() for x in fused.buffers()])
        self.end_state = _state(fused)
        obs = torch.stack(self.obs).cpu().numpy()
        done = torch.stack(self.done).cpu().numpy()
        from gym_auv_amd.framestack import stack_reference
        self.rows, self.mirror_state = stack_reference(obs, done, frames)               # [2 T, N, frames * D]: computed once, never modified
        self.rows_dev = torch.as_tensor(self.rows, device=DEV)


@functools.lru_cache(maxsize=None)
def _run(n_sensors, frames):
    return Run(n_sensors, frames)


def _sensors(obs_dim):
    return obs_dim - 6


# ------------------------------------------------------------------------------ 1. k = 1
@pytest.mark.parametrize("obs_dim", [6, 26])
def test_one_frame_is_the_plain_rollout_bit_for_bit(obs_dim):
    """auv_policy_rollout_stacked with frames = 1 (hist and stk NULL) against auv_policy_rollout from the same seed and reset."""
    from gym_auv_amd import _capi
    lib = _lib()
    ea, eb = _env(_sensors(obs_dim)), _env(_sensors(obs_dim))
    fa, fb = _fused(ea, 1), _fused(eb, 1)
    s = (_capi.AuvPolicyStack * 1)()
    s[0].io, s[0].hist, s[0].stk, s[0].frames = fb._ios[0], None, None, 1
    for rnd in range(2):
        fa.begin_rollout(), fb.begin_rollout()
        fa.rollout(T)
        t0, g0 = (C.c_int64 * 1)(fb._t[0]), (C.c_int64 * 1)(fb._g[0])
        rc = lib.auv_policy_rollout_stacked(eb._h, 1, eb._bounds_c, eb._streams_c, s, C.c_void_p(eb.obs.data_ptr()), C.c_void_p(eb.reward.data_ptr()),
                                            C.c_void_p(eb.done.data_ptr()), T, 1, t0, g0)
        assert rc == 0, lib.auv_last_error()
        fb._t[0], fb._g[0] = min(fb._t[0] + T + 1, T + 1), fb._g[0] + T + 1
        torch.cuda.synchronize()
        for name, x, y in zip("O A LP V R Dn".split(), fa.buffers(), fb.buffers()):
            assert torch.equal(x, y), (rnd, name)
        assert torch.equal(fa.actions, fb.actions) and torch.equal(fa.mu, fb.mu) and torch.equal(fa.eps, fb.eps)
        assert torch.equal(fa.buf[0]["ctr"], fb.buf[0]["ctr"])
        assert torch.equal(ea.read("STATE"), eb.read("STATE")) and torch.equal(ea.obs, eb.obs)
        assert float(fa.buffers()[5].sum()) > 0                           # episodes did end
    # ... and the single launch, on the device's counters
    fa.begin_rollout(), fb.begin_rollout()
    fa.act(0)
    rc = lib.auv_policy_act_stacked(eb._h, 0, N, C.byref(s[0]), C.c_void_p(eb._sub_streams[0].cuda_stream))
    assert rc == 0, lib.auv_last_error()
    torch.cuda.synchronize()
    for x, y in zip(fa.buffers(), fb.buffers()):
        assert torch.equal(x, y)
    assert torch.equal(fa.actions, fb.actions) and torch.equal(fa.mu, fb.mu) and torch.equal(fa.buf[0]["ctr"], fb.buf[0]["ctr"])
    ea.close(), eb.close()


# ------------------------------------------------------------------------------ 2. stacked rows
@pytest.mark.parametrize("obs_dim,frames", CASES)
def test_stacked_rows_equal_the_mirror_and_the_rollout_call_equals_the_loop(obs_dim, frames):
    r = _run(_sensors(obs_dim), frames)
    done = torch.stack(r.done)
    # the shapes under test did occur: dones inside both rollouts, and in front of the second rollout's first launch
    assert int(done[1:T].sum()) > 0 and int(done[T + 1:].sum()) > 0 and 0 < int(done[T].sum()) < N
    for rnd in range(2):
        O = r.buffers[rnd][0]
        assert O.shape == (T, N, frames * obs_dim)
        assert torch.equal(O, r.rows_dev[rnd * T:(rnd + 1) * T]), rnd
    hist, stk = r.end_state
    assert np.array_equal(hist.cpu().numpy(), r.mirror_state["hist"])
    assert np.array_equal((stk[:, 0] & 255).cpu().numpy(), r.mirror_state["pos"]) and np.array_equal(stk[:, 1].cpu().numpy(), r.mirror_state["age"])
    # the same two rollouts as ONE call each
    env = _env(_sensors(obs_dim))
    fused = _fused(env, frames)
    for rnd in range(2):
        fused.begin_rollout()
        fused.rollout(T)
        torch.cuda.synchronize()
        for name, x, y in zip("O A LP V R Dn".split(), fused.buffers(), r.buffers[rnd]):
            assert torch.equal(x, y), (rnd, name)
    h2, s2 = _state(fused)
    assert torch.equal(h2, hist) and torch.equal(s2, stk)
    assert torch.equal(env.read("STATE"), r.env.read("STATE"))
    env.close()


# ------------------------------------------------------------------------------ 3. network outputs
@pytest.mark.parametrize("obs_dim,frames", CASES)
def test_means_and_values_are_policy_eval_on_the_mirror_rows_and_the_epilogue_is_the_plain_launch(obs_dim, frames):
    from gym_auv_amd import _capi
    from gym_auv_amd.batched_env import BatchedAuvEnv
    from gym_auv_amd.policy import policy_eval
    lib = _lib()
    r = _run(_sensors(obs_dim), frames)
    W = frames * obs_dim
    # "the same matrix chains": auv_policy_eval on the mirror's rows
    for k in range(2 * T):
        ev = policy_eval(r.fused.params, W, r.rows_dev[k], want=("mu", "value"))
        assert torch.equal(ev["mu"], r.mu[k]), k
        assert torch.equal(ev["value"], r.buffers[k // T][3][k % T]), k
    # the epilogue: auv_policy_act of a handle whose observation has W columns, the mirror's rows as its observation buffer, the same
    # seed, rollout position and generator step
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        wide = BatchedAuvEnv(_cfg(W - 6), _bank(True), N, device=DEV)
    wide.reset()
    assert wide.obs_dim == W
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=DEV)   # noqa: E731
    A, LP, V, R, Dn, act, mu = z(T, N, 2), z(T, N), z(T, N), z(T, N), z(T, N), z(N, 2), z(N, 2)
    ctr = torch.zeros(4, dtype=torch.int64, device=DEV)
    io = _capi.AuvPolicyIO()
    C.memmove(C.byref(io), C.byref(r.fused._sios[0].io), C.sizeof(io))
    io.obs_dim, io.O, io.eps_out, io.ctr = W, None, None, ctr.data_ptr()
    io.A, io.LP, io.V, io.R, io.Dn, io.actions_out, io.mu_out = (x.data_ptr() for x in (A, LP, V, R, Dn, act, mu))
    for k in range(2 * T):
        t = k % T
        ctr[0], ctr[1], ctr[2] = t, r.gstep[k], 0
        io.obs = r.rows_dev[k].data_ptr()
        torch.cuda.synchronize()
        rc = lib.auv_policy_act(wide._h, 0, N, C.byref(io), None)
        assert rc == 0, lib.auv_last_error()
        torch.cuda.synchronize()
        buf = r.buffers[k // T]
        assert torch.equal(mu, r.mu[k]) and torch.equal(V[t], buf[3][t]), k
        assert torch.equal(A[t], buf[1][t]) and torch.equal(LP[t], buf[2][t]), k
        assert torch.equal(act, r.actions[k]), k
    wide.close()


# ------------------------------------------------------------------------------ 4. two slices
def test_two_slices_equal_one():
    obs_dim, frames, n = 26, 4, 104
    runs = []
    for slices in (1, 2):
        env = _env(_sensors(obs_dim), n=n, slices=slices)
        if slices == 2:
            assert [lo for lo, _ in env._slices] == [0, 64] and env._slices[1][1] == N
        fused = _fused(env, frames)
        got = []
        for rnd in range(2):
            fused.begin_rollout()
            fused.rollout(T)
            torch.cuda.synchronize()
            got += [x.clone() for x in fused.buffers()] + [fused.actions.clone(), fused.mu.clone()]
        got += list(_state(fused)) + [env.read("STATE"), env.obs.clone()]
        runs.append(got)
        env.close()
    assert len(runs[0]) == len(runs[1])
    for j, (x, y) in enumerate(zip(*runs)):
        assert torch.equal(x, y), j
    assert float(runs[0][5].sum()) > 0


# ------------------------------------------------------------------------------ 5. the flush launch
@pytest.mark.parametrize("obs_dim,frames", CASES)
def test_the_flush_launch_leaves_the_history_alone(obs_dim, frames):
    r = _run(_sensors(obs_dim), frames)
    for (h0, s0), (h1, s1) in r.flush_state:
        assert torch.equal(h0, h1) and torch.equal(s0, s1)
        assert int(s0[:, 1].min()) >= 1                                    # (there WAS a history to spoil)
    # ... and it did store the last step's reward and done
    for rnd in range(2):
        assert torch.equal(r.buffers[rnd][5][T - 1], r.done[T].float() if rnd == 0 else r.env.done.float())
    assert float(r.buffers[0][5][T - 1].sum()) > 0                         # episodes that end at a rollout's last step


# ------------------------------------------------------------------------------ 6. auv_stack_frames
@pytest.mark.parametrize("obs_dim,frames", CASES + [(6, 1), (5, 3), (8, 2)])
def test_stack_frames_push_and_peek(obs_dim, frames):
    """The row copy at 4 (obs_dim 5), 8 (6, 26) and 16 bytes (8) per lane: push over 12 steps equals the mirror, peek returns the row
    push would and stores nothing.  Rows: the recorded rollout's where there is one, random rows and dones otherwise."""
    from gym_auv_amd.framestack import FrameStack, stack_reference
    if (obs_dim, frames) in CASES:
        r = _run(_sensors(obs_dim), frames)
        obs, done = r.obs[:T], r.done[:T]
    else:
        g = torch.Generator().manual_seed(obs_dim)
        obs = [torch.randn(N, obs_dim, generator=g).to(DEV) for _ in range(T)]
        done = [(torch.rand(N, generator=g) < 0.2).to(torch.uint8).to(DEV) for _ in range(T)]
    want, _ = stack_reference(torch.stack(obs).cpu().numpy(), torch.stack(done).cpu().numpy(), frames)
    fs = FrameStack((N, obs_dim), frames, device=DEV)
    for t in range(T):
        h0, s0 = fs.hist.clone(), fs.stk.clone()
        peek = fs.peek(obs[t], done[t])
        torch.cuda.synchronize()
        assert torch.equal(fs.hist, h0) and torch.equal(fs.stk, s0), t
        rows = fs.push(obs[t], done[t])
        assert torch.equal(rows, peek), t
        assert np.array_equal(rows.cpu().numpy(), want[t]), t
    # a strided output: columns of a wider buffer
    wide = torch.full((N, frames * obs_dim + 3), 7.0, device=DEV)
    out = fs.peek(obs[0], None, out=wide[:, :frames * obs_dim])
    again = fs.peek(obs[0], None)
    assert torch.equal(out, again) and float(wide[:, frames * obs_dim:].min()) == 7.0


@pytest.mark.parametrize("obs_dim,frames", CASES)
def test_value_and_predict_without_rows_use_the_peeked_row(obs_dim, frames):
    from gym_auv_amd.framestack import stack_reference
    from gym_auv_amd.policy import policy_eval
    r = _run(_sensors(obs_dim), frames)
    env, fused = r.env, r.fused
    before = _state(fused)
    v = fused.value()
    a = fused.predict(out=torch.empty((N, 2), dtype=torch.float32, device=DEV))
    row = fused.stack.peek(env.obs, env.done)
    after = _state(fused)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    nxt, _ = stack_reference(env.obs.cpu().numpy()[None], env.done.cpu().numpy()[None], frames, r.mirror_state)
    assert np.array_equal(row.cpu().numpy(), nxt[0])
    ev = policy_eval(fused.params, frames * obs_dim, row, want=("value", "action"), action_map=fused.action_map)
    assert torch.equal(v, ev["value"]) and torch.equal(a, ev["action"])
    # reset_frames: the next row is the observation and zeros
    fused.reset_frames(torch.arange(0, N, 2, device=DEV))
    row = fused.stack.peek(env.obs, env.done)
    assert torch.equal(row[:, :obs_dim], env.obs) and float(row[0::2, obs_dim:].abs().max()) == 0.0
    fused.stack.stk.copy_(before[1])                                       # (the shared run is left as it was)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ 7. refusals
def test_refusals_name_the_function():
    from gym_auv_amd import _capi
    lib = _lib()
    r = _run(_sensors(26), 4)
    env, fused = r.env, r.fused
    st = C.c_void_p(env._sub_streams[0].cuda_stream)
    t0, g0 = (C.c_int64 * 1)(0), (C.c_int64 * 1)(0)

    def both(s):
        rc = lib.auv_policy_act_stacked(env._h, 0, N, C.byref(s), st)
        assert rc == AUV_EINVAL and b"auv_policy_act_stacked" in lib.auv_last_error(), (rc, lib.auv_last_error())
        arr = (_capi.AuvPolicyStack * 1)(s)
        rc = lib.auv_policy_rollout_stacked(env._h, 1, env._bounds_c, env._streams_c, arr, C.c_void_p(env.obs.data_ptr()),
                                            C.c_void_p(env.reward.data_ptr()), C.c_void_p(env.done.data_ptr()), 1, 0, t0, g0)
        assert rc == AUV_EINVAL and b"auv_policy_rollout_stacked" in lib.auv_last_error(), (rc, lib.auv_last_error())

    def copy():
        s = _capi.AuvPolicyStack()
        C.memmove(C.byref(s), C.byref(fused._sios[0]), C.sizeof(s))
        return s
    before = _state(fused)
    for frames in (9, 0):
        s = copy()
        s.frames = frames
        both(s)
    s = copy()
    s.io.params_bf16 = fused.params.data_ptr()
    both(s)
    for field in ("hist", "stk"):
        s = copy()
        setattr(s, field, None)
        both(s)
    # a width over the LDS limit: 546 columns (three channels of 180 beams) x 5 frames
    import warnings
    from gym_auv_amd.batched_env import BatchedAuvEnv
    cfg = effective_reference_config(use_lidar=True)
    cfg.vessel.sensor_use_velocity_observations = True
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        big = BatchedAuvEnv(cfg, _bank(True), 16, device=DEV)
    big.reset()
    assert big.obs_dim == 546
    s = copy()
    s.io.obs_dim, s.io.ld, s.frames = 546, 16, 5
    s.io.obs = big.obs.data_ptr()
    rc = lib.auv_policy_act_stacked(big._h, 0, 16, C.byref(s), st)
    assert rc == AUV_EINVAL and b"auv_policy_act_stacked" in lib.auv_last_error() and b"LDS" in lib.auv_last_error(), lib.auv_last_error()
    big.close()
    # auv_stack_frames
    x = torch.zeros((N, 26), device=DEV)
    out = torch.zeros((N, 26 * 9), device=DEV)
    h, k = fused.stack.hist, fused.stack.stk
    for frames, ldx, hist in ((9, 26 * 9, h), (4, 103, h), (4, 104, None)):
        rc = lib.auv_stack_frames(0, C.c_void_p(x.data_ptr()), None, C.c_void_p(hist.data_ptr()) if hist is not None else None,
                                  C.c_void_p(k.data_ptr()), C.c_void_p(out.data_ptr()), ldx, 0, N, 26, frames, 0, None)
        assert rc == AUV_EINVAL and b"auv_stack_frames" in lib.auv_last_error(), (frames, ldx, lib.auv_last_error())
    after = _state(fused)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])      # nothing was enqueued


# ------------------------------------------------------------------------------ 8. the update on stacked rows
def test_ppo_update_runs_on_the_stacked_rows():
    """One FusedPPOUpdate.step on the stacked O of a rollout (obs_dim 26, k = 4): the gradient against autograd by the rule and with the
    helper of tests/test_gpu_ppo_update.py (e(fused) <= max(8 e(g32), 1e-5) per tensor against fp64), then the step moves `params`."""
    from gym_auv_amd.ppo_update import FusedPPOUpdate
    from test_gpu_ppo_update import CLIP, ENT, VF, assert_parity
    obs_dim, frames = 26, 4
    env = _env(_sensors(obs_dim))
    fused = _fused(env, frames)
    upd = FusedPPOUpdate(fused.net, clip=CLIP, vf_coef=VF, ent_coef=ENT, max_batch=T * N)
    upd.attach(fused)
    fused.begin_rollout()
    fused.rollout(T)
    torch.cuda.synchronize()
    O, A, LP, V, R, Dn = fused.buffers()
    W = frames * obs_dim
    assert float(O[:, :, obs_dim:].abs().max()) > 0                        # there is history in the rows
    torch.manual_seed(3)
    adv = torch.randn(T * N, device=DEV)
    adv = torch.where(adv.abs() < 1e-3, torch.ones_like(adv), adv)
    data = (O.reshape(T * N, W).clone(), A.reshape(T * N, 2).clone(), LP.reshape(T * N).clone(), adv, torch.randn(T * N, device=DEV))
    idx = torch.randperm(T * N, device=DEV)[:333].contiguous()
    assert_parity(fused.net, data, upd, idx, "stacked %d x %d" % (frames, obs_dim))
    before = fused.params.clone()
    stats = upd.step(*data, idx)
    torch.cuda.synchronize()
    assert torch.isfinite(stats).all() and float(stats[5]) == 0.0
    assert not torch.equal(before, fused.params)
    changed = (before != fused.params).float().mean()
    assert float(changed) > 0.5                                            # (the padding columns of W1 stay zero)
    env.close()


# ------------------------------------------------------------------------------ 9. the launch tag in stk
TAG_MOD = 0x7fffff                                                         # tag = generator step mod (2^23 - 1), plus 1: 1 .. 2^23 - 1


def _tag(g):
    return g % TAG_MOD + 1


@functools.lru_cache(maxsize=None)
def _tag_case():
    """obs_dim 6, k = 3, four steps in: even environments hold three frames, odd ones two (their episode ended at step 2).  The state
    in front of the fifth launch, and what the mirror makes of it.  Nothing here is modified afterwards (the device state is put back
    by every launch of the tests below)."""
    from gym_auv_amd.framestack import stack_reference
    env = _env(0)
    fused = _fused(env, 3)
    fused.begin_rollout()
    for _ in range(4):
        fused.act(0)
        env.step_slice(0, fused.actions)
    h0, s0 = _state(fused)
    obs, done = env.obs.clone(), env.done.clone()
    state0 = dict(hist=h0.cpu().numpy(), pos=(s0[:, 0] & 255).cpu().numpy(), age=s0[:, 1].cpu().numpy())
    assert sorted(set(state0["age"].tolist())) == [2, 3]
    row, state1 = stack_reference(obs.cpu().numpy()[None], done.cpu().numpy()[None], 3, state0)
    return env, fused, h0, s0, obs, state0, torch.as_tensor(row[0], device=DEV), state1


def _launch_at(g, stk_in):
    """One auv_policy_act_stacked launch at generator step g on the case's history with `stk_in` in stk: checks O, mean, value and the
    state behind the launch against the mirror's ONE step from the case's state."""
    from gym_auv_amd.policy import policy_eval
    env, fused, h0, s0, obs, state0, row, state1 = _tag_case()
    assert torch.equal(env.obs, obs)
    fused.stack.hist.copy_(h0), fused.stack.stk.copy_(stk_in)
    fused.begin_rollout()
    with torch.cuda.stream(env._sub_streams[0]):
        fused.buf[0]["ctr"][1] = g
    fused._g[0] = g
    torch.cuda.synchronize()
    fused.act(0)
    torch.cuda.synchronize()
    O, A, LP, V, R, Dn = fused.buffers()
    assert torch.equal(O[0], row), g
    ev = policy_eval(fused.params, 18, row, want=("mu", "value"))
    assert torch.equal(fused.mu, ev["mu"]) and torch.equal(V[0], ev["value"]), g
    hist, stk = _state(fused)
    assert np.array_equal(hist.cpu().numpy(), state1["hist"]), g
    assert int(stk[:, 0].min()) >= 0, g                                                   # the tag never reaches the sign bit
    assert np.array_equal((stk[:, 0] & 255).cpu().numpy(), state1["pos"]) and np.array_equal(stk[:, 1].cpu().numpy(), state1["age"]), g
    assert int((stk[:, 0] >> 8).min()) == int((stk[:, 0] >> 8).max()) == _tag(g), g
    assert int(fused.buf[0]["ctr"][1]) == g + 1


TAG_STEPS = [0, 7, TAG_MOD - 1, TAG_MOD, 2 ** 23, 3 * TAG_MOD + 11]      # TAG_MOD - 1: the largest tag; TAG_MOD = 2^23 - 1: the wrap to tag 1


@pytest.mark.parametrize("g", TAG_STEPS)
def test_a_workgroup_that_finds_its_own_launch_tag_takes_the_state_as_it_stands(g):
    """What the value workgroup of a tile meets when its policy sibling has stored already, made deterministic: stk holds (pos', age')
    with THIS launch's tag before the launch.  Both workgroups must form the row of (pos', age') as they stand -- the mirror's row for
    the state before -- and not advance a second time."""
    state1 = _tag_case()[7]
    stk_in = torch.as_tensor(np.stack([state1["pos"] | (_tag(g) << 8), state1["age"]], 1).astype(np.int32), device=DEV)
    _launch_at(g, stk_in)


@pytest.mark.parametrize("g", TAG_STEPS)
def test_a_foreign_tag_and_no_tag_advance_normally(g):
    state0 = _tag_case()[5]
    for tag in (0, _tag(g + 1), _tag(g + TAG_MOD - 1), 1 if _tag(g) != 1 else 2, TAG_MOD if _tag(g) != TAG_MOD else TAG_MOD - 1):
        assert tag != _tag(g)
        stk_in = torch.as_tensor(np.stack([state0["pos"] | (tag << 8), state0["age"]], 1).astype(np.int32), device=DEV)
        _launch_at(g, stk_in)


def test_more_workgroups_than_are_resident_at_once():
    """obs_dim 6, k = 3, N = 16384: 1024 tiles x 2 nets, several times what the device holds at once, so value workgroups do start
    behind policy workgroups that have finished.  The value of every row is the value net on the row the POLICY workgroup wrote to O,
    and O's older frames are the newer frames of the rows before."""
    from gym_auv_amd.policy import policy_eval
    n, D, k = 16384, 6, 3
    env = _env(0, n=n)
    fused = _fused(env, k)
    for rnd in range(2):
        fused.begin_rollout()
        fused.rollout(T)
        torch.cuda.synchronize()
        O, A, LP, V, R, Dn = fused.buffers()
        for t in range(T):
            assert torch.equal(policy_eval(fused.params, k * D, O[t], want=("value",))["value"], V[t]), (rnd, t)
        for t in range(1, T):
            cont = Dn[t - 1] == 0
            assert torch.equal(O[t][cont][:, D:2 * D], O[t - 1][cont][:, :D]), (rnd, t)
            assert float(O[t][~cont][:, D:].abs().max()) == 0.0 if bool((~cont).any()) else True
            if t >= 2:
                cont2 = cont & (Dn[t - 2] == 0)
                assert torch.equal(O[t][cont2][:, 2 * D:], O[t - 2][cont2][:, :D]), (rnd, t)
        assert float(Dn.sum()) > 0
    stk = fused.stack.stk
    assert int(stk[:, 0].min()) >= 0 and int((stk[:, 0] & 255).max()) == int((stk[:, 0] & 255).min()) == (2 * T) % k
    env.close()
