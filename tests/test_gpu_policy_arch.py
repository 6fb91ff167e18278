"""-m gpu: the fused forward launches at the hidden widths (128, 128, 64), (128, 64, 64) and (64, 64, 64) (csrc/auv_policy_mfma.h:
PolArch, POL_ARCH_LIST; the auv_policy_*_arch entries) -- against the torch modules in fp32, bit for bit across the launches (act /
rollout, eval, stacked), and the default widths through the new entries against the old ones.

Shapes: 40 environments (two full 16-row tiles and a ragged one of 8) as two sub-batch chains of 24 + 16, T = 3, observation widths 6
(LiDAR off, K0p = 32) and 186 (180 beams), a small world of static circles, episodes of 3 steps with the odd environments one step into
theirs, so that episodes end inside the rollout.

Tolerance against torch: 1e-5 absolute on means, values and log-probabilities alike -- what DESIGN.md section 5 and
tests/test_gpu_policy.py hold this kernel's means to at [256, 128, 64]; a narrower net sums fewer products, so nothing wider is needed
(the test prints what it measures).  Everything else is torch.equal."""
import ctypes as C
import functools
import os
import sys
import warnings

import pytest
import torch

from gym_auv_amd import _capi
from gym_auv_amd.config import effective_reference_config
from gym_auv_amd.scenarios import static_circles_world
from gym_auv_amd.world import build_world, pack_bank

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

DEV = "cuda:0"
N, T, MAX_T = 40, 3, 3
BOUNDS = (0, 24, 40)
DEFAULT = (256, 128, 64)
NEW = [(128, 128, 64), (128, 64, 64), (64, 64, 64)]
LIDAR = [False, True]                                      # obs_dim 6 / 186
TOL = 1e-5


@functools.lru_cache(maxsize=None)
def _bank():
    return pack_bank([build_world(static_circles_world(3000 + i, 6)) for i in range(4)])


def _env(lidar):
    from gym_auv_amd.batched_env import BatchedAuvEnv
    cfg = effective_reference_config(use_lidar=lidar)
    cfg.episode.max_timesteps = MAX_T
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # (4 worlds for 40 auto-resetting environments: fine here)
        env = BatchedAuvEnv(cfg, _bank(), N, device=DEV, rewarder="colav" if lidar else "pathfollow")
    assert env.obs_dim == (186 if lidar else 6)
    env.reset()
    env.step(torch.zeros((N, 2), dtype=torch.float32, device=DEV))
    mask = torch.zeros(N, dtype=torch.uint8, device=DEV)
    mask[0::2] = 1
    env.reset(mask)                                        # odd environments stay one step into their episode
    torch.cuda.synchronize()
    env.set_sub_batches(2, probe_streams=False)
    # (set_sub_batches cuts at multiples of 64 environments: the 24 + 16 under test are put in place of its one slice)
    k = len(BOUNDS) - 1
    env._slices = [(BOUNDS[i], BOUNDS[i + 1] - BOUNDS[i]) for i in range(k)]
    env.sub_batches = k
    env._sub_streams = [torch.cuda.Stream(device=DEV) for _ in range(k)]
    env._bounds_c = (C.c_int32 * (k + 1))(*BOUNDS)
    env._streams_c = (C.c_void_p * k)(*[st.cuda_stream for st in env._sub_streams])
    return env


def _net(width, hidden, seed=5):
    import ppo
    torch.manual_seed(seed)
    net = ppo.ActorCritic(width, hidden=hidden).to(DEV)
    with torch.no_grad():
        net.log_std.copy_(torch.tensor([-0.5, -1.1]))
        for m in net.modules():                            # weights of ordinary size, biases that matter
            if isinstance(m, torch.nn.Linear):
                m.bias.uniform_(-0.3, 0.3)
    return net


def _fused(env, hidden, frames=1, **kw):
    from gym_auv_amd.policy import FusedActorCritic
    return FusedActorCritic(_net(frames * env.obs_dim, hidden), env, rollout=T, debug=True, seed=5, reward_scale=0.01, reward_clip=50.0,
                            frames=frames, **kw)


def _lib():
    from gym_auv_amd.batched_env import _LIB
    return _LIB


def _sync_buffers(fused):
    torch.cuda.synchronize()
    return [x.clone() for x in fused.buffers()]


class Stepwise:
    """A rollout one launch at a time -- act(i), the device-counter form, then the chain's step -- and the flush launch; keeps what
    every launch saw (obs, done) and gave (mu)."""

    def __init__(self, lidar, hidden, frames=1, **kw):
        self.env = env = _env(lidar)
        self.fused = fused = _fused(env, hidden, frames, **kw)
        self.obs, self.done, self.mu = [], [], []
        fused.begin_rollout()
        for t in range(T):
            torch.cuda.synchronize()
            self.obs.append(env.obs.clone()), self.done.append(env.done.clone())
            for i in range(env.sub_batches):
                fused.act(i)
            torch.cuda.synchronize()
            self.mu.append(fused.mu.clone())
            for i in range(env.sub_batches):
                env.step_slice(i, fused.actions)
        torch.cuda.synchronize()
        for i in range(env.sub_batches):
            fused.act(i)                                   # the flush launch
        self.buffers = _sync_buffers(fused)
        self.ctr = [b["ctr"].clone() for b in fused.buf]


def _rollout_call(lidar, hidden, frames=1, **kw):
    """The same rollout as ONE call (the host-count form, flush included)."""
    env = _env(lidar)
    fused = _fused(env, hidden, frames, **kw)
    fused.begin_rollout()
    fused.rollout(T, flush=True)
    return env, fused, _sync_buffers(fused)


@functools.lru_cache(maxsize=None)
def _stepwise(lidar, hidden, frames=1):
    return Stepwise(lidar, hidden, frames)                 # computed once, shared, never modified


def _equal(a, b, what):
    for x, y, name in zip(a, b, ("O", "A", "LP", "V", "R", "Dn")):
        assert torch.equal(x, y), (what, name)


@pytest.mark.parametrize("lidar", LIDAR)
@pytest.mark.parametrize("hidden", NEW)
def test_evaluate_matches_the_torch_modules(hidden, lidar):
    run = _stepwise(lidar, hidden)
    net, fused = run.fused.net, run.fused
    assert fused.hidden == hidden and fused.params.numel() == int(_lib().auv_policy_param_floats_arch(
        fused.in_dim, C.byref(_capi.AuvPolicyArch(*hidden))))
    O, A = run.buffers[0].reshape(T * N, -1), run.buffers[1].reshape(T * N, 2)
    lp, v, mu = fused.evaluate(O, A)
    with torch.no_grad():
        mu_ref, v_ref = net.pi(O), net.v(O).squeeze(-1)
        lp_ref = net.log_prob(mu_ref, A)
    torch.cuda.synchronize()
    e_mu = float((mu - mu_ref).abs().max())
    e_v = float((v - v_ref).abs().max())
    e_lp = float((lp - lp_ref).abs().max())
    print("hidden %s obs_dim %d: max |mu - ref| %.3e, |value - ref| %.3e, |logp - ref| %.3e" % (hidden, fused.in_dim, e_mu, e_v, e_lp))
    assert e_mu <= TOL and e_v <= TOL and e_lp <= TOL
    # the episodes did end inside the rollout, and the sampled actions are not the means
    assert bool(run.buffers[5].any()) and not torch.equal(A, mu)
    # predict / value: the same launch on the environment's rows
    assert torch.equal(fused.value(O), v)
    act = fused.predict(run.obs[0])
    lo, hi = (torch.as_tensor(x, device=DEV) for x in (run.env.action_space.low, run.env.action_space.high))
    assert torch.equal(act, torch.max(torch.min(run.mu[0], hi), lo))


@pytest.mark.parametrize("lidar", LIDAR)
@pytest.mark.parametrize("hidden", NEW)
def test_rollout_is_the_eval_launch_bit_for_bit(hidden, lidar):
    from gym_auv_amd.policy import policy_eval
    run = _stepwise(lidar, hidden)
    fused = run.fused
    O, A, LP, V, R, Dn = run.buffers
    for t in range(T):
        assert torch.equal(O[t], run.obs[t])
        r = policy_eval(fused.params, fused.in_dim, O[t], want=("mu", "value"), hidden=hidden)
        assert torch.equal(r["mu"], run.mu[t]) and torch.equal(r["value"], V[t]), t
        lp, v, mu = fused.evaluate(O[t], A[t])
        assert torch.equal(lp, LP[t]) and torch.equal(v, V[t]) and torch.equal(mu, run.mu[t]), t
    # a gathered, strided evaluation of the same rows
    wide = torch.zeros((T * N, fused.in_dim + 3), dtype=torch.float32, device=DEV)
    wide[:, :fused.in_dim] = O.reshape(T * N, -1)
    idx = torch.arange(T * N - 1, -1, -1, device=DEV)
    r = policy_eval(fused.params, fused.in_dim, wide[:, :fused.in_dim], idx=idx, want=("value",), hidden=hidden)
    assert torch.equal(r["value"], V.reshape(-1).flip(0))
    # gae runs on these buffers as on any
    adv, ret = fused.gae(V, fused.value(run.env.obs), 0.999, 0.98)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(adv).all()) and torch.equal(ret, adv + V)


@pytest.mark.parametrize("lidar", LIDAR)
@pytest.mark.parametrize("hidden", NEW)
def test_counter_forms_and_repeats_leave_the_same_buffers(hidden, lidar):
    run = _stepwise(lidar, hidden)                         # device counters, a flush launch of its own
    env1, f1, b1 = _rollout_call(lidar, hidden)            # host-named counters, the flush inside the call
    _equal(run.buffers, b1, "act(i) against rollout()")
    for i in range(2):
        assert torch.equal(run.ctr[i][:3], f1.buf[i]["ctr"][:3]) and int(run.ctr[i][0]) == T + 1
    assert torch.equal(run.env.obs, env1.obs)
    env2, f2, b2 = _rollout_call(lidar, hidden)            # the same seed again
    _equal(b1, b2, "two runs")
    for e in (env1, env2):
        e.close()


@pytest.mark.parametrize("lidar", LIDAR)
@pytest.mark.parametrize("hidden", NEW)
def test_one_frame_through_the_stacked_entry_is_the_plain_rollout(hidden, lidar):
    run = _stepwise(lidar, hidden)
    env = _env(lidar)
    fused = _fused(env, hidden)
    fused.begin_rollout()
    s = (_capi.AuvPolicyStack * 2)()
    for i in range(2):
        s[i].io, s[i].frames = fused._ios[i], 1            # hist, stk: NULL, not touched with one frame
    t0, g0 = (C.c_int64 * 2)(0, 0), (C.c_int64 * 2)(0, 0)
    rc = _lib().auv_policy_rollout_stacked_arch(env._h, 2, env._bounds_c, env._streams_c, s, C.byref(_capi.AuvPolicyArch(*hidden)),
                                                C.c_void_p(env.obs.data_ptr()), C.c_void_p(env.reward.data_ptr()),
                                                C.c_void_p(env.done.data_ptr()), T, 1, t0, g0)
    assert rc == 0, _lib().auv_last_error()
    _equal(run.buffers, _sync_buffers(fused), "frames = 1")
    env.close()


@pytest.mark.parametrize("lidar", LIDAR)
@pytest.mark.parametrize("hidden", NEW)
def test_two_frames_are_the_mirror_s_rows_through_the_eval_launch(hidden, lidar):
    from gym_auv_amd.framestack import stack_reference
    from gym_auv_amd.policy import policy_eval
    run = _stepwise(lidar, hidden, 2)
    fused = run.fused
    obs, done = torch.stack(run.obs).cpu().numpy(), torch.stack(run.done).cpu().numpy()
    rows, _ = stack_reference(obs, done, 2)
    rows = torch.as_tensor(rows, device=DEV)
    O, A, LP, V, R, Dn = run.buffers
    assert fused.in_dim == 2 * run.env.obs_dim and bool((rows[:, :, run.env.obs_dim:] != 0).any())
    for t in range(T):
        assert torch.equal(O[t], rows[t]), t
        r = policy_eval(fused.params, fused.in_dim, rows[t], actions=A[t], want=("mu", "value", "logp"), hidden=hidden)
        assert torch.equal(r["mu"], run.mu[t]) and torch.equal(r["value"], V[t]) and torch.equal(r["logp"], LP[t]), t
    env1, f1, b1 = _rollout_call(lidar, hidden, 2)         # the host-count form of the stacked rollout
    _equal(run.buffers, b1, "stacked: act(i) against rollout()")
    assert torch.equal(run.fused.stack.hist, f1.stack.hist)
    env1.close()


@pytest.mark.parametrize("lidar", LIDAR)
def test_default_widths_through_the_new_entries_are_the_old_entries(lidar):
    from gym_auv_amd.policy import policy_eval
    for frames in (1, 2):
        old = Stepwise(lidar, DEFAULT, frames)
        new = Stepwise(lidar, DEFAULT, frames, arch_entry=True)
        assert old.fused._arch is None and new.fused._arch is not None
        _equal(old.buffers, new.buffers, "act, frames = %d" % frames)
        for t in range(T):
            assert torch.equal(old.mu[t], new.mu[t])
        e_new, f_new, b_new = _rollout_call(lidar, DEFAULT, frames, arch_entry=True)
        _equal(old.buffers, b_new, "rollout, frames = %d" % frames)
        O, A = old.buffers[0].reshape(T * N, -1), old.buffers[1].reshape(T * N, 2)
        a = policy_eval(old.fused.params, old.fused.in_dim, O, actions=A, want=("mu", "value", "logp", "action"))
        b = policy_eval(old.fused.params, old.fused.in_dim, O, actions=A, want=("mu", "value", "logp", "action"), arch_entry=True)
        for k in a:
            assert torch.equal(a[k], b[k]), k
        for e in (old.env, new.env, e_new):
            e.close()


def test_the_entries_refuse_what_is_not_listed():
    env = _env(False)
    fused = _fused(env, (64, 64, 64))
    lib = _lib()
    st = C.c_void_p(env._sub_streams[0].cuda_stream)
    for h in [(64, 64, 32), (256, 128, 128), (64, 128, 64), (0, 0, 0)]:
        rc = lib.auv_policy_act_arch(env._h, 0, 24, C.byref(fused._ios[0]), C.byref(_capi.AuvPolicyArch(*h)), st)
        assert rc == -1 and b"not compiled in" in lib.auv_last_error(), h
    assert lib.auv_policy_act_arch(env._h, 0, 24, C.byref(fused._ios[0]), None, st) == -1
    ev = _capi.AuvPolicyEval()
    assert lib.auv_policy_eval_arch(0, C.byref(ev), C.byref(_capi.AuvPolicyArch(64, 64, 32)), None) == -1
    # bf16 weights with another triple than the default
    io = _capi.AuvPolicyIO.from_buffer_copy(fused._ios[0])
    io.params_bf16 = fused.params.data_ptr()
    rc = lib.auv_policy_act_arch(env._h, 0, 24, C.byref(io), C.byref(_capi.AuvPolicyArch(64, 64, 64)), st)
    assert rc == -1 and b"f32 only" in lib.auv_last_error()
    torch.cuda.synchronize()
    assert not bool(fused.A.any())                         # nothing was launched
    env.close()
