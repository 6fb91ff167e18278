"""-m gpu: running normalisation in the fused policy rollout (csrc/k16_policy_norm.hip) through the C ABI, against the NumPy mirrors of
gym_auv_amd/normalize.py, auv_policy_eval and auv_policy_act.  Everything is bit for bit.

N = 40 environments -- two full 16-row tiles and a ragged one of 8 -- as the two slices [0, 24) and [24, 40) on two streams: the first
slice ends in the ragged tile and the second has part_base = 2.  T = 3, max_timesteps = 5 with the odd environments three steps into
their episode, so episodes end inside the rollouts.  obs_dim 186 (even: float2 loads) and the pooled 15 (odd: scalar loads); hidden
widths [256, 128, 64] and [64, 64, 64].  The environment steps in the three-launch shape: the step is not what is under test here, and
slices that are no multiple of 64 are not a shape BatchedAuvEnv.set_sub_batches makes."""
import ctypes as C
import functools
import os
import sys
import warnings

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
N, T, MAX_T = 40, 3, 5
BOUNDS = [0, 24, 40]
SLICES = [(0, 24), (24, 16)]
AUV_EINVAL = -1
CASES = [(186, (256, 128, 64)), (15, (64, 64, 64)), (186, (64, 64, 64)), (15, (256, 128, 64))]


@functools.lru_cache(maxsize=None)
def _bank():
    return pack_bank([build_world(moving_obstacles_world(2000 + i)) for i in range(16)])


def _lib():
    from gym_auv_amd.batched_env import _LIB
    return _LIB


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _env(obs_dim):
    from gym_auv_amd.batched_env import BatchedAuvEnv
    cfg = effective_reference_config(use_lidar=True)
    cfg.episode.max_timesteps = MAX_T
    if obs_dim == 15:
        cfg.vessel.sensor_use_feasibility_pooling = True
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # (16 worlds for 40 auto-resetting environments: fine here)
        env = BatchedAuvEnv(cfg, _bank(), N, device=DEV, rewarder="colav")
    assert env.obs_dim == obs_dim
    env.set_step_mode("side_by_side")
    env.reset()
    zero = torch.zeros((N, 2), dtype=torch.float32, device=DEV)
    for _ in range(3):
        env.step(zero)
    mask = torch.zeros(N, dtype=torch.uint8, device=DEV)
    mask[0::2] = 1
    env.reset(mask)
    env.set_sub_batches(1, probe_streams=False)
    # the two slices of the module docstring, each on a stream of its own
    streams = [torch.cuda.Stream(device=DEV) for _ in SLICES]
    env._slices, env.sub_batches, env._sub_streams = list(SLICES), len(SLICES), streams
    env._bounds_c = (C.c_int32 * (len(SLICES) + 1))(*BOUNDS)
    env._streams_c = (C.c_void_p * len(SLICES))(*[s.cuda_stream for s in streams])
    torch.cuda.synchronize()
    return env


def _net(width, hidden, seed=5):
    import ppo
    torch.manual_seed(seed)
    net = ppo.ActorCritic(width, hidden=hidden).to(DEV)
    with torch.no_grad():
        net.log_std.copy_(torch.tensor([-0.5, -1.1]))
        for m in net.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.uniform_(-0.3, 0.3)
    return net


def _fused(env, hidden, normalize=None, seed=5):
    from gym_auv_amd.policy import FusedActorCritic
    fused = FusedActorCritic(_net(env.obs_dim, hidden, seed), env, rollout=T, debug=True, seed=seed, reward_scale=0.01, reward_clip=50.0,
                             normalize=normalize)
    return fused


def _norm(env, **kw):
    from gym_auv_amd.normalize import RunningNorm
    return RunningNorm(env.obs_dim, 0.99, **kw)


def _table(obs, seed=1):
    """A table that matters: per-column mean and deviation of the observations at hand (a few columns tightened so that values hit the
    clip), float32 [D, 2]."""
    x = obs.double().cpu().numpy()
    rs = np.random.RandomState(seed)
    mean = x.mean(0) + rs.uniform(-0.1, 0.1, x.shape[1])
    inv = 1.0 / (x.std(0) + 0.05)
    inv[::4] *= 400.0                                       # every fourth column: far outside the clip where it varies at all
    return torch.as_tensor(np.stack([mean, inv], 1).astype(np.float32), device=DEV)


def _sync_chains(env):
    torch.cuda.synchronize()


def _eval(fused, rows):
    from gym_auv_amd.policy import policy_eval
    return policy_eval(fused.params, fused.in_dim, rows, want=("mu", "value"), **fused._eval_kw())


# ------------------------------------------------------------------------------ 1. identity table
@pytest.mark.parametrize("obs_dim,hidden", CASES[:2])
def test_identity_table_is_the_plain_launch_bit_for_bit(obs_dim, hidden):
    ea, eb = _env(obs_dim), _env(obs_dim)
    fa = _fused(ea, hidden)
    nb = _norm(eb, clip_obs=1e30)
    fb = _fused(eb, hidden, normalize=nb)
    nb.table[:, 0], nb.table[:, 1] = 0.0, 1.0
    assert torch.equal(ea.obs, eb.obs) and float(ea.obs.abs().max()) < 1e30
    fa.begin_rollout(), fb.begin_rollout()
    for i in range(2):
        fa.act(i), fb.act(i)
    torch.cuda.synchronize()
    for name, x, y in zip("O A LP V".split(), fa.buffers(), fb.buffers()):
        assert torch.equal(x[0], y[0]), name
    assert torch.equal(fa.actions, fb.actions) and torch.equal(fa.mu, fb.mu) and torch.equal(fa.eps, fb.eps)
    for i in range(2):
        assert torch.equal(fa.buf[i]["ctr"], fb.buf[i]["ctr"])
    ea.close(), eb.close()


# ------------------------------------------------------------------------------ 2. + 3. a table that matters; the partials
class Run:
    """One rollout of T steps launch by launch (act + step_slice on both slices) under a non-trivial table, with everything a launch saw."""

    def __init__(self, obs_dim, hidden):
        self.env = env = _env(obs_dim)
        self.norm = norm = _norm(env)
        self.fused = fused = _fused(env, hidden, normalize=norm)
        norm.table.copy_(_table(env.obs))
        self.table = norm.table.cpu().numpy().copy()
        self.obs, self.mu, self.done = [], [], []
        fused.begin_rollout()
        for t in range(T):
            torch.cuda.synchronize()
            self.obs.append(env.obs.clone()), self.done.append(env.done.clone())
            for i in range(2):
                fused.act(i)
            torch.cuda.synchronize()
            self.mu.append(fused.mu.clone())
            for i in range(2):
                env.step_slice(i, fused.actions)
        torch.cuda.synchronize()
        self.part_before_flush, self.pcnt_before_flush = norm.part.clone(), norm.pcnt.clone()
        for i in range(2):
            fused.act(i)                                    # the flush launches
        torch.cuda.synchronize()
        self.buffers = [x.clone() for x in fused.buffers()]
        self.part, self.pcnt = norm.part.clone(), norm.pcnt.clone()


@functools.lru_cache(maxsize=None)
def _run(obs_dim, hidden):
    return Run(obs_dim, hidden)


@pytest.mark.parametrize("obs_dim,hidden", CASES)
def test_stored_rows_are_the_mirror_and_the_nets_saw_them(obs_dim, hidden):
    from gym_auv_amd.normalize import norm_rows
    r = _run(obs_dim, hidden)
    lib = _lib()
    O, A, LP, V, R, Dn = r.buffers
    hit = 0
    for t in range(T):
        want = norm_rows(r.obs[t].cpu().numpy(), r.table, 10.0)
        assert np.array_equal(O[t].cpu().numpy(), want), t
        hit += int((np.abs(want) == 10.0).sum())
        ev = _eval(r.fused, O[t])
        assert torch.equal(ev["mu"], r.mu[t]) and torch.equal(ev["value"], V[t]), t
        # auv_norm_rows: the same bits, without idx (also from a strided window) and with
        raw = r.obs[t]
        assert torch.equal(r.norm.normalize(raw), O[t])
        wide = torch.full((N, obs_dim + 3), 7.0, device=DEV)
        wide[:, :obs_dim] = raw
        assert torch.equal(r.norm.normalize(wide[:, :obs_dim]), O[t])
        idx = torch.as_tensor([39, 0, 17, 17, 24], dtype=torch.int64, device=DEV)
        assert torch.equal(r.norm.normalize(raw, idx=idx), O[t][idx])
    assert hit > 0 and float(Dn.sum()) > 0                  # the clip was hit, and episodes did end
    assert lib.auv_last_error() is not None


@pytest.mark.parametrize("obs_dim,hidden", CASES[:2])
def test_partials_are_the_tile_moments_of_the_raw_rows(obs_dim, hidden):
    from gym_auv_amd.normalize import slice_partials
    r = _run(obs_dim, hidden)
    assert r.norm.part_base == [0, 2] and r.norm.part_ld == 3
    part, pcnt = r.part.cpu().numpy(), r.pcnt.cpu().numpy()
    for t in range(T):
        wp, wc = slice_partials(r.obs[t].cpu().numpy(), BOUNDS)
        assert wc.tolist() == [16, 8, 16]                   # the ragged tile carries 8
        assert np.array_equal(pcnt[3 * t:3 * t + 3], wc), t
        assert np.array_equal(part[3 * t:3 * t + 3], wp), t
    # nothing is written by the flush launches
    assert torch.equal(r.part, r.part_before_flush) and torch.equal(r.pcnt, r.pcnt_before_flush)


# ------------------------------------------------------------------------------ 4. fold and return pass
@pytest.mark.parametrize("obs_dim", [186, 15])
def test_fold_is_the_mirror_and_reruns_are_bit_identical(obs_dim):
    from gym_auv_amd.normalize import fold_moments
    r = _run(obs_dim, (256, 128, 64) if obs_dim == 186 else (64, 64, 64))
    lib = _lib()
    rs = np.random.RandomState(4)
    mom0 = np.stack([np.full(obs_dim, 1e-4), np.zeros(obs_dim), np.full(obs_dim, 1e-4)], 1)
    mom1 = np.stack([np.full(obs_dim, 200.0), rs.uniform(-3, 3, obs_dim), rs.uniform(10, 5000, obs_dim)], 1)
    # the rollout's 9 slots, and 150 slots (more than a wave's 64 lanes, empty ones among them)
    part150 = torch.as_tensor(rs.standard_normal((150, 2, obs_dim)).astype(np.float32), device=DEV)
    part150[:, 1].abs_()
    pcnt150 = torch.as_tensor(rs.choice([0, 1, 8, 16], 150).astype(np.int32), device=DEV)
    for part, pcnt in ((r.part, r.pcnt), (part150, pcnt150)):
        for start in (mom0, mom1):
            want_mom, want_table = fold_moments(part.cpu().numpy(), pcnt.cpu().numpy(), start, 1e-8)
            got = []
            for rerun in range(2):
                mom = torch.as_tensor(start, device=DEV).clone()
                table = torch.zeros((obs_dim, 2), dtype=torch.float32, device=DEV)
                rc = lib.auv_norm_fold(0, _p(part), _p(pcnt), int(pcnt.numel()), obs_dim, 1e-8, _p(mom), _p(table), None)
                assert rc == 0, lib.auv_last_error()
                torch.cuda.synchronize()
                got.append((mom.cpu().numpy(), table.cpu().numpy()))
            assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
            assert np.array_equal(got[0][0], want_mom), np.abs(got[0][0] - want_mom).max()
            assert np.array_equal(got[0][1], want_table), np.abs(got[0][1] - want_table).max()


def test_return_pass_is_the_mirror_and_reruns_are_bit_identical():
    from gym_auv_amd.normalize import return_pass
    lib = _lib()
    rs = np.random.RandomState(9)
    for (Tn, Nn) in ((3, 40), (5, 200)):                    # (200: more environments than a wave's 64 lanes)
        R = (rs.standard_normal((Tn, Nn)) * 3 + 0.2).astype(np.float32)
        R[rs.uniform(size=R.shape) < 0.05] = -5000.0
        Dn = (rs.uniform(size=R.shape) < 0.25).astype(np.float32)
        Dn[0, 1], Dn[Tn - 1, 2] = 1.0, 1.0                   # done at t = 0 and at t = T - 1
        ret = np.zeros(Nn)
        rmom = np.array([1e-4, 0.0, 1e-4])
        Rd, Dd = torch.as_tensor(R, device=DEV), torch.as_tensor(Dn, device=DEV)
        for call in range(2):                               # ret carried across two calls
            want_ret, want_mom, want_R = return_pass(R, Dn, ret, rmom, 0.99, 1e-8, 10.0)
            got = []
            for rerun in range(2):
                ret_d, mom_d = torch.as_tensor(ret, device=DEV).clone(), torch.as_tensor(rmom, device=DEV).clone()
                rpart, out = torch.zeros((Nn, 2), dtype=torch.float64, device=DEV), torch.zeros_like(Rd)
                rc = lib.auv_norm_returns(0, _p(Rd), _p(Dd), _p(out), Tn, Nn, 0.99, 10.0, 1e-8, _p(ret_d), _p(rpart), _p(mom_d), 1, None)
                assert rc == 0, lib.auv_last_error()
                torch.cuda.synchronize()
                got.append((ret_d.cpu().numpy(), mom_d.cpu().numpy(), out.cpu().numpy()))
            for a, b in zip(got[0], got[1]):
                assert np.array_equal(a, b)
            assert np.array_equal(got[0][0], want_ret) and np.array_equal(got[0][1], want_mom), (got[0][1], want_mom)
            assert np.array_equal(got[0][2], want_R), np.abs(got[0][2] - want_R).max()
            # update == 0: the scaling alone, in place, nothing else written
            inplace, mom_d = Rd.clone(), torch.as_tensor(want_mom, device=DEV).clone()
            rc = lib.auv_norm_returns(0, _p(inplace), None, _p(inplace), Tn, Nn, 0.99, 10.0, 1e-8, None, None, _p(mom_d), 0, None)
            assert rc == 0, lib.auv_last_error()
            torch.cuda.synchronize()
            assert np.array_equal(inplace.cpu().numpy(), want_R) and np.array_equal(mom_d.cpu().numpy(), want_mom)
            ret, rmom = want_ret, want_mom


# ------------------------------------------------------------------------------ 5. end to end
@pytest.mark.parametrize("obs_dim,hidden", CASES[:2])
def test_end_to_end_two_rollouts_a_fold_and_training_off(obs_dim, hidden):
    from gym_auv_amd.normalize import fold_moments, norm_rows, return_pass, slice_partials
    # the same seed through the plain rollout call, directly: normalize = None is today's path
    ea, eb = _env(obs_dim), _env(obs_dim)
    fa, fb = _fused(ea, hidden), _fused(eb, hidden)
    lib = _lib()
    fa.begin_rollout(), fb.begin_rollout()
    fa.rollout(T)
    t0, g0 = (C.c_int64 * 2)(0, 0), (C.c_int64 * 2)(0, 0)
    call = lib.auv_policy_rollout_arch if fb._arch is not None else lib.auv_policy_rollout
    args = [eb._h, 2, eb._bounds_c, eb._streams_c, fb._ios] + ([C.byref(fb._arch)] if fb._arch is not None else []) + \
        [_p(eb.obs), _p(eb.reward), _p(eb.done), T, 1, t0, g0]
    assert call(*args) == 0, lib.auv_last_error()
    torch.cuda.synchronize()
    for name, x, y in zip("O A LP V R Dn".split(), fa.buffers(), fb.buffers()):
        assert torch.equal(x, y), name
    assert torch.equal(ea.obs, eb.obs) and fa._nios is None
    ea.close(), eb.close()

    env = _env(obs_dim)
    norm = _norm(env)
    fused = _fused(env, hidden, normalize=norm)
    table0 = norm.table.cpu().numpy().copy()
    mom = norm.obs_mom.cpu().numpy().copy()
    # rollout 1 on the initial table, one step per call so that the raw rows can be read in between
    raw = []
    fused.begin_rollout()
    for t in range(T):
        torch.cuda.synchronize()
        raw.append(env.obs.clone())
        fused.rollout(1, flush=(t == T - 1))
    torch.cuda.synchronize()
    O1 = fused.O.clone()
    for t in range(T):
        assert np.array_equal(O1[t].cpu().numpy(), norm_rows(raw[t].cpu().numpy(), table0, 10.0)), t
    parts = [slice_partials(x.cpu().numpy(), BOUNDS) for x in raw]
    want_mom, want_table = fold_moments(np.concatenate([p for p, _ in parts]), np.concatenate([c for _, c in parts]), mom, 1e-8)
    R_raw, Dn = fused.R.clone(), fused.Dn.clone()
    norm.fold()
    scaled = norm.returns(fused.R, fused.Dn)
    torch.cuda.synchronize()
    assert np.array_equal(norm.obs_mom.cpu().numpy(), want_mom) and np.array_equal(norm.table.cpu().numpy(), want_table)
    assert int(norm.pcnt.sum()) == 0                       # the slots are consumed
    w_ret, w_rmom, w_R = return_pass(R_raw.cpu().numpy(), Dn.cpu().numpy(), np.zeros(N), [1e-4, 0.0, 1e-4], 0.99, 1e-8, 10.0)
    assert scaled.data_ptr() == fused.R.data_ptr() and np.array_equal(fused.R.cpu().numpy(), w_R)
    assert np.array_equal(norm.ret.cpu().numpy(), w_ret) and np.array_equal(norm.ret_mom.cpu().numpy(), w_rmom)
    # rollout 2 under the folded table, as ONE call
    raw2 = env.obs.clone()
    fused.begin_rollout()
    fused.rollout(T)
    torch.cuda.synchronize()
    assert np.array_equal(fused.O[0].cpu().numpy(), norm_rows(raw2.cpu().numpy(), want_table, 10.0))
    assert not np.array_equal(want_table, table0)
    ev = _eval(fused, fused.O[T - 1])
    assert torch.equal(ev["value"], fused.V[T - 1])
    # training off: a third rollout, fold() and returns() leave every statistic as it is
    norm.fold()
    torch.cuda.synchronize()
    norm.training = False
    before = norm.state_dict()
    fused.begin_rollout()
    fused.rollout(T)
    torch.cuda.synchronize()
    R3 = fused.R.clone()
    norm.fold()
    norm.returns(fused.R, fused.Dn)
    torch.cuda.synchronize()
    after = norm.state_dict()
    for k in ("obs_mom", "ret_mom", "table", "ret"):
        assert torch.equal(before[k], after[k]), k
    _, _, w_R3 = return_pass(R3.cpu().numpy(), fused.Dn.cpu().numpy(), None, before["ret_mom"].numpy(), 0.99, 1e-8, 10.0, update=False)
    assert np.array_equal(fused.R.cpu().numpy(), w_R3)
    # predict / value on raw observations = auv_policy_eval on normalize()d rows
    from gym_auv_amd.policy import policy_eval
    rows = norm.normalize(env.obs)
    assert np.array_equal(rows.cpu().numpy(), norm_rows(env.obs.cpu().numpy(), norm.table.cpu().numpy(), 10.0))
    want = policy_eval(fused.params, obs_dim, rows, want=("action", "value"), action_map=fused.action_map, **fused._eval_kw())
    out = torch.zeros((N, 2), device=DEV)
    assert torch.equal(fused.predict(out=out), want["action"]) and torch.equal(fused.value(), want["value"])
    lp, v, mu = fused.evaluate(env.obs, fused.A[0])
    assert torch.equal(v, want["value"])
    env.close()


# ------------------------------------------------------------------------------ 6. refusals
def test_refusals_name_the_function_and_enqueue_nothing():
    from gym_auv_amd import _capi
    lib = _lib()
    r = _run(15, (64, 64, 64))
    env, fused, norm = r.env, r.fused, r.norm
    st = C.c_void_p(env._sub_streams[0].cuda_stream)
    t0, g0 = (C.c_int64 * 2)(0, 0), (C.c_int64 * 2)(0, 0)
    arch = _capi.AuvPolicyArch(64, 64, 64)
    torch.cuda.synchronize()
    keep = [x.clone() for x in (norm.part, norm.pcnt, fused.O, fused.actions, env.obs)] + [b["ctr"].clone() for b in fused.buf]

    def both(s, a=arch):
        rc = lib.auv_policy_act_norm_arch(env._h, 0, 24, C.byref(s), C.byref(a) if a is not None else None, st)
        assert rc == AUV_EINVAL and b"auv_policy_act_norm_arch" in lib.auv_last_error(), (rc, lib.auv_last_error())
        arr = (_capi.AuvPolicyNorm * 2)(s, fused._nios[1])
        rc = lib.auv_policy_rollout_norm_arch(env._h, 2, env._bounds_c, env._streams_c, arr, C.byref(a) if a is not None else None, _p(env.obs),
                                              _p(env.reward), _p(env.done), 1, 0, t0, g0)
        assert rc == AUV_EINVAL and b"auv_policy_rollout_norm_arch" in lib.auv_last_error(), (rc, lib.auv_last_error())

    def copy():
        s = _capi.AuvPolicyNorm()
        C.memmove(C.byref(s), C.byref(fused._nios[0]), C.sizeof(s))
        return s
    for field, value in (("table", None), ("table", norm.table.data_ptr() + 4), ("part", None), ("pcnt", None), ("clip_obs", 0.0),
                         ("clip_obs", -1.0), ("clip_obs", float("nan")), ("part_base", -1), ("part_base", 2), ("part_ld", 1)):
        s = copy()
        setattr(s, field, value)
        both(s)
    s = copy()
    s.io.params_bf16 = fused.params.data_ptr()
    both(s)
    both(copy(), _capi.AuvPolicyArch(96, 64, 64))           # a triple outside the list
    both(copy(), None)
    # the entries without _arch name themselves (here: a table that is NULL)
    s = copy()
    s.table = None
    rc = lib.auv_policy_act_norm(env._h, 0, 24, C.byref(s), st)
    assert rc == AUV_EINVAL and b"auv_policy_act_norm:" in lib.auv_last_error()
    # (obs_dim too wide for the LDS tile is auv_policy_act's own check, which runs first here too; only a handle whose observation has
    # thousands of columns reaches it.)  An obs_dim that is not the handle's:
    s = copy()
    s.io.obs_dim = 16
    both(s)
    # auv_norm_rows / auv_norm_fold / auv_norm_returns
    x, out = torch.zeros((N, 15), device=DEV), torch.zeros((N, 15), device=DEV)
    tb = norm.table
    for args in ((0, _p(x), None, 15, None, 10.0, _p(out), 15, N, 15, None), (0, _p(x), None, 14, _p(tb), 10.0, _p(out), 15, N, 15, None),
                 (0, _p(x), None, 15, _p(tb), 0.0, _p(out), 15, N, 15, None), (0, _p(x), None, 15, _p(tb), 10.0, _p(out), 15, -1, 15, None),
                 (0, _p(x), None, 15, C.c_void_p(tb.data_ptr() + 4), 10.0, _p(out), 15, N, 15, None), (-1, _p(x), None, 15, _p(tb), 10.0, _p(out), 15, N, 15, None),
                 (0, _p(x), None, 15, _p(tb), 10.0, _p(out), 15, N, 0, None)):
        assert lib.auv_norm_rows(*args) == AUV_EINVAL and b"auv_norm_rows" in lib.auv_last_error(), args
    mom = norm.obs_mom.clone()
    for args in ((0, None, _p(norm.pcnt), 9, 15, 1e-8, _p(mom), _p(tb), None), (0, _p(norm.part), _p(norm.pcnt), 0, 15, 1e-8, _p(mom), _p(tb), None),
                 (0, _p(norm.part), _p(norm.pcnt), 9, 15, -1.0, _p(mom), _p(tb), None), (0, _p(norm.part), _p(norm.pcnt), 9, 15, 1e-8, None, _p(tb), None)):
        assert lib.auv_norm_fold(*args) == AUV_EINVAL and b"auv_norm_fold" in lib.auv_last_error(), args
    R = torch.zeros((T, N), device=DEV)
    ret, rp, rm = torch.zeros(N, dtype=torch.float64, device=DEV), torch.zeros((N, 2), dtype=torch.float64, device=DEV), norm.ret_mom.clone()
    for args in ((0, None, _p(R), _p(R), T, N, 0.99, 10.0, 1e-8, _p(ret), _p(rp), _p(rm), 1, None),
                 (0, _p(R), _p(R), _p(R), T, N, 0.99, 10.0, 1e-8, None, _p(rp), _p(rm), 1, None),
                 (0, _p(R), _p(R), _p(R), T, N, 0.99, 0.0, 1e-8, _p(ret), _p(rp), _p(rm), 1, None),
                 (0, _p(R), _p(R), _p(R), 0, N, 0.99, 10.0, 1e-8, _p(ret), _p(rp), _p(rm), 1, None),
                 (0, _p(R), _p(R), _p(R), T, N, float("inf"), 10.0, 1e-8, _p(ret), _p(rp), _p(rm), 1, None)):
        assert lib.auv_norm_returns(*args) == AUV_EINVAL and b"auv_norm_returns" in lib.auv_last_error(), args
    torch.cuda.synchronize()
    now = [norm.part, norm.pcnt, fused.O, fused.actions, env.obs] + [b["ctr"] for b in fused.buf]
    for a, b in zip(keep, now):
        assert torch.equal(a, b)                            # nothing was enqueued
    assert float(out.abs().max()) == 0.0 and torch.equal(mom, norm.obs_mom)
