"""-m gpu: the recording launch of several steps (auv_step_multi_record / k_step_record, BatchedAuvEnv.step_multi(record=...),
AuvVecEnv.step_sequence).  Row k of a record must be, bit for bit, what the k-th of T one-step calls hands its caller -- on twin
environments, one stepped by T one-step calls (outputs collected after each), one by a single recording call -- with auto-reset
inside the launch (max_timesteps = 13: every environment ends at least once per 13 steps), odd widths and odd batch sizes, records
that are slices of larger buffers, and once against the oracle, which does not lean on the one-step path."""
import ctypes as C

import numpy as np
import pytest
import torch

from gym_auv_amd._capi import make_config
from gym_auv_amd.config import effective_reference_config
from gym_auv_amd.scenarios import moving_obstacles_world, polygon_world
from gym_auv_amd.world import build_world, pack_bank

pytestmark = pytest.mark.gpu

FIELDS = ("STATE", "LIDAR_D", "OBS64", "REWARD64", "INFO64", "NAV64", "MOVER_STATE", "NEARBY", "COLLISION", "COUNTERS", "EPISODE",
          "CULL_LIMITS", "STEP_INFO", "WORLD_IDX")
CLEAN = dict(handover_ok=1, probe_failures=0, timeouts=0, pending=0)
DEV = "cuda:0"


def _np(t):
    return t.detach().cpu().numpy()


def _env(cfg, bank, n):
    from gym_auv_amd.batched_env import BatchedAuvEnv
    return BatchedAuvEnv(cfg, bank, n, device=DEV, auto_reset=True)


def _bank(kind, n_worlds):
    if kind == "moving":
        return pack_bank([build_world(moving_obstacles_world(500 + i)) for i in range(n_worlds)])
    return pack_bank([build_world(polygon_world(700 + i, n_polygons=10, n_circles=6, n_moving=5)) for i in range(n_worlds)])


def _cfg(ns=8, nps=8, pooled=False, max_timesteps=13):
    cfg = effective_reference_config(use_lidar=True)
    cfg.vessel.n_sectors, cfg.vessel.n_sensors_per_sector = ns, nps
    cfg.vessel.sensor_use_feasibility_pooling = pooled
    cfg.episode.max_timesteps = max_timesteps
    return cfg


def _ring(slots, n, seed=12):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.rand((slots, n, 2), generator=g, device=DEV) * torch.tensor([2.0, 0.3], device=DEV) - torch.tensor([1.0, 0.15], device=DEV)


def _one_step_calls(ref, ring, t, T, k=1):
    """T one-step calls on `ref`; the stacked obs / reward / done its caller saw after each."""
    slots = ring.shape[0]
    o, r, d = [], [], []
    for j in range(T):
        if k > 1:
            ref.step_pipelined(ring[(t + j) % slots])
        else:
            ref.step(ring[(t + j) % slots])
        torch.cuda.synchronize()
        o.append(ref.obs.clone()), r.append(ref.reward.clone()), d.append(ref.done.clone())
    return torch.stack(o), torch.stack(r), torch.stack(d)


def _assert_same_state(ref, mul, where):
    assert torch.equal(ref.obs, mul.obs) and torch.equal(ref.reward, mul.reward) and torch.equal(ref.done, mul.done), where
    for f in FIELDS:
        assert torch.equal(ref.read(f), mul.read(f)), (where, f)


def _assert_record(rec, want, where, prev_obs=None, n_done_min=0):
    """rec == want bitwise; enough done flags; a row with done = 1 carries the reset observation: the twin's (that IS the
    equality) and not the row before it."""
    (o, r, d), (wo, wr, wd) = rec, want
    if o is not None:
        assert o.shape == wo.shape and torch.equal(o, wo), where
    assert torch.equal(r, wr), where
    assert torch.equal(d, wd), where
    assert int(d.sum()) >= n_done_min, (where, int(d.sum()), n_done_min)
    if o is not None:
        before = torch.cat([prev_obs[None] if prev_obs is not None else o[:1], o[:-1]])
        ended = d.bool()
        if prev_obs is None:
            ended[0] = False
        if bool(ended.any()):
            assert bool((o[ended] != before[ended]).any(dim=-1).all()), where


@pytest.mark.parametrize("kind,n,k,lengths,order", [("moving", 256, 1, (1, 2, 7, 30), "cohorts"), ("moving", 256, 1, (1, 2, 7, 30), "steps"),
                                                    ("mixed", 1024, 4, (3, 16, 29), "cohorts"), ("moving", 1000, 2, (64,), "cohorts")])
def test_record_is_the_one_step_trajectory_bitwise(kind, n, k, lengths, order):
    cfg = _cfg()
    bank = _bank(kind, 48)
    ref, mul = _env(cfg, bank, n), _env(cfg, bank, n)
    ref.reset(), mul.reset()
    if k > 1:
        ref.set_sub_batches(k, strict=True), mul.set_sub_batches(k, strict=True)
    mul.set_multi_order(order)
    slots = 16
    ring = _ring(slots, n)
    t = 0
    for rep in range(3):
        for T in lengths:
            prev = ref.obs.clone()
            want = _one_step_calls(ref, ring, t, T, k)
            rec = mul.step_multi(ring, t % slots, T, record=True)
            t += T
            torch.cuda.synchronize()
            assert rec[0].shape == (T, n, mul.obs_dim) and rec[1].shape == (T, n) and rec[2].shape == (T, n)
            assert rec[0].dtype == torch.float32 and rec[1].dtype == torch.float32 and rec[2].dtype == torch.uint8
            _assert_record(rec, want, (rep, T), prev_obs=prev, n_done_min=n if T >= 16 else 0)
            _assert_same_state(ref, mul, (rep, T))
    assert int(ref.read("COUNTERS")[:, 2].sum()) >= 3 * n
    la, lb = _np(ref.episode_log()), _np(mul.episode_log())
    np.testing.assert_array_equal(la[np.lexsort(la.T[::-1])], lb[np.lexsort(lb.T[::-1])])
    assert mul.health() == CLEAN
    ref.close(), mul.close()


@pytest.mark.parametrize("n", [251, 1001])
@pytest.mark.parametrize("pooled", [True, False])
def test_odd_batch_sizes_and_widths_into_an_odd_row_slice(n, pooled):
    """obs_dim 15 (pooled: nothing is stored in pairs) and 70 (the tail stores float pairs: a record row starts an even number of
    floats further on); the record is buf[1:21] of a larger buffer, so with odd n and odd obs_dim it starts 4 bytes off an 8-byte
    boundary.  Slices that are not a multiple of 64 environments also take the step-major order."""
    cfg = _cfg(9, 8, True) if pooled else _cfg(8, 8, False)
    bank = _bank("mixed", 48)
    ref, mul = _env(cfg, bank, n), _env(cfg, bank, n)
    assert mul.obs_dim == (15 if pooled else 70)
    ref.reset(), mul.reset()
    ring = _ring(16, n, 5)
    T = 20
    bo = torch.full((23, n, mul.obs_dim), 7.0, device=DEV)
    br = torch.full((23, n), 7.0, device=DEV)
    bd = torch.full((23, n), 7, dtype=torch.uint8, device=DEV)
    t = 0
    for rep in range(2):
        prev = ref.obs.clone()
        want = _one_step_calls(ref, ring, t, T)
        torch.cuda.synchronize()
        rec = mul.step_multi(ring, t % 16, T, record=(bo[1:21], br[1:21], bd[1:21]))
        t += T
        torch.cuda.synchronize()
        assert rec[0].data_ptr() == bo[1].data_ptr()
        _assert_record(rec, want, rep, prev_obs=prev, n_done_min=n)
        _assert_same_state(ref, mul, rep)
        # nothing outside the slice was touched
        for b in (bo, br, bd):
            assert bool((b[0] == 7).all()) and bool((b[21:] == 7).all())
    assert mul.health() == CLEAN
    ref.close(), mul.close()


def test_reward_and_done_only():
    n, T = 320, 20
    cfg = _cfg()
    bank = _bank("moving", 48)
    ref, mul = _env(cfg, bank, n), _env(cfg, bank, n)
    ref.reset(), mul.reset()
    ring = _ring(16, n, 3)
    for rep in range(2):
        want = _one_step_calls(ref, ring, rep * T, T)
        rec = mul.step_multi(ring, (rep * T) % 16, T, record="reward")
        torch.cuda.synchronize()
        assert rec[0] is None
        _assert_record(rec, want, rep, n_done_min=n)
        _assert_same_state(ref, mul, rep)                          # (env.obs: the twin's last observation)
    assert mul.health() == CLEAN
    ref.close(), mul.close()


def test_two_calls_into_the_halves_of_a_buffer_equal_one_call():
    n = 512
    cfg = _cfg()
    bank = _bank("mixed", 48)
    a, b = _env(cfg, bank, n), _env(cfg, bank, n)
    a.reset(), b.reset()
    ring = _ring(32, n, 9)
    bufa = (torch.zeros((32, n, a.obs_dim), device=DEV), torch.zeros((32, n), device=DEV), torch.zeros((32, n), dtype=torch.uint8, device=DEV))
    bufb = tuple(torch.zeros_like(x) for x in bufa)
    torch.cuda.synchronize()
    a.step_multi(ring, 0, 16, record=tuple(x[:16] for x in bufa))
    a.step_multi(ring, 16, 16, record=tuple(x[16:] for x in bufa))
    b.step_multi(ring, 0, 32, record=bufb)
    torch.cuda.synchronize()
    for x, y in zip(bufa, bufb):
        assert torch.equal(x, y)
    assert int(bufb[2].sum()) >= 2 * n
    _assert_same_state(a, b, "halves")
    assert a.health() == CLEAN and b.health() == CLEAN
    a.close(), b.close()


def test_action_repeat_is_a_ring_of_one_slot():
    n, T = 256, 8
    cfg = _cfg()
    bank = _bank("moving", 48)
    ref, mul = _env(cfg, bank, n), _env(cfg, bank, n)
    ref.reset(), mul.reset()
    ring = _ring(1, n, 4)
    for rep in range(3):
        prev = ref.obs.clone()
        want = _one_step_calls(ref, ring, 0, T)
        rec = mul.step_multi(ring, 0, T, record=True)
        torch.cuda.synchronize()
        _assert_record(rec, want, rep, prev_obs=prev)
        _assert_same_state(ref, mul, rep)
    assert int(mul.read("COUNTERS")[:, 2].sum()) >= n               # episodes ended inside the repeats
    assert mul.health() == CLEAN
    ref.close(), mul.close()


def test_recorded_reward_and_done_against_the_oracle():
    """1024 environments, 40 steps in ONE recording launch, polygons and movers; a 64-environment subset stepped by the oracle with
    the same actions, following the batch's world rotation (tests/test_gpu_fullsize.py), reward within that file's tolerance and
    done exact.  The only test here that does not lean on the one-step path."""
    from oracle.pyoracle import Oracle
    n, T = 1024, 40
    cfg = _cfg(16, 16, False, max_timesteps=23)
    bank = pack_bank([build_world(polygon_world(3000 + i, 10, n_circles=20, n_moving=17)) for i in range(96)])
    W = int(bank["n_worlds"])
    env = _env(cfg, bank, n)
    rs = np.random.RandomState(11)
    sub = np.sort(rs.choice(n, 64, replace=False))
    ora = Oracle(make_config(cfg, auto_reset=False), len(sub), bank)
    w_now = (sub % W).astype(np.int32)
    env.reset(), ora.reset(world_idx=w_now)
    a_np = rs.uniform([-1, -0.15], [1, 0.15], (T, n, 2))
    a_np[..., 0] = np.abs(a_np[..., 0]) ** 0.3
    ring = torch.as_tensor(a_np, device=DEV).contiguous()
    obs, rew, done = env.step_multi(ring, 0, T, record=True)
    torch.cuda.synchronize()
    g_rew, g_done, g_obs = _np(rew), _np(done), _np(obs)
    n_done = 0
    for t in range(T):
        o_obs, o_rew, o_done = ora.step(a_np[t][sub])
        np.testing.assert_array_equal(g_done[t][sub], o_done, err_msg="done step %d" % t)
        np.testing.assert_allclose(g_rew[t][sub], o_rew, rtol=1e-6, atol=1e-4, err_msg="reward step %d" % t)
        n_done += int(o_done.sum())
        if o_done.any():                                           # the oracle's subset follows the batch's world rotation
            w_now = np.where(o_done > 0, (w_now + n) % W, w_now).astype(np.int32)
            o_obs_r = ora.reset(mask=o_done, world_idx=w_now)
            o_obs = np.where(o_done[:, None] > 0, o_obs_r, o_obs)
        np.testing.assert_allclose(g_obs[t][sub], o_obs, rtol=0, atol=1e-6, err_msg="obs step %d" % t)
    assert n_done >= 64
    assert env.health() == CLEAN
    env.close()


def test_refusals_launch_nothing():
    from gym_auv_amd import _capi
    from gym_auv_amd.devgen import FreshWorlds
    n = 128
    cfg = _cfg()
    ring = _ring(4, n, 2)
    env = _env(cfg, FreshWorlds(seed=1, batch_cap=8), 16)
    with pytest.raises(RuntimeError, match="fresh world"):
        env.step_multi(_ring(4, 16, 2), 0, 2, record=True)
    assert env.health()["timeouts"] == 0
    env.close()
    bank = _bank("moving", 8)
    env, twin = _env(cfg, bank, n), _env(cfg, bank, n)
    assert env.obs_dim == 70
    env.reset(), twin.reset()
    env.step_multi(ring, 0, 3, record=True), twin.step_multi(ring, 0, 3, record=True)
    torch.cuda.synchronize()
    env.set_step_mode("side_by_side")
    with pytest.raises(RuntimeError, match="one-launch"):
        env.step_multi(ring, 0, 2, record=True)
    env.set_step_mode("auto")
    for T in (0, 1025):
        with pytest.raises(RuntimeError, match="n_steps"):
            env.step_multi(ring, 0, T, record="reward")
    good = (torch.zeros((2, n, 70), device=DEV), torch.zeros((2, n), device=DEV), torch.zeros((2, n), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        env.step_multi(ring, 0, 2, record=(good[0], None, good[2]))                                  # a missing reward record
    with pytest.raises(ValueError):
        env.step_multi(ring, 0, 2, record=(good[0][:, :, :69], good[1], good[2]))                    # wrong shape (and not contiguous)
    with pytest.raises(ValueError):
        env.step_multi(ring, 0, 3, record=good)                                                      # two rows for three steps
    with pytest.raises(ValueError):
        env.step_multi(ring, 0, 2, record=(good[0], good[1].double(), good[2]))                      # wrong dtype
    with pytest.raises(ValueError):
        env.step_multi(ring, 0, 2, record=(good[0].cpu(), good[1], good[2]))                         # wrong device
    with pytest.raises(ValueError):
        env.step_multi(ring, 0, 2, record="obs")
    # through the C ABI (AUV_EINVAL = -1): a NULL reward / done record, and an obs_rec 4 but not 8 bytes aligned at an even obs_dim
    lib = _capi.load_library()
    big = torch.zeros((2 * n * 70 + 2,), device=DEV)
    assert big.data_ptr() % 8 == 0

    def call(obs_rec, reward_rec, done_rec):
        return lib.auv_step_multi_record(env._h, env.sub_batches, env._bounds_c, env._streams_c, C.c_void_p(ring.data_ptr()), _capi.AUV_F32,
                                         4, 0, 2, C.c_void_p(env.obs.data_ptr()), C.c_void_p(env.reward.data_ptr()), C.c_void_p(env.done.data_ptr()),
                                         obs_rec, reward_rec, done_rec)
    rr, dr = C.c_void_p(good[1].data_ptr()), C.c_void_p(good[2].data_ptr())
    assert call(C.c_void_p(big.data_ptr()), None, dr) == -1
    assert call(C.c_void_p(big.data_ptr()), rr, None) == -1
    assert call(C.c_void_p(big.data_ptr() + 4), rr, dr) == -1
    assert b"aligned" in lib.auv_last_error()
    torch.cuda.synchronize()
    _assert_same_state(env, twin, "after the refusals")
    assert all(bool((g == 0).all()) for g in good) and bool((big == 0).all())
    # ... and no step number was spent: the two go on in lockstep
    ra, rb = env.step_multi(ring, 3, 20, record=True), twin.step_multi(ring, 3, 20, record=True)
    torch.cuda.synchronize()
    for x, y in zip(ra, rb):
        assert torch.equal(x, y)
    _assert_same_state(env, twin, "after the refusals, 20 steps on")
    assert env.health() == CLEAN and twin.health() == CLEAN
    env.close(), twin.close()


def test_recording_launch_past_the_dispatch_limit_is_refused():
    """32 768 environments x 1024 steps (tests/test_gpu_multi_geometry.py), reward and done records only: 134 MB + 34 MB."""
    n = 32768
    cfg = _cfg()
    bank = _bank("moving", 16)
    env, twin = _env(cfg, bank, n), _env(cfg, bank, n)
    env.reset(), twin.reset()
    ring = _ring(8, n, 23)
    for order in ("cohorts", "steps"):
        env.set_multi_order(order)
        with pytest.raises(RuntimeError, match="work-items"):
            env.step_multi(ring, 0, 1024, record="reward")
    env.set_multi_order("cohorts")
    torch.cuda.synchronize()
    _assert_same_state(env, twin, "after the refusal")
    ra, rb = env.step_multi(ring, 0, 5, record="reward"), twin.step_multi(ring, 0, 5, record="reward")
    torch.cuda.synchronize()
    assert torch.equal(ra[1], rb[1]) and torch.equal(ra[2], rb[2])
    _assert_same_state(env, twin, "5 steps on")
    assert env.health() == CLEAN and twin.health() == CLEAN
    env.close(), twin.close()


@pytest.mark.parametrize("dict_obs", [False, True])
def test_vec_env_step_sequence_equals_step_calls(dict_obs):
    from gym_auv_amd.vec_env import AuvVecEnv
    n = 64
    cfg = effective_reference_config(use_lidar=True)
    cfg.vessel.n_sectors, cfg.vessel.n_sensors_per_sector = 8, 8
    cfg.episode.max_timesteps = 5
    if dict_obs:
        cfg.vessel.use_dict_observation = True
    worlds = [build_world(moving_obstacles_world(300 + i) if i % 2 == 0 else polygon_world(300 + i, 12, n_circles=4, n_moving=3))
              for i in range(2 * n)]
    a, b = AuvVecEnv(cfg, worlds, n), AuvVecEnv(cfg, worlds, n)
    rs = np.random.RandomState(3)

    def same(x, y, where):
        if dict_obs:
            assert set(x) == set(y) == {"proprioceptive", "lidar"}
            for key in x:
                assert x[key].dtype == y[key].dtype and np.array_equal(x[key], y[key]), (where, key)
        else:
            assert x.dtype == y.dtype and np.array_equal(x, y), where

    oa, ob = a.reset(), b.reset()
    same(oa, ob, "reset")
    n_done = 0
    for T in (1, 12, 1):
        acts = rs.uniform([-1, -0.15], [1, 0.15], (T, n, 2)).astype(np.float32)
        so, sr, sd = b.step_sequence(acts)
        assert sr.shape == (T, n) and sr.dtype == np.float32 and sd.shape == (T, n) and sd.dtype == bool
        for t in range(T):
            o, r, d, infos = a.step(acts[t])
            same(o, {key: v[t] for key, v in so.items()} if dict_obs else so[t], (T, t))
            assert np.array_equal(r, sr[t]) and np.array_equal(d, sd[t]), (T, t)
            n_done += int(d.sum())
        for f in FIELDS:
            assert torch.equal(a.env.read(f), b.env.read(f)), (T, f)
    assert n_done >= 2 * n
    assert a.get_attr("total_t_steps") == b.get_attr("total_t_steps")
    with pytest.raises(ValueError):
        b.step_sequence(np.zeros((3, n - 1, 2), dtype=np.float32))
    assert a.env.health() == CLEAN and b.env.health() == CLEAN
    a.close(), b.close()
