"""-m gpu: the closed-loop launch of several steps (auv_step_feedback / k_step_feedback, BatchedAuvEnv.step_feedback).

The reference in every test is T one-step step() calls on a twin environment: after each step the host reads OBS64 through
auv_read, forms the action with feedback.affine_action (NumPy fp64, the law's association) and passes it as an fp64 action.
Compared bit for bit: every step's obs / reward / done record, the action record, the final state, counters, INFO64 rows and
episode-log rows -- at the smallest shapes at which the hand-over of the action can go wrong:

  * 256 environments, one chain: four cohorts, the cohort-pipelined order; 20 and 64: step-major (20: ragged, idle groups)
  * T = 1: "step 0 reads the arrays" alone; T = 2: one hand-over; T = 5: hand-overs of hand-overs
  * max_timesteps = 3, T = 8: every environment is restored at least twice inside the launch, the action after each restore comes
    from the reset row
  * T = 30 crosses the nearby-mask refresh (every 25 vessel steps)
  * two and four chains, one slice ragged: (64, 192) and four 64s
  * gains with columns 0..6 = 0 and column 7 = 1: the open-loop recording launch
  * no ring; the feasibility-pooled configuration (the float row and OBS64's stride differ); the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from gym_auv_amd.config import effective_reference_config
from gym_auv_amd.feedback import affine_action, los_gains
from gym_auv_amd.scenarios import moving_obstacles_world, polygon_world
from gym_auv_amd.world import build_world, pack_bank

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FIELDS = ("STATE", "LIDAR_D", "OBS64", "REWARD64", "INFO64", "NAV64", "MOVER_STATE", "NEARBY", "COLLISION", "COUNTERS", "EPISODE",
          "CULL_LIMITS", "STEP_INFO", "WORLD_IDX")
CLEAN = dict(handover_ok=1, probe_failures=0, timeouts=0, pending=0)
_BANKS = {}


def _np(t):
    return t.detach().cpu().numpy()


def _bank(kind):
    """Built once per kind and shared (read only)."""
    if kind not in _BANKS:
        if kind == "moving":
            worlds = [build_world(moving_obstacles_world(500 + i)) for i in range(8)]
        elif kind == "mixed":
            worlds = [build_world(polygon_world(700 + i, n_polygons=10, n_circles=6, n_moving=5)) for i in range(8)]
        else:
            assert kind == "k128"
            worlds = [build_world(moving_obstacles_world(1100 + i, n_moving=17, n_static=111)) for i in range(2)]
        _BANKS[kind] = pack_bank(worlds)
    return _BANKS[kind]


def _cfg(ns=1, nps=8, pooled=False, max_timesteps=10000):
    cfg = effective_reference_config(use_lidar=True)
    cfg.vessel.n_sectors, cfg.vessel.n_sensors_per_sector = ns, nps
    cfg.vessel.sensor_use_feasibility_pooling = pooled
    cfg.episode.max_timesteps = max_timesteps
    return cfg


def _twins(cfg, bank, n):
    import warnings
    from gym_auv_amd.batched_env import BatchedAuvEnv
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # (fewer worlds than environments: an episode restarts in its own world)
        ref, mul = (BatchedAuvEnv(cfg, bank, n, device=DEV, auto_reset=True) for _ in range(2))
    ref.reset(), mul.reset()
    return ref, mul


def _ring(slots, n, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.rand((slots, n, 2), generator=g, device=DEV) * torch.tensor([2.0, 0.3], device=DEV) - torch.tensor([1.0, 0.15], device=DEV)


def _gains(n, seed, scale=1.5):
    """Per-environment random gains of moderate size with column 7 = 1 (a residual on the ring)."""
    g = np.random.RandomState(seed).normal(0.0, scale, (n, 2, 8))
    g[:, :, 7] = 1.0
    return g


def _reference(ref, gains, ring, t0, T):
    """T one-step calls on `ref`, each fed by the host mirror; the stacked obs / reward / done / actions its caller saw."""
    o, r, d, a = [], [], [], []
    for j in range(T):
        x = _np(ref.read("OBS64"))[:, :6]
        act = affine_action(x, gains, None if ring is None else _np(ring[(t0 + j) % ring.shape[0]]))
        ref.step(torch.as_tensor(act, device=DEV))
        torch.cuda.synchronize()
        o.append(ref.obs.clone()), r.append(ref.reward.clone()), d.append(ref.done.clone()), a.append(act)
    return torch.stack(o), torch.stack(r), torch.stack(d), np.stack(a)


def _assert_same_state(ref, mul, where):
    torch.cuda.synchronize()
    assert torch.equal(ref.obs, mul.obs) and torch.equal(ref.reward, mul.reward) and torch.equal(ref.done, mul.done), where
    for f in FIELDS:
        assert torch.equal(ref.read(f), mul.read(f)), (where, f)


def _assert_same_log(ref, mul):
    la, lb = _np(ref.episode_log()), _np(mul.episode_log())
    np.testing.assert_array_equal(la[np.lexsort(la.T[::-1])], lb[np.lexsort(lb.T[::-1])])
    return len(la)


def _check_launch(ref, mul, gains, ring, t0, T, where, record=True):
    want = _reference(ref, gains, ring, t0, T)
    rec, act = mul.step_feedback(torch.as_tensor(gains, device=DEV), T, ring=ring, first_slot=0 if ring is None else t0 % ring.shape[0],
                                 record=record, record_actions=True)
    torch.cuda.synchronize()
    if record is True:
        assert rec[0].shape == (T, mul.n_envs, mul.obs_dim) and torch.equal(rec[0], want[0]), (where, "obs record")
    else:
        assert rec[0] is None
    assert torch.equal(rec[1], want[1]), (where, "reward record")
    assert torch.equal(rec[2], want[2]), (where, "done record")
    assert act.shape == (T, mul.n_envs, 2) and act.dtype == torch.float64
    assert np.array_equal(_np(act).view(np.uint64), want[3].view(np.uint64)), (where, "action record")
    _assert_same_state(ref, mul, where)
    return want


def test_cohort_order_random_gains_hit_both_clips():
    n, T = 256, 5
    ref, mul = _twins(_cfg(), _bank("moving"), n)
    gains, ring = _gains(n, 1), _ring(8, n, 31)
    acts = []
    for rep in range(2):
        acts.append(_check_launch(ref, mul, gains, ring, rep * T, T, rep)[3])
    a = np.concatenate(acts)
    # both clips of the action range (thrust [0, 1], rudder [-1, 1]) are hit in some environments
    assert (a[..., 0] < 0).any() and (a[..., 0] > 1).any() and (a[..., 1] < -1).any() and (a[..., 1] > 1).any()
    _assert_same_log(ref, mul)
    assert mul.health() == CLEAN
    ref.close(), mul.close()


@pytest.mark.parametrize("n", [20, 64])
def test_step_major_order_one_two_and_five_steps(n):
    ref, mul = _twins(_cfg(), _bank("moving"), n)
    gains, ring = _gains(n, 2), _ring(4, n, 32)
    t = 0
    for T in (1, 2, 5, 1):
        _check_launch(ref, mul, gains, ring, t, T, (n, T))
        t += T
    assert mul.health() == CLEAN
    ref.close(), mul.close()


def test_resets_inside_the_launch_take_the_action_from_the_reset_row():
    n, T = 64, 8
    ref, mul = _twins(_cfg(max_timesteps=3), _bank("moving"), n)
    gains, ring = _gains(n, 3), _ring(8, n, 33)
    want = _check_launch(ref, mul, gains, ring, 0, T, "resets")
    assert int(want[2].sum(dim=0).min()) >= 2                      # the reference really restores every environment twice
    assert int(ref.read("COUNTERS")[:, 2].min()) >= 2
    assert _assert_same_log(ref, mul) >= 2 * n
    _check_launch(ref, mul, gains, ring, T, 3, "resets, 3 steps on")
    assert mul.health() == CLEAN
    ref.close(), mul.close()


def test_nearby_mask_refresh_crossed():
    n, T = 64, 30
    ref, mul = _twins(_cfg(), _bank("mixed"), n)
    _check_launch(ref, mul, _gains(n, 4, 0.5), _ring(8, n, 34), 0, T, "T30", record="reward")
    assert int(ref.read("COUNTERS")[:, 1].max()) >= 26
    assert mul.health() == CLEAN
    ref.close(), mul.close()


@pytest.mark.parametrize("bounds", [(0, 64, 256), (0, 64, 128, 192, 256)])
def test_chains_and_a_ragged_slice(bounds):
    n, T = 256, 5
    ref, mul = _twins(_cfg(), _bank("moving"), n)
    k = len(bounds) - 1
    mul.set_sub_batches(k, strict=True)
    # (set_sub_batches cuts equal slices: the slices under test are put in their place)
    mul._slices = [(bounds[i], bounds[i + 1] - bounds[i]) for i in range(k)]
    mul._bounds_c = (C.c_int32 * (k + 1))(*bounds)
    gains, ring = _gains(n, 5), _ring(8, n, 35)
    for rep in range(2):
        _check_launch(ref, mul, gains, ring, rep * T, T, (bounds, rep))
    assert mul.health() == CLEAN
    ref.close(), mul.close()


def test_identity_gains_are_the_open_loop_recording_launch():
    n, T = 256, 5
    ref, mul = _twins(_cfg(max_timesteps=7), _bank("moving"), n)
    gains = torch.zeros((2, 8), dtype=torch.float64, device=DEV)
    gains[:, 7] = 1.0
    ring = _ring(8, n, 36)
    for rep in range(2):
        want = ref.step_multi(ring, (rep * T) % 8, T, record=True)
        got, act = mul.step_feedback(gains, T, ring=ring, first_slot=(rep * T) % 8, record=True, record_actions=True)
        torch.cuda.synchronize()
        for x, y in zip(got, want):
            assert torch.equal(x, y), rep
        slots = [(rep * T + j) % 8 for j in range(T)]
        assert torch.equal(act, ring[slots].double())
        _assert_same_state(ref, mul, rep)
    assert int(ref.read("COUNTERS")[:, 2].min()) >= 1
    _assert_same_log(ref, mul)
    assert mul.health() == CLEAN
    ref.close(), mul.close()


def test_no_ring_line_of_sight_autopilot_closes_the_loop():
    n, T = 64, 6
    ref, mul = _twins(_cfg(), _bank("moving"), n)
    gains = np.broadcast_to(los_gains(0.7, 0.8, 0.4, 0.5), (n, 2, 8)).copy()
    want = _check_launch(ref, mul, gains, None, 0, T, "los")
    assert np.all(want[3][..., 0] == 0.7)
    # the rudder follows the observation: not constant over the steps of ONE launch
    assert (np.ptp(want[3][..., 1], axis=0) > 0).all()
    # ... also through the [2, 8] form, with nothing recorded
    ref2 = _reference(ref, gains, None, 0, 2)
    assert mul.step_feedback(torch.as_tensor(los_gains(0.7, 0.8, 0.4, 0.5), device=DEV), 2) is None
    _assert_same_state(ref, mul, "los, [2, 8] gains, no record")
    assert ref2[0].shape[0] == 2
    assert mul.health() == CLEAN
    ref.close(), mul.close()


def test_feasibility_pooled_configuration():
    n, T = 64, 5
    ref, mul = _twins(_cfg(9, 8, pooled=True, max_timesteps=4), _bank("mixed"), n)
    assert mul.obs_dim == 15 and mul.n_sensors == 72             # the float row and OBS64's stride differ
    _check_launch(ref, mul, _gains(n, 7), _ring(8, n, 37), 0, T, "pooled")
    assert mul.health() == CLEAN
    ref.close(), mul.close()


def test_refusals_return_einval_and_launch_nothing():
    from gym_auv_amd import _capi
    from gym_auv_amd.batched_env import BatchedAuvEnv
    from gym_auv_amd.devgen import FreshWorlds
    lib = _capi.load_library()
    EINVAL = -1

    def call(env, gains, T=2):
        if env._slices is None:
            env.set_sub_batches(1)
        return lib.auv_step_feedback(env._h, env.sub_batches, env._bounds_c, env._streams_c, None if gains is None else C.c_void_p(gains.data_ptr()),
                                     None, _capi.AUV_F32, 1, 0, T, C.c_void_p(env.obs.data_ptr()), C.c_void_p(env.reward.data_ptr()),
                                     C.c_void_p(env.done.data_ptr()), None, None, None, None)

    def snapshot(env):
        torch.cuda.synchronize()
        return [env.read(f).clone() for f in ("STATE", "COUNTERS", "OBS64", "INFO64")]

    def unchanged(env, before):
        return all(torch.equal(x, y) for x, y in zip(before, snapshot(env)))

    # a fresh world per reset
    env = BatchedAuvEnv(_cfg(), FreshWorlds(seed=1, batch_cap=8), 16, device=DEV, auto_reset=True)
    g16 = torch.zeros((16, 2, 8), dtype=torch.float64, device=DEV)
    before = snapshot(env)
    assert call(env, g16) == EINVAL and b"fresh world" in lib.auv_last_error()
    assert unchanged(env, before) and env.health()["timeouts"] == 0
    env.close()
    # more than 64 obstacles per world
    n = 64
    ref, mul = _twins(_cfg(), _bank("k128"), n)
    g = torch.as_tensor(_gains(n, 8), device=DEV)
    assert call(mul, g) == EINVAL and b"more than 64 obstacles" in lib.auv_last_error()
    _assert_same_state(ref, mul, "k128")
    ref.close(), mul.close()
    # NULL and misaligned gains; the step number is not spent: the twins go on in lockstep
    ref, mul = _twins(_cfg(), _bank("moving"), n)
    assert call(mul, None) == EINVAL and b"gains" in lib.auv_last_error()
    odd = torch.zeros((n * 16 * 8 + 8,), dtype=torch.uint8, device=DEV)[4:]
    assert odd.data_ptr() % 8 == 4 and call(mul, odd) == EINVAL
    for T in (0, 1025):
        assert call(mul, g, T) == EINVAL
    _assert_same_state(ref, mul, "NULL gains")
    _check_launch(ref, mul, _np(g), None, 0, 3, "after the refusals")
    with pytest.raises(ValueError):
        mul.step_feedback(g.float(), 2)
    with pytest.raises(ValueError):
        mul.step_feedback(g[:, :, :7], 2)
    assert mul.health() == CLEAN
    ref.close(), mul.close()
