"""-m gpu: the closed-loop launch with LiDAR sector inputs in its law (auv_step_feedback_sectors / k_step_sector_feedback,
BatchedAuvEnv.step_feedback(..., sector_gains=)).

Every parity case is a pair of twin environments.  The reference twin makes T one-step step() calls: after each step the host
reads OBS64 through auv_read, forms the action with feedback.sector_action (NumPy fp64, the law's association) and passes it as an
fp64 action.  The other twin makes ONE step_feedback(..., sector_gains=, record=True, record_actions=True) call.  Compared bit for
bit: every step's obs / reward / done record, the action record (as uint64), env.obs / reward / done, every field
tests/test_gpu_feedback.py compares, the episode log; health() clean.  Against a vacuous pass every parity case asserts, from the
reference twin's rows, that in some step at least one environment in eight has a non-zero sector input and that some
environment's action differs from feedback.affine_action's on the same row (banks and seeds were chosen with the CPU oracle's
rollout: the `mixed` and `moving` banks have returns in the reset rows already).

The smallest shapes at which the new loads can go wrong:
  * 64 environments (one cohort), 192 (the smallest slice the default order pipelines), 20 (step-major, a ragged group of eight)
  * T = 1: step 0 forms the law from the arrays alone; T = 2: one hand-over; T = 5
  * plain 4 x 8: only the first group sum carries sectors (w_j is all padding); plain 9 x 20: an uneven partition, sector 8 in the
    second group sum, ranges wider than one 64-beam pass of the sweep's stores; pooled 9 x 20: the float row and OBS64's stride differ
  * max_timesteps = 3, T = 8: every environment is restored at least twice inside the launch (the columns come from the reset row)
  * T = 30 on the `mixed` bank, across the nearby refresh; chains (0, 64, 256) and four 64s; a residual ring and no ring
  * caller-given bounds K = 3, b = (2, 2, 5, 8): an empty first sector, sensors left out at both ends
  * zero sector gains against the existing step_feedback; the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from gym_auv_amd.config import effective_reference_config
from gym_auv_amd.feedback import affine_action, default_sector_bounds, sector_action, sector_inputs
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
    """Built once per kind and shared (read only); the banks of tests/test_gpu_feedback.py."""
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


def _cfg(ns=4, nps=8, pooled=False, max_timesteps=10000, lidar=True):
    cfg = effective_reference_config(use_lidar=lidar)
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


def _gains(n, seed, scale=1.5, ring=True):
    """Per-environment random gains of moderate size; column 7 = 1 (a residual on the ring) or 0 (no ring)."""
    g = np.random.RandomState(seed).normal(0.0, scale, (n, 2, 8))
    g[:, :, 7] = 1.0 if ring else 0.0
    return g


def _sgains(n, seed, scale=1.0):
    return np.random.RandomState(1000 + seed).normal(0.0, scale, (n, 2, 16))


class _Seen:
    """What the reference twin's rows show over a case: the largest share of environments with a non-zero sector input in one
    step, and whether any action differed from the law without sectors."""

    def __init__(self):
        self.share, self.differs = 0.0, False

    def look(self, x, z, a, gains, ring_row):
        self.share = max(self.share, float((z != 0).any(axis=1).mean()))
        self.differs = self.differs or bool((a != affine_action(x, gains, ring_row)).any())

    def check(self, where):
        print(where, "largest share of environments with a non-zero sector input in one step: %.3f; an action differs: %s" % (self.share, self.differs))
        assert self.share >= 1.0 / 8.0, (where, "sector inputs non-zero in too few environments", self.share)
        assert self.differs, (where, "no action differs from affine_action's")


def _reference(ref, gains, sgains, bounds, ring, t0, T, seen):
    """T one-step calls on `ref`, each fed by the host mirror; the stacked obs / reward / done / actions its caller saw."""
    L = ref.n_sectors if ref.n_sectors else ref.n_sensors
    o, r, d, a = [], [], [], []
    for j in range(T):
        x = _np(ref.read("OBS64"))[:, :6 + L]
        ring_row = None if ring is None else _np(ring[(t0 + j) % ring.shape[0]])
        act = sector_action(x, gains, sgains, bounds, ring_row)
        seen.look(x, sector_inputs(x, bounds), act, gains, ring_row)
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


def _check_launch(ref, mul, gains, sgains, ring, t0, T, where, seen, record=True, bounds=None):
    b = default_sector_bounds(ref.config) if bounds is None else np.asarray(bounds, dtype=np.int32)
    want = _reference(ref, gains, sgains, b, ring, t0, T, seen)
    rec, act = mul.step_feedback(torch.as_tensor(gains, device=DEV), T, ring=ring, first_slot=0 if ring is None else t0 % ring.shape[0],
                                 record=record, record_actions=True, sector_gains=torch.as_tensor(sgains, device=DEV), sector_bounds=bounds)
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


def _end(ref, mul, seen, where):
    seen.check(where)
    _assert_same_log(ref, mul)
    assert mul.health() == CLEAN
    ref.close(), mul.close()


@pytest.mark.parametrize("n", [20, 64])
@pytest.mark.parametrize("T", [1, 2, 5])
def test_plain_4x8_one_two_and_five_steps(n, T):
    """n = 20: step-major, a ragged group of eight; n = 64: one cohort.  4 x 8: w_j is all padding.  Every T from a fresh reset, so
    that T = 1 is `step 0 from the arrays` alone."""
    ref, mul = _twins(_cfg(4, 8), _bank("moving"), n)
    seen = _Seen()
    gains, sg, ring = _gains(n, 2), _sgains(n, 2), _ring(4, n, 32)
    _check_launch(ref, mul, gains, sg, ring, 0, T, (n, T), seen)
    _check_launch(ref, mul, gains, sg, ring, T, 1, (n, T, "one more"), seen)
    _end(ref, mul, seen, (n, T))


def test_plain_9x20_pipelined_slice_of_192():
    """The reference's own partition (uneven; sector 8 in the second group sum; ranges of up to 54 beams), the smallest slice the
    default order pipelines."""
    n, T = 192, 5
    ref, mul = _twins(_cfg(9, 20), _bank("mixed"), n)
    assert np.diff(default_sector_bounds(ref.config)).max() > 48
    seen = _Seen()
    gains, sg, ring = _gains(n, 1), _sgains(n, 1), _ring(8, n, 31)
    for rep in range(2):
        _check_launch(ref, mul, gains, sg, ring, rep * T, T, rep, seen)
    _end(ref, mul, seen, "9x20")


def test_feasibility_pooled_9x20():
    n, T = 64, 5
    ref, mul = _twins(_cfg(9, 20, pooled=True, max_timesteps=4), _bank("mixed"), n)
    assert mul.obs_dim == 15 and mul.n_sensors == 180 and mul.n_sectors == 9       # the float row and OBS64's stride differ
    assert default_sector_bounds(mul.config).tolist() == list(range(10))
    seen = _Seen()
    _check_launch(ref, mul, _gains(n, 7), _sgains(n, 7), _ring(8, n, 37), 0, T, "pooled", seen)
    _end(ref, mul, seen, "pooled")


def test_resets_inside_the_launch_take_the_columns_from_the_reset_row():
    n, T = 64, 8
    ref, mul = _twins(_cfg(4, 8, max_timesteps=3), _bank("moving"), n)
    seen = _Seen()
    gains, sg, ring = _gains(n, 3), _sgains(n, 3), _ring(8, n, 33)
    want = _check_launch(ref, mul, gains, sg, ring, 0, T, "resets", seen)
    assert int(want[2].sum(dim=0).min()) >= 2                      # the reference really restores every environment twice
    assert int(ref.read("COUNTERS")[:, 2].min()) >= 2
    assert _assert_same_log(ref, mul) >= 2 * n
    _check_launch(ref, mul, gains, sg, ring, T, 3, "resets, 3 steps on", seen)
    _end(ref, mul, seen, "resets")


def test_nearby_mask_refresh_crossed_no_ring():
    n, T = 64, 30
    ref, mul = _twins(_cfg(4, 8), _bank("mixed"), n)
    seen = _Seen()
    _check_launch(ref, mul, _gains(n, 4, 0.5, ring=False), _sgains(n, 4, 0.5), None, 0, T, "T30", seen, record="reward")
    assert int(ref.read("COUNTERS")[:, 1].max()) >= 26
    _end(ref, mul, seen, "T30")


@pytest.mark.parametrize("bounds", [(0, 64, 256), (0, 64, 128, 192, 256)])
def test_chains_and_a_ragged_slice(bounds):
    n, T = 256, 5
    ref, mul = _twins(_cfg(4, 8), _bank("moving"), n)
    k = len(bounds) - 1
    mul.set_sub_batches(k, strict=True)
    # (set_sub_batches cuts equal slices: the slices under test are put in their place)
    mul._slices = [(bounds[i], bounds[i + 1] - bounds[i]) for i in range(k)]
    mul._bounds_c = (C.c_int32 * (k + 1))(*bounds)
    seen = _Seen()
    gains, sg, ring = _gains(n, 5), _sgains(n, 5), _ring(8, n, 35)
    for rep in range(2):
        _check_launch(ref, mul, gains, sg, ring, rep * T, T, (bounds, rep), seen)
    _end(ref, mul, seen, bounds)


def test_caller_given_bounds_with_an_empty_sector():
    """K = 3, b = (2, 2, 5, 8): an empty first sector, sensors 0, 1 and 8 .. 31 left out; the [2, 16] form of the gains."""
    n, T = 64, 5
    ref, mul = _twins(_cfg(4, 8), _bank("mixed"), n)
    seen = _Seen()
    sg = _sgains(1, 9)[0]
    _check_launch(ref, mul, _gains(n, 9), np.broadcast_to(sg, (n, 2, 16)).copy(), _ring(8, n, 39), 0, T, "K3", seen, bounds=(2, 2, 5, 8))
    # ... and through the [2, 16] form with nothing recorded
    x = _np(ref.read("OBS64"))[:, :6 + 32]
    act = sector_action(x, _gains(n, 9, ring=False), sg, (2, 2, 5, 8))
    ref.step(torch.as_tensor(act, device=DEV))
    assert mul.step_feedback(torch.as_tensor(_gains(n, 9, ring=False), device=DEV), 1, sector_gains=torch.as_tensor(sg, device=DEV),
                             sector_bounds=(2, 2, 5, 8)) is None
    _assert_same_state(ref, mul, "K3, [2, 16] gains, no record")
    _end(ref, mul, seen, "K3")


def test_zero_sector_gains_are_the_existing_closed_loop_launch():
    n, T = 64, 5
    ref, mul = _twins(_cfg(9, 20, max_timesteps=4), _bank("mixed"), n)
    gains, ring = torch.as_tensor(_gains(n, 6), device=DEV), _ring(8, n, 36)
    zero = torch.zeros((2, 16), dtype=torch.float64, device=DEV)
    for rep in range(2):
        want, wact = ref.step_feedback(gains, T, ring=ring, first_slot=(rep * T) % 8, record=True, record_actions=True)
        got, act = mul.step_feedback(gains, T, ring=ring, first_slot=(rep * T) % 8, record=True, record_actions=True, sector_gains=zero)
        torch.cuda.synchronize()
        for x, y in zip(got, want):
            assert torch.equal(x, y), rep
        assert torch.equal(act, wact), rep                         # as numbers: s + 0.0 may turn -0.0 into +0.0
        _assert_same_state(ref, mul, rep)
    assert int(ref.read("COUNTERS")[:, 2].min()) >= 1
    _assert_same_log(ref, mul)
    assert mul.health() == CLEAN
    ref.close(), mul.close()


def test_refusals_return_einval_and_launch_nothing():
    from gym_auv_amd import _capi
    from gym_auv_amd.batched_env import BatchedAuvEnv
    from gym_auv_amd.devgen import FreshWorlds
    lib = _capi.load_library()
    EINVAL = -1
    B48 = (0, 13, 17, 20, 32)

    def call(env, gains, sgains, b=B48, T=2, k=None):
        if env._slices is None:
            env.set_sub_batches(1)
        return lib.auv_step_feedback_sectors(env._h, env.sub_batches, env._bounds_c, env._streams_c, None if gains is None else C.c_void_p(gains.data_ptr()),
                                             None, _capi.AUV_F32, 1, 0, T, C.c_void_p(env.obs.data_ptr()), C.c_void_p(env.reward.data_ptr()),
                                             C.c_void_p(env.done.data_ptr()), None, None, None, None,
                                             None if sgains is None else C.c_void_p(sgains.data_ptr()), None if b is None else (C.c_int32 * len(b))(*b),
                                             (len(b) - 1) if k is None else k)

    def snapshot(env):
        torch.cuda.synchronize()
        return [env.read(f).clone() for f in ("STATE", "COUNTERS", "OBS64", "INFO64")] + [env.obs.clone(), env.reward.clone(), env.done.clone()]

    def unchanged(env, before):
        return all(torch.equal(x, y) for x, y in zip(before, snapshot(env)))

    # a fresh world per reset
    env = BatchedAuvEnv(_cfg(), FreshWorlds(seed=1, batch_cap=8), 16, device=DEV, auto_reset=True)
    g16, h16 = torch.zeros((16, 2, 8), dtype=torch.float64, device=DEV), torch.zeros((16, 2, 16), dtype=torch.float64, device=DEV)
    before = snapshot(env)
    assert call(env, g16, h16) == EINVAL and b"fresh world" in lib.auv_last_error()
    assert unchanged(env, before) and env.health()["timeouts"] == 0
    env.close()
    # more than 64 obstacles per world
    n = 64
    ref, mul = _twins(_cfg(), _bank("k128"), n)
    g, h = torch.as_tensor(_gains(n, 8, ring=False), device=DEV), torch.as_tensor(_sgains(n, 8), device=DEV)
    assert call(mul, g, h) == EINVAL and b"more than 64 obstacles" in lib.auv_last_error()
    _assert_same_state(ref, mul, "k128")
    assert mul.health()["timeouts"] == 0
    ref.close(), mul.close()
    # the LiDAR off
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = BatchedAuvEnv(_cfg(lidar=False), _bank("moving"), n, device=DEV, auto_reset=True)
    env.reset()
    before = snapshot(env)
    assert call(env, g, h) == EINVAL and b"use_lidar" in lib.auv_last_error()
    assert unchanged(env, before) and env.health()["timeouts"] == 0
    with pytest.raises(ValueError):
        env.step_feedback(g, 2, sector_gains=h)
    env.close()
    # pointers, n_sectors, bounds; the step number is not spent: the twins go on in lockstep
    ref, mul = _twins(_cfg(), _bank("moving"), n)
    before = snapshot(mul)
    odd = torch.zeros((n * 32 * 8 + 8,), dtype=torch.uint8, device=DEV)[4:]
    assert odd.data_ptr() % 8 == 4
    for args, msg in (((None, h), b"gains_dev"), ((g, None), b"sector_gains_dev"), ((g, odd), b"sector_gains_dev"), ((odd, h), b"gains_dev"),
                      ((g, h, None, 2, 4), b"sector_bounds_host"), ((g, h, B48, 2, 0), b"n_sectors"), ((g, h, tuple(range(18)), 2, 17), b"n_sectors"),
                      ((g, h, (0, 13, 12, 20, 32)), b"ascending"), ((g, h, (-1, 13, 17, 20, 32)), b"ascending"), ((g, h, (0, 13, 17, 20, 33)), b"ascending"),
                      ((g, h, B48, 0), b"n_steps"), ((g, h, B48, 1025), b"n_steps")):
        assert call(mul, *args) == EINVAL and msg in lib.auv_last_error(), (msg, lib.auv_last_error())
    assert unchanged(mul, before) and mul.health()["timeouts"] == 0
    _assert_same_state(ref, mul, "after the refusals")
    seen = _Seen()
    _check_launch(ref, mul, _np(g), _np(h), None, 0, 3, "after the refusals", seen)
    for kw in (dict(sector_gains=h.float()), dict(sector_gains=h[:, :, :15]), dict(sector_gains=h, sector_bounds=(0, 40)),
               dict(sector_gains=h, sector_bounds=(0, 9, 5)), dict(sector_bounds=B48)):
        with pytest.raises(ValueError):
            mul.step_feedback(g, 2, **kw)
    _assert_same_state(ref, mul, "after the ValueErrors")
    _end(ref, mul, seen, "refusals")
