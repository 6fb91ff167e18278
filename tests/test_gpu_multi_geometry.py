"""-m gpu: k_step_multi's launch geometry (csrc/auv_multi_geom.h) on the device.

The cohort order at cohort counts that are not powers of two (the division by C is then not exact by the multiplier alone), at
every lead / lag clamp, bit for bit against one-step launches and the step-major order; whole batches against the oracle in the
multi-step shape; one slice where the multiplier alone decodes wrong (C = 10923, from step 36 on: tests/test_multi_geometry.py
checks the decode of that very launch on the host first); and a launch past the dispatch limit, refused before anything runs."""
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


def _np(t):
    return t.detach().cpu().numpy()


def _env(cfg, bank, n):
    from gym_auv_amd.batched_env import BatchedAuvEnv
    return BatchedAuvEnv(cfg, bank, n, device="cuda:0", auto_reset=True)


def _moving_bank(n_worlds):
    return pack_bank([build_world(moving_obstacles_world(500 + i)) for i in range(n_worlds)])


def _cfg(max_timesteps=13):
    cfg = effective_reference_config(use_lidar=True)
    cfg.vessel.n_sectors, cfg.vessel.n_sensors_per_sector = 8, 8
    cfg.episode.max_timesteps = max_timesteps
    return cfg


def _ring(slots, n, seed, dtype=torch.float32):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    u = torch.rand((slots, n, 2), generator=g, device="cuda:0", dtype=torch.float64)
    return (u * torch.tensor([2.0, 0.3], device="cuda:0", dtype=torch.float64) - torch.tensor([1.0, 0.15], device="cuda:0", dtype=torch.float64)).to(dtype)


def _assert_same(a, b, where):
    assert torch.equal(a.obs, b.obs) and torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done), where
    for f in FIELDS:
        assert torch.equal(a.read(f), b.read(f)), (where, f)


ORDERS = [(1, 1), (0, 0), (4096, 4096), (2, 60)]


@pytest.mark.parametrize("n", [192, 320, 4032, 4160])        # C = 3 (lead = lag = 1 whatever is asked), 5, 63, 65
def test_cohort_order_off_powers_of_two_is_bitwise(n):
    cfg = _cfg()
    bank = _moving_bank(48)
    ref, coh, stp = _env(cfg, bank, n), _env(cfg, bank, n), _env(cfg, bank, n)
    for e in (ref, coh, stp):
        e.reset()
    stp.set_multi_order("steps")
    slots = 16
    ring = _ring(slots, n, 31)
    t = 0
    lengths = [(lead, lag, T) for lead, lag in ORDERS for T in (1, 5, 64)] + ([(16, 30, 1024)] if n == 192 else [])
    for lead, lag, T in lengths:
        coh.set_multi_order("cohorts", lead, lag)
        for j in range(T):
            ref.step(ring[(t + j) % slots])
        coh.step_multi(ring, t % slots, T)
        stp.step_multi(ring, t % slots, T)
        t += T
        torch.cuda.synchronize()
        _assert_same(ref, coh, ("cohorts", lead, lag, T))
        _assert_same(ref, stp, ("steps", lead, lag, T))
    assert int(ref.read("COUNTERS")[:, 2].sum()) >= 3 * n                 # every environment turned over inside launches
    for e in (coh, stp):
        assert e.health()["timeouts"] == 0
    for e in (ref, coh, stp):
        e.close()


def _fullsize_bank(kind, n_worlds=48):
    gen = {"polygons50": lambda s: polygon_world(s, 50),
           "mixed47": lambda s: polygon_world(s, 10, n_circles=20, n_moving=17)}[kind]
    return pack_bank([build_world(gen(3000 + i)) for i in range(n_worlds)])


class _OracleRun:
    """The oracle over a set of the batch's environments, with the batch's auto-reset: a finished environment restarts in
    world (w + N) % W, step by step (also inside a multi-step launch)."""

    def __init__(self, cfg, bank, n_batch, envs):
        from oracle.pyoracle import Oracle
        self.ora = Oracle(make_config(cfg, auto_reset=False), len(envs), bank)
        self.n, self.W = n_batch, int(bank["n_worlds"])
        self.w = (np.asarray(envs) % self.W).astype(np.int32)
        self.obs = self.ora.reset(world_idx=self.w)
        self.last = None                                        # (obs, reward, done) of the last step

    def step(self, a):
        obs, rew, done = self.ora.step(a)
        if done.any():
            self.w = np.where(done > 0, (self.w + self.n) % self.W, self.w).astype(np.int32)
            o_r = self.ora.reset(mask=done, world_idx=self.w)
            obs = np.where(done[:, None] > 0, o_r, obs)
        self.obs = obs
        return obs, rew, done


def _check_against(env, run, envs, where):
    """test_gpu_fullsize.py's tolerances."""
    np.testing.assert_array_equal(_np(env.done)[envs], run.last[2], err_msg=str(where))
    np.testing.assert_allclose(_np(env.obs)[envs], run.obs, rtol=0, atol=1e-6, err_msg=str(where))
    np.testing.assert_allclose(_np(env.reward)[envs], run.last[1], rtol=1e-6, atol=1e-4, err_msg=str(where))
    np.testing.assert_allclose(_np(env.read("OBS64"))[envs], run.obs, rtol=0, atol=1e-6, err_msg=str(where))
    np.testing.assert_allclose(_np(env.read("STATE"))[:, envs], run.ora.read("STATE"), rtol=0, atol=1e-9, err_msg=str(where))
    np.testing.assert_allclose(_np(env.read("LIDAR_D"))[envs], run.ora.read("LIDAR_D"), rtol=0, atol=1e-9, err_msg=str(where))
    np.testing.assert_array_equal(_np(env.read("WORLD_IDX"))[envs], run.w, err_msg=str(where))


@pytest.mark.parametrize("kind,n,ns,nps", [("polygons50", 4160, 9, 20), ("mixed47", 4032, 16, 16)])
def test_whole_batch_matches_oracle_in_multi_step_launches(kind, n, ns, nps):
    cfg = effective_reference_config(use_lidar=True)
    cfg.vessel.n_sectors, cfg.vessel.n_sensors_per_sector = ns, nps
    cfg.episode.max_timesteps = 23
    bank = _fullsize_bank(kind)
    env = _env(cfg, bank, n)
    envs = np.arange(n)
    env.reset()
    run = _OracleRun(cfg, bank, n, envs)
    np.testing.assert_allclose(_np(env.obs), run.obs, rtol=0, atol=1e-6)
    ring = _ring(128, n, 5, torch.float64)
    a_np = _np(ring)
    t, total_done = 0, 0
    for T in [64] + [7, 1] * 8:                                 # 128 steps
        env.step_multi(ring, t, T)
        for j in range(T):
            run.last = run.step(a_np[t + j])
            total_done += int(run.last[2].sum())
        t += T
        torch.cuda.synchronize()
        _check_against(env, run, envs, (kind, t))
    assert t == 128 and total_done >= n
    assert env.health()["timeouts"] == 0
    env.close()


def test_slice_where_the_multiplier_alone_decodes_wrong():
    """C = 10923 cohorts (699 072 environments): ceil(2^32 / C) alone puts q = 36 C + C - 1 in step 37, cohort -1.  One 40-step
    cohort launch (within the dispatch limit: 4.03 G work-items) equals the same 40 steps in step-major order bit for bit."""
    n, T = 64 * 10923, 40
    cfg = _cfg()
    bank = _moving_bank(16)
    coh, stp = _env(cfg, bank, n), _env(cfg, bank, n)
    for e in (coh, stp):
        e.set_step_mode("one_launch")                           # ("auto" takes three launches from 65536 environments on)
        e.reset()
    stp.set_multi_order("steps")
    rs = np.random.RandomState(3)
    sub = np.sort(rs.choice(n, 64, replace=False))
    sub[-1] = n - 1                                             # the last cohort's last environment among them
    run = _OracleRun(cfg, bank, n, sub)
    ring = _ring(T, n, 17, torch.float64)
    coh.step_multi(ring, 0, T)
    stp.step_multi(ring, 0, T)
    torch.cuda.synchronize()
    _assert_same(coh, stp, "C = 10923")
    a_np = _np(ring[:, sub])
    for j in range(T):
        run.last = run.step(a_np[j])
    _check_against(coh, run, sub, "C = 10923")
    assert int(coh.read("COUNTERS")[:, 2].min()) >= 1               # every environment finished an episode inside the launch
    assert coh.health()["timeouts"] == 0 and stp.health()["timeouts"] == 0
    coh.close(), stp.close()


def test_launch_past_the_dispatch_limit_is_refused_and_launches_nothing():
    """32 768 environments x 1024 steps: 75.5 M workgroups (4.8 G work-items) step-major, 4.8 G in cohort order."""
    n = 32768
    cfg = _cfg()
    bank = _moving_bank(16)
    env, twin = _env(cfg, bank, n), _env(cfg, bank, n)
    env.reset(), twin.reset()
    ring = _ring(8, n, 23)
    for order in ("cohorts", "steps"):
        env.set_multi_order(order)
        with pytest.raises(RuntimeError, match="work-items"):
            env.step_multi(ring, 0, 1024)
    env.set_multi_order("cohorts")
    torch.cuda.synchronize()
    _assert_same(env, twin, "after the refusal")
    t = 0
    for T in (5, 64, 3):
        env.step_multi(ring, t % 8, T)
        twin.step_multi(ring, t % 8, T)
        t += T
        torch.cuda.synchronize()
        _assert_same(env, twin, T)
    assert env.health() == twin.health() and env.health()["timeouts"] == 0
    env.close(), twin.close()
