"""-m gpu: A FRESH WORLD ON EVERY RESET in launches of SEVERAL steps (FreshWorlds(multi_step=True); auv_fresh_worlds_multi,
k_fresh_multi / k_fresh_record).

The steps of one launch read a bound slot's tables with plain loads and no kernel boundary in between, so a launch binds only
slots that were rebuilt and published before any kernel of its call began; an environment whose next
slot does not qualify starts over in the world it has just left, and `fresh_stats()["reused"]` counts it.  What is pinned:
  * BITWISE equality -- every step's record, every field, the slot depth-wise -- with a handle whose large cycling bank was
    generated from the same draws, with a flush between the launches and with passes running beside them;
  * the counted fallback: re-use shows in `reused` AND in the episode log, and nowhere else (finite rows, clean health);
  * one chain == three chains == a shard of the batch;
  * the mode is opt-in: the refusals stay for a default handle and for the closed-loop launches.
The twins' conditions (how many episodes an environment may end inside one launch) are asserted on the cycling handle's own
done record, never on the handle under test; the seeds were checked against them with the CPU oracle stepping the host
mirror's worlds (every episode of these runs ends at the time limit).
"""
import numpy as np
import pytest
import torch

from gym_auv_amd.config import effective_reference_config
from gym_auv_amd.devgen import FreshWorlds, GeneratedWorlds

pytestmark = pytest.mark.gpu

BITWISE = ("STATE", "LIDAR_D", "OBS64", "REWARD64", "INFO64", "NAV64", "MOVER_STATE", "NEARBY", "COLLISION", "COUNTERS", "EPISODE",
           "CULL_LIMITS", "STEP_INFO")
CLEAN = dict(handover_ok=1, probe_failures=0, timeouts=0, pending=0)
SLOTS = 16


def _np(t):
    return t.detach().cpu().numpy()


def _env(cfg, spec, n, **kw):
    from gym_auv_amd.batched_env import BatchedAuvEnv
    kw.setdefault("auto_reset", True)
    return BatchedAuvEnv(cfg, spec, n, device="cuda:0", **kw)


def _cfg(max_timesteps, sensors=(4, 8)):
    cfg = effective_reference_config(use_lidar=True)
    cfg.vessel.n_sectors, cfg.vessel.n_sensors_per_sector = sensors
    cfg.episode.max_timesteps = max_timesteps
    return cfg


def _ring(seed, n):
    """[SLOTS, n, 2] float64 actions from the host's generator (the CPU oracle can replay them)."""
    rs = np.random.RandomState(seed)
    return torch.as_tensor(rs.uniform([-1, -0.15], [1, 0.15], (SLOTS, n, 2)), device="cuda:0").contiguous()


def _twins(cfg, spec, n, n_serial):
    """(fresh, big): the handle under test and a cycling bank of n * n_serial worlds generated from fresh's own draws."""
    fresh = _env(cfg, spec, n)
    rows = fresh.fresh_draws([i % n for i in range(n * n_serial)], [i // n for i in range(n * n_serial)])
    big = _env(cfg, GeneratedWorlds(n * n_serial, seed=0), n)
    big.generate(GeneratedWorlds(n * n_serial, seed=0), draws=rows)
    assert torch.equal(fresh.reset(), big.reset())
    return fresh, big


def _same(big, fresh, n, tag):
    for f in BITWISE:
        assert torch.equal(big.read(f), fresh.read(f)), (tag, f)
    assert torch.equal(big.read("WORLD_IDX") % n, fresh.read("WORLD_IDX") % n), tag


def _launches(big, fresh, ring, n, T, launches, most_ends, between):
    ends_total = 0
    for L in range(launches):
        s = (L * T) % SLOTS
        rb = big.step_multi(ring, s, T, record=True)
        rf = fresh.step_multi(ring, s, T, record=True)
        between()
        ends = rb[2].to(torch.int64).sum(dim=0)
        assert int(ends.max()) <= most_ends, (L, int(ends.max()))       # the condition, on the cycling handle's own record
        ends_total += int(ends.sum())
        for a, b, what in zip(rb, rf, ("obs", "reward", "done")):
            assert torch.equal(a, b), (L, what)
        _same(big, fresh, n, L)
    return ends_total


def test_multi_step_fresh_is_bitwise_a_bank_that_never_repeats():
    """T = 6, max_timesteps = 7, ten launches, a flush between them: every slot left so far is bindable by the next call, so with
    depth 3 an environment may end up to two episodes inside a launch (asserted: it never ends more)."""
    n, T, launches = 64, 6, 10
    cfg = _cfg(7)
    fresh, big = _twins(cfg, FreshWorlds(depth=3, multi_step=True, period=1, batch_cap=64, seed=21), n, launches * T // 7 + 4)
    ring = _ring(4, n)

    def between():
        torch.cuda.synchronize()
        fresh.refill(flush=True)

    ends = _launches(big, fresh, ring, n, T, launches, 2, between)
    assert ends >= (launches * T // 7) * n
    st = fresh.fresh_stats()
    assert st["reused"] == 0 and st["regenerated"] > 0, st
    assert fresh.health() == CLEAN and big.health() == CLEAN
    big.close(), fresh.close()


def test_multi_step_fresh_with_passes_beside_the_launches():
    """T = 16, max_timesteps = 23, twelve launches, no flush -- only a synchronise after each launch, so the pass a call has
    enqueued behind its launches has run when the next call begins.  At most one episode end per environment per launch."""
    n, T, launches = 64, 16, 12
    cfg = _cfg(23)
    fresh, big = _twins(cfg, FreshWorlds(depth=3, multi_step=True, period=1, batch_cap=64, seed=21), n, launches * T // 23 + 4)
    ring = _ring(4, n)
    ends = _launches(big, fresh, ring, n, T, launches, 1, torch.cuda.synchronize)
    assert ends >= (launches * T // 23) * n
    st = fresh.fresh_stats()
    assert st["reused"] == 0 and st["regenerated"] > 0, st
    assert fresh.health() == CLEAN
    big.close(), fresh.close()


def test_counted_fallback_inside_a_launch():
    """No pass is ever enqueued by the steps (period 10^9): with T = 6 and max_timesteps = 2 every environment ends three episodes
    in the first launch and has two spare slots -- the third start is a counted re-use of the world just left."""
    n, T = 64, 6
    cfg = _cfg(2)
    env = _env(cfg, FreshWorlds(depth=3, multi_step=True, period=10 ** 9, batch_cap=64, seed=2), n)
    env.reset()
    ring = _ring(5, n)
    obs, _, done = env.step_multi(ring, 0, T, record=True)
    torch.cuda.synchronize()
    st = env.fresh_stats()
    assert st["reused"] > 0 and st["regenerated"] == 0, st
    assert torch.isfinite(obs).all() and torch.isfinite(env.obs).all()
    assert env.health() == CLEAN
    # a re-use, seen from outside: the environment sits in the world of the episode it has just finished (world = e + N * serial)
    log = _np(env.episode_log())
    assert len(log) == int(done.sum())
    w = _np(env.read("WORLD_IDX"))
    now = np.arange(n) + n * _np(env.read("FW_SERIAL"))[w]
    last = np.array([log[log[:, 0] == e][-1, 7] for e in range(n)])
    assert int((now == last).sum()) == st["reused"], (int((now == last).sum()), st)
    # every slot left so far becomes bindable by the next call; two episode ends per environment then find their two spare slots
    env.refill(flush=True)
    st = env.fresh_stats()
    assert st["queued"] == 0 and st["regenerated"] > 0, st
    _, _, done2 = env.step_multi(ring, T % SLOTS, 4, record=True)
    torch.cuda.synchronize()
    per_env = done2.to(torch.int64).sum(dim=0)
    assert int(per_env.max()) <= 2 and int(per_env.sum()) > 0
    assert env.fresh_stats()["reused"] == st["reused"]
    # the re-used worlds' second episodes have ended now: in the log, an environment's consecutive episodes that share a world are
    # exactly the counted re-uses
    log2 = _np(env.episode_log())                             # (the episodes finished since the last look)
    assert len(log2) == int(done2.sum())
    log = np.concatenate([log, log2])
    shared = 0
    for e in range(n):
        mine = log[log[:, 0] == e][:, 7]
        shared += int((mine[1:] == mine[:-1]).sum())
    assert shared == st["reused"], (shared, st)
    assert torch.isfinite(env.obs).all() and env.health() == CLEAN
    env.close()


def test_chains_and_shards_meet_the_same_worlds_in_multi_step_launches():
    """One chain == three chains, bit for bit, and a handle over the second half of the batch (env_index_base = n / 2) == those
    environments of the whole batch; at most one episode end per environment per launch (asserted on the one-chain record)."""
    n, T, launches = 128, 8, 10
    cfg = _cfg(23)
    kw = dict(depth=3, multi_step=True, period=1, seed=9)
    one = _env(cfg, FreshWorlds(batch_cap=128, **kw), n)
    three = _env(cfg, FreshWorlds(batch_cap=128, **kw), n)
    half = _env(cfg, FreshWorlds(batch_cap=64, env_index_base=n // 2, **kw), n // 2)
    three.set_sub_batches(3, strict=True)
    for e in (one, three, half):
        e.reset()
    ring = _ring(8, n)
    ring_half = ring[:, n // 2:].contiguous()
    torch.cuda.synchronize()
    ends_total = 0
    for L in range(launches):
        s = (L * T) % SLOTS
        r1 = one.step_multi(ring, s, T, record=True)
        r3 = three.step_multi(ring, s, T, record=True)
        rh = half.step_multi(ring_half, s, T, record=True)
        torch.cuda.synchronize()
        ends = r1[2].to(torch.int64).sum(dim=0)
        assert int(ends.max()) <= 1, L
        ends_total += int(ends.sum())
        for a, b, c in zip(r1, r3, rh):
            assert torch.equal(a, b), L
            assert torch.equal(a[:, n // 2:], c), L
    assert ends_total >= 3 * n
    for e in (one, three, half):
        assert e.fresh_stats()["reused"] == 0, e.fresh_stats()
    for f in BITWISE + ("WORLD_IDX",):
        a, b, c = one.read(f), three.read(f), half.read(f)
        assert torch.equal(a, b), f
        if f == "STATE":
            assert torch.equal(a[:, n // 2:], c), f
        elif f == "WORLD_IDX":
            assert torch.equal(a[n // 2:] // n, c // (n // 2)), f       # the same slot depth-wise
        else:
            assert torch.equal(a[n // 2:], c), f
    assert three.health() == CLEAN
    one.close(), three.close(), half.close()


def test_multi_step_fresh_is_opt_in():
    n, T = 64, 6
    cfg = _cfg(7)
    ring = _ring(4, n)
    plain = _env(cfg, FreshWorlds(depth=3, period=1, batch_cap=64, seed=21), n)
    plain.reset()
    with pytest.raises(RuntimeError, match="fresh world"):
        plain.step_multi(ring, 0, T)
    with pytest.raises(RuntimeError, match="fresh world"):
        plain.step_multi(ring, 0, T, record=True)
    plain.close()
    with pytest.raises(ValueError):
        FreshWorlds(depth=2, multi_step=True)
    fresh, big = _twins(cfg, FreshWorlds(depth=3, multi_step=True, period=1, batch_cap=64, seed=21), n, 8)
    gains = torch.zeros((n, 2, 8), dtype=torch.float64, device="cuda:0")
    with pytest.raises(RuntimeError, match="fresh world"):
        fresh.step_feedback(gains, T)
    # one-step calls behind a multi-step launch: the handle steps on as a one-step fresh-world handle does
    big.step_multi(ring, 0, T)
    fresh.step_multi(ring, 0, T)
    torch.cuda.synchronize()
    _same(big, fresh, n, "multi")
    for t in range(12):
        a = ring[(T + t) % SLOTS]
        o0, r0, d0, _ = big.step(a)
        o1, r1, d1, _ = fresh.step(a)
        torch.cuda.synchronize()
        assert torch.equal(o0, o1) and torch.equal(r0, r1) and torch.equal(d0, d1), t
    _same(big, fresh, n, "one-step")
    assert int(big.read("COUNTERS")[:, 2].min()) >= 2
    assert fresh.fresh_stats()["reused"] == 0 and fresh.health() == CLEAN
    big.close(), fresh.close()
