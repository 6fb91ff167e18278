"""-m gpu: CLOSED-LOOP launches of several steps with A FRESH WORLD ON EVERY RESET (FreshWorlds(multi_step=True, closed_loop=True);
auv_fresh_worlds_multi(h, 2); k_fresh_feedback / k_fresh_sector_feedback / k_fresh_hidden_feedback).

What the feature adds is one hand-over: the action of the step after a reset is the feedback law of the reset row of the world the
reset ACTUALLY bound -- the environment's next slot if that was published before the call began, else (counted) the world just left.
What is pinned:
  * BITWISE equality -- obs, reward, done AND the action record of every step, every field, the slot depth-wise -- with a handle whose
    large cycling bank was generated from the same draws and which runs the EXISTING closed-loop launch with the same parameters
    (itself pinned bit for bit to one-step calls fed by the NumPy mirrors: tests/test_gpu_feedback*.py); with a flush between the
    launches for every law kind, and with passes running beside the launches;
  * the step after a reset: its action is the NumPy mirror law of the fp64 reset row of the world bound, bit for bit;
  * the counted fallback: re-use shows in `reused` and in the episode log, every row is finite, and the action after a re-use reset
    is the law of the re-used world's reset row;
  * one chain == three chains == a shard of the batch;
  * the mode is opt-in: multi_step alone keeps the refusal for all three law kinds, a capturing stream is refused, depth 2 is EINVAL.
The gains differ between environments (a seeded host generator around the line-of-sight autopilot's): a law fed from another
environment's row, or from the row of the world just left, gives other bits.

The twins' condition -- at most two (one, without a flush) episode ends per environment per launch -- is asserted on the cycling
handle's own done record, never on the handle under test.  The seeds and the gain scale were checked against it on the CPU: the
oracle stepping the host mirror's worlds (devgen.counter_draws -> world_from_draws) with feedback.*_action forming every action
from the oracle's own OBS64 rows.  In that check every episode of the seed-21 runs ends at the time limit (max_timesteps 4, 7 and
23 are too short for these vessels to reach anything else), at most one per environment per launch at max_timesteps = 7 and 23 and
at most two at max_timesteps = 4.  Ends by something OTHER than the time limit were found within the condition with seed 9, 128
environments, max_timesteps = 23: two episodes (environment 60 after 20 steps, environment 42 after 18) in the 192 steps of the
second case of the passes-beside-the-launches test, one of them also in the 80 steps of the chains-and-shards test; the law's
inputs after such a reset come from a row the launch did not see coming.  The counted-fallback test does not depend on why an
episode ends (it derives every expected row from the done record).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from gym_auv_amd import feedback
from gym_auv_amd.config import effective_reference_config
from gym_auv_amd.devgen import FreshWorlds, GeneratedWorlds

pytestmark = pytest.mark.gpu

BITWISE = ("STATE", "LIDAR_D", "OBS64", "REWARD64", "INFO64", "NAV64", "MOVER_STATE", "NEARBY", "COLLISION", "COUNTERS", "EPISODE",
           "CULL_LIMITS", "STEP_INFO")
CLEAN = dict(handover_ok=1, probe_failures=0, timeouts=0, pending=0)
SLOTS = 16
DEV = "cuda:0"
BOUNDS = (0, 13, 17, 20, 32)                       # four uneven sectors over the 32 beams; sectors 4..15 are empty ranges
SEED = 21
# (law kind, activation, ring present)
CASES = [("affine", None, True), ("sectors", None, False), ("hidden", "relu", True), ("hidden", "hardtanh", False)]


def _np(t):
    return t.detach().cpu().numpy()


def _env(cfg, spec, n, **kw):
    from gym_auv_amd.batched_env import BatchedAuvEnv
    kw.setdefault("auto_reset", True)
    return BatchedAuvEnv(cfg, spec, n, device=DEV, **kw)


def _cfg(max_timesteps, sensors=(4, 8)):
    cfg = effective_reference_config(use_lidar=True)
    cfg.vessel.n_sectors, cfg.vessel.n_sensors_per_sector = sensors
    cfg.episode.max_timesteps = max_timesteps
    return cfg


def ring_np(seed, n):
    """[SLOTS, n, 2] float64 actions from the host's generator (the CPU oracle can replay them)."""
    return np.random.RandomState(seed).uniform([-1, -0.15], [1, 0.15], (SLOTS, n, 2))


def law_np(kind, n, seed=5):
    """The law's parameters, per environment, from a seeded host generator around the line-of-sight autopilot's gains (NumPy)."""
    rs = np.random.RandomState(seed)
    p = dict(kind=kind, gains=np.broadcast_to(feedback.los_gains(0.7, 0.8, 0.4, 0.5), (n, 2, 8)) + rs.normal(0.0, 0.2, (n, 2, 8)))
    if kind != "affine":
        p["sector_gains"] = rs.normal(0.0, 0.3, (n, 2, 16))
    if kind == "hidden":
        p["hidden"] = feedback.pack_hidden(rs.normal(0.0, 0.3, (n, 16, 24)), rs.normal(0.0, 0.2, (n, 16)), rs.normal(0.0, 0.2, (n, 2, 16)))
    return p


def law_action(p, rows, ring_action, activation=None, envs=None):
    """The NumPy mirror law of parameters `p` (rows of `envs`, default all) on whole OBS64 rows."""
    sl = slice(None) if envs is None else envs
    if p["kind"] == "affine":
        return feedback.affine_action(rows, p["gains"][sl], ring_action)
    if p["kind"] == "sectors":
        return feedback.sector_action(rows, p["gains"][sl], p["sector_gains"][sl], BOUNDS, ring_action)
    return feedback.hidden_action(rows, p["gains"][sl], p["sector_gains"][sl], BOUNDS, p["hidden"][sl], activation, ring_action)


def _kw(p, activation, lo=0, hi=None):
    """step_feedback's arguments for the parameters `p` (environments lo .. hi)."""
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a[lo:hi]), device=DEV)
    kw = dict(gains=dev(p["gains"]))
    if p["kind"] != "affine":
        kw.update(sector_gains=dev(p["sector_gains"]), sector_bounds=BOUNDS)
    if p["kind"] == "hidden":
        kw.update(hidden=dev(p["hidden"]), activation=activation)
    return kw


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


def _launches(big, fresh, kw, ring, n, T, launches, most_ends, between):
    ends_total = 0
    for L in range(launches):
        s = (L * T) % SLOTS if ring is not None else 0
        rb, ab = big.step_feedback(n_steps=T, ring=ring, first_slot=s, record=True, record_actions=True, **kw)
        rf, af = fresh.step_feedback(n_steps=T, ring=ring, first_slot=s, record=True, record_actions=True, **kw)
        between()
        ends = rb[2].to(torch.int64).sum(dim=0)
        assert int(ends.max()) <= most_ends, (L, int(ends.max()))       # the condition, on the cycling handle's own record
        ends_total += int(ends.sum())
        for a, b, what in zip(rb + (ab,), rf + (af,), ("obs", "reward", "done", "act_rec")):
            assert torch.equal(a, b), (L, what)
        _same(big, fresh, n, L)
    return ends_total


@pytest.mark.parametrize("kind,activation,with_ring,max_t", [c + (7,) for c in CASES] + [CASES[2] + (4,)])
def test_closed_loop_fresh_is_bitwise_a_bank_that_never_repeats(kind, activation, with_ring, max_t):
    """T = 6, max_timesteps = 7, ten launches, a flush between them: every slot left so far is bindable by the next call, so with
    depth 3 an environment may end up to two episodes inside a launch (asserted: it never ends more).  With max_timesteps = 7 no
    environment ends more than one; the last case, max_timesteps = 4, has launches with two ends per environment -- two hand-overs
    of an action across a reset in one launch, the second one into the environment's last spare slot."""
    n, T, launches = 64, 6, 10
    cfg = _cfg(max_t)
    n_serial = launches * T // max_t + 4
    fresh, big = _twins(cfg, FreshWorlds(depth=3, multi_step=True, closed_loop=True, period=1, batch_cap=64, seed=SEED), n, n_serial)
    ring = torch.as_tensor(ring_np(4, n), device=DEV).contiguous() if with_ring else None
    p = law_np(kind, n)
    g = p["gains"]
    assert (np.abs(g[1:] - g[:-1]).max(axis=(1, 2)) > 0.05).all()         # the environments' laws differ

    def between():
        torch.cuda.synchronize()
        fresh.refill(flush=True)

    ends = _launches(big, fresh, _kw(p, activation), ring, n, T, launches, 2, between)
    assert ends >= (launches * T // max_t) * n
    assert int(big.read("COUNTERS")[:, 2].max()) < n_serial                # (the yardstick's bank never came round)
    st = fresh.fresh_stats()
    assert st["reused"] == 0 and st["regenerated"] > 0, st
    assert fresh.health() == CLEAN and big.health() == CLEAN
    big.close(), fresh.close()


@pytest.mark.parametrize("seed,n,ring_seed,activation,early", [(SEED, 64, 4, "relu", False), (9, 128, 8, "hardtanh", True)])
def test_closed_loop_fresh_with_passes_beside_the_launches(seed, n, ring_seed, activation, early):
    """T = 16, max_timesteps = 23, twelve launches, no flush -- only a synchronise after each launch, so the pass a call has
    enqueued behind its launches has run when the next call begins.  At most one episode end per environment per launch.
    `early`: the run has episodes that end before the time limit (asserted on the cycling handle's counters)."""
    T, launches = 16, 12
    cfg = _cfg(23)
    n_serial = launches * T // 23 + 4
    fresh, big = _twins(cfg, FreshWorlds(depth=3, multi_step=True, closed_loop=True, period=1, batch_cap=n, seed=seed), n, n_serial)
    ring = torch.as_tensor(ring_np(ring_seed, n), device=DEV).contiguous()
    ends = _launches(big, fresh, _kw(law_np("hidden", n), activation), ring, n, T, launches, 1, torch.cuda.synchronize)
    assert ends >= (launches * T // 23) * n
    steps = _np(big.episode_log())[:, 2]
    assert len(steps) == ends and bool((steps < 23).any()) == early, (len(steps), ends, int((steps < 23).sum()))
    assert int(big.read("COUNTERS")[:, 2].max()) < n_serial
    st = fresh.fresh_stats()
    assert st["reused"] == 0 and st["regenerated"] > 0, st
    assert fresh.health() == CLEAN
    big.close(), fresh.close()


def _reset_rows(cfg, fresh, n, serials):
    """[len(serials), n, 6 + S] fp64: the reset rows of the worlds (environment e, serial k), from a cycling handle generated from
    `fresh`'s draws and reset into each of them."""
    k = len(serials)
    rows = fresh.fresh_draws([i % n for i in range(n * k)], [serials[i // n] for i in range(n * k)])
    bank = _env(cfg, GeneratedWorlds(n * k, seed=0), n)
    bank.generate(GeneratedWorlds(n * k, seed=0), draws=rows)
    out = []
    for j in range(k):
        bank.reset(world_idx=torch.arange(n, dtype=torch.int32, device=DEV) + n * j)
        out.append(_np(bank.read("OBS64")).copy())
    bank.close()
    return np.stack(out)


@pytest.mark.parametrize("kind,activation,with_ring", [CASES[0], CASES[2]])
def test_the_action_of_the_step_after_a_reset_is_the_law_of_the_world_bound(kind, activation, with_ring):
    """max_timesteps = 4 < T = 6, from a reset: every environment ends its first episode in step 3 (asserted) and is bound to the
    world of serial 1; row 4 of the action record is the mirror law of that world's fp64 reset row -- not of the row the tail left,
    and not of the world just left."""
    n, T = 64, 6
    cfg = _cfg(4)
    fresh = _env(cfg, FreshWorlds(depth=3, multi_step=True, closed_loop=True, period=1, batch_cap=64, seed=SEED), n)
    fresh.reset()
    row0 = _np(fresh.read("OBS64")).copy()
    rows = _reset_rows(cfg, fresh, n, [0, 1])
    assert np.array_equal(rows[0], row0)                                   # (the mirror bank's serial 0 is the world the handle is in)
    rn = ring_np(4, n)
    ring = torch.as_tensor(rn, device=DEV).contiguous()
    p = law_np(kind, n)
    (obs, _, done), act = fresh.step_feedback(n_steps=T, ring=ring, first_slot=2, record=True, record_actions=True, **_kw(p, activation))
    torch.cuda.synchronize()
    done, act = _np(done), _np(act)
    assert (done[3] == 1).all() and done.sum() == n
    want = law_action(p, rows[1], rn[(2 + 4) % SLOTS], activation)
    assert np.array_equal(act[4].view(np.uint64), want.view(np.uint64))
    assert not np.array_equal(act[4], law_action(p, rows[0], rn[(2 + 4) % SLOTS], activation))      # (the world just left gives other bits)
    assert np.array_equal(act[0].view(np.uint64), law_action(p, rows[0], rn[2], activation).view(np.uint64))   # step 0: from the arrays
    w = _np(fresh.read("WORLD_IDX"))
    assert (_np(fresh.read("FW_SERIAL"))[w] == 1).all() and (w % n == np.arange(n)).all()
    assert torch.isfinite(obs).all()
    assert fresh.fresh_stats()["reused"] == 0 and fresh.health() == CLEAN
    fresh.close()


def test_counted_fallback_inside_a_closed_loop_launch():
    """No pass is ever enqueued by the steps (period 10^9): with T = 8 and max_timesteps = 2 every environment ends four episodes in
    the launch and has two spare slots -- from the third end on it starts over in the world it has just left, counted.  The action
    after EVERY reset, re-use included, is the law of the reset row of the world the environment is then in: serial min(k, 2) after
    its k-th end (derived from the done record, whatever ended the episodes)."""
    n, T = 64, 8
    cfg = _cfg(2)
    env = _env(cfg, FreshWorlds(depth=3, multi_step=True, closed_loop=True, period=10 ** 9, batch_cap=64, seed=2), n)
    env.reset()
    rows = _reset_rows(cfg, env, n, [0, 1, 2])
    rn = ring_np(5, n)
    ring = torch.as_tensor(rn, device=DEV).contiguous()
    p = law_np("hidden", n)
    (obs, reward, done), act = env.step_feedback(n_steps=T, ring=ring, first_slot=0, record=True, record_actions=True, **_kw(p, "relu"))
    torch.cuda.synchronize()
    st = env.fresh_stats()
    assert st["reused"] > 0 and st["regenerated"] == 0, st
    assert torch.isfinite(obs).all() and torch.isfinite(reward).all() and torch.isfinite(act).all() and torch.isfinite(env.obs).all()
    assert env.health() == CLEAN
    done, act = _np(done), _np(act)
    ends = done.astype(np.int64).cumsum(axis=0)
    assert int(ends[-1].min()) >= 3                                        # every environment ran out of spare slots
    assert int(np.maximum(ends[-1] - 2, 0).sum()) == st["reused"], st
    checked = reused_checked = 0
    for t in range(T - 1):
        envs = np.nonzero(done[t])[0]
        if not len(envs):
            continue
        serial = np.minimum(ends[t, envs], 2)
        want = law_action(p, rows[serial, envs], rn[(t + 1) % SLOTS][envs], "relu", envs=envs)
        assert np.array_equal(act[t + 1, envs].view(np.uint64), want.view(np.uint64)), t
        checked += len(envs)
        reused_checked += int((ends[t, envs] > 2).sum())
    assert checked >= 3 * n and reused_checked > 0
    # the episode log shows the re-use: consecutive episodes of an environment in one world (world = e + N * serial)
    log = _np(env.episode_log())
    assert len(log) == int(done.sum())
    w = _np(env.read("WORLD_IDX"))
    now = np.arange(n) + n * _np(env.read("FW_SERIAL"))[w]
    shared = 0
    for e in range(n):
        mine = np.append(log[log[:, 0] == e][:, 7], now[e])
        shared += int((mine[1:] == mine[:-1]).sum())
    assert shared == st["reused"], (shared, st)
    env.close()


def test_chains_and_shards_meet_the_same_worlds_in_closed_loop_launches():
    """One chain == three chains, bit for bit, and a handle over the second half of the batch (env_index_base = n / 2) == those
    environments of the whole batch; at most one episode end per environment per launch (asserted on the one-chain record)."""
    n, T, launches = 128, 8, 10
    cfg = _cfg(23)
    kw = dict(depth=3, multi_step=True, closed_loop=True, period=1, seed=9)
    one = _env(cfg, FreshWorlds(batch_cap=128, **kw), n)
    three = _env(cfg, FreshWorlds(batch_cap=128, **kw), n)
    half = _env(cfg, FreshWorlds(batch_cap=64, env_index_base=n // 2, **kw), n // 2)
    three.set_sub_batches(3, strict=True)
    for e in (one, three, half):
        e.reset()
    ring = torch.as_tensor(ring_np(8, n), device=DEV).contiguous()
    ring_half = ring[:, n // 2:].contiguous()
    p = law_np("hidden", n)
    kw_all, kw_half = _kw(p, "hardtanh"), _kw(p, "hardtanh", n // 2, n)
    torch.cuda.synchronize()
    ends_total = 0
    for L in range(launches):
        s = (L * T) % SLOTS
        r1, a1 = one.step_feedback(n_steps=T, ring=ring, first_slot=s, record=True, record_actions=True, **kw_all)
        r3, a3 = three.step_feedback(n_steps=T, ring=ring, first_slot=s, record=True, record_actions=True, **kw_all)
        rh, ah = half.step_feedback(n_steps=T, ring=ring_half, first_slot=s, record=True, record_actions=True, **kw_half)
        torch.cuda.synchronize()
        ends = r1[2].to(torch.int64).sum(dim=0)
        assert int(ends.max()) <= 1, L
        ends_total += int(ends.sum())
        for a, b, c in zip(r1 + (a1,), r3 + (a3,), rh + (ah,)):
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


def test_closed_loop_fresh_is_opt_in():
    from gym_auv_amd import _capi
    lib = _capi.load_library()
    n, T = 64, 6
    cfg = _cfg(7)
    # multi_step alone: all three law kinds stay refused
    multi = _env(cfg, FreshWorlds(depth=3, multi_step=True, period=1, batch_cap=64, seed=SEED), n)
    multi.reset()
    for kind, activation, _ in CASES:
        with pytest.raises(RuntimeError, match="fresh world"):
            multi.step_feedback(n_steps=T, **_kw(law_np(kind, n), activation))
    multi.close()
    # depth 2: the specification refuses, and so does the library (AUV_EINVAL = -1) -- for 2 as for 1
    with pytest.raises(ValueError):
        FreshWorlds(depth=2, multi_step=True, closed_loop=True)
    two = _env(cfg, FreshWorlds(depth=2, period=1, batch_cap=64, seed=SEED), n)
    assert lib.auv_fresh_worlds_multi(two._h, 2) == -1 and b"depth" in lib.auv_last_error()
    assert lib.auv_fresh_worlds_multi(two._h, 1) == -1
    two.close()
    # a stream that is being captured: refused before anything is launched (the call's number is a launch argument)
    env = _env(cfg, FreshWorlds(depth=3, multi_step=True, closed_loop=True, period=1, batch_cap=64, seed=SEED), n)
    env.reset()
    gains = torch.as_tensor(np.ascontiguousarray(law_np("affine", n)["gains"]), device=DEV)
    scratch = torch.zeros(8, device=DEV)
    cap = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cap):
        scratch.add_(1.0)                                                  # (so that the captured graph is not empty)
        rc = lib.auv_step_feedback(env._h, 1, (C.c_int32 * 2)(0, n), (C.c_void_p * 1)(cap.cuda_stream), C.c_void_p(gains.data_ptr()), None,
                                   _capi.AUV_F32, 1, 0, T, C.c_void_p(env.obs.data_ptr()), C.c_void_p(env.reward.data_ptr()),
                                   C.c_void_p(env.done.data_ptr()), None, None, None, None)
        err = lib.auv_last_error()
    assert rc == -1 and b"captured" in err, (rc, err)
    torch.cuda.synchronize()
    # ... and the same call outside a capture goes through
    assert env.step_feedback(gains, T) is None
    torch.cuda.synchronize()
    assert env.health() == CLEAN
    env.close()
