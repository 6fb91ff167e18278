"""-m gpu: the navigation's path search and knot lookup where their shortcuts can go wrong -- exact ties between distant parts
of a path (across chunks, across the two chunks of one trip to memory, between the two chunks held in registers, on the route
for paths of more than 256 chunks), hints that name the wrong, the last or no chunk, chunk-boundary sizes, repeated vertices,
knot tables the uniform guess misses -- on the hand-built banks of tests/nav_edge_banks.py, against the oracle (which
tests/test_nav_edges.py holds to the brute-force definition on the very same poses) and against that definition itself."""
import numpy as np
import pytest
import torch

import nav_edge_banks as nb

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS = ("STATE", "OBS64", "REWARD64", "INFO64", "NAV64")
ATOL = 1e-9                      # the standing fp64 tolerance (tests/test_gpu_parity.py)


def _np(t):
    return t.detach().cpu().numpy()


def _env(cfg, bank, n, **kw):
    from gym_auv_amd.batched_env import BatchedAuvEnv
    return BatchedAuvEnv(cfg, bank, n, device=DEV, auto_reset=False, **kw)


def _snapshot(env):
    torch.cuda.synchronize()
    out = {f: env.read(f).clone() for f in FIELDS}
    out["obs"], out["done"], out["reward"] = env.obs.clone(), env.done.clone(), env.reward.clone()
    return out


def _assert_oracle(snap, want, msg):
    for f in FIELDS:
        np.testing.assert_allclose(_np(snap[f]), want[f], rtol=0, atol=ATOL, err_msg="%s %s" % (f, msg))
    np.testing.assert_array_equal(_np(snap["done"]), want["done"], err_msg="done %s" % msg)
    np.testing.assert_allclose(_np(snap["obs"]), want["OBS64"][:, :snap["obs"].shape[1]], rtol=0, atol=1e-6, err_msg="obs %s" % msg)


def _oracle_fields(ora, done):
    out = {f: ora.read(f) for f in FIELDS}
    out["done"] = np.asarray(done).copy()
    return out


@pytest.mark.parametrize("name", nb.CASE_NAMES)
def test_search_and_lookup_whatever_the_hint(name):
    """Per-kernel (nav_reward(mode=1)): every pose of the case once per hint -- 0, the true arclength, the opposite leg, the
    last (partial) chunk, L, 1.5 L, -5 -- written to INFO64[6] before the call.  The outputs are the same bits for every hint,
    the oracle's to 1e-9, and s / chi / look-ahead heading / heading error / cross-track error / s_t the brute-force
    definition's to 1e-9; on a far tie s is the smaller of the tied arclengths."""
    c = nb.case(name)
    n = len(c.poses)
    ora = nb.oracle_nav(c)
    want = _oracle_fields(ora, ora.last_done)
    brute = nb.brute_force_rows(c)
    env = _env(nb.nav_config(c.look_ahead), c.bank, n)
    env.reset(world_idx=torch.as_tensor(c.world))
    first = None
    for h in nb.HINTS:
        env.write("STATE", nb.nav_state(c.poses)), env.write("INFO64", nb.hint_info(c, h))
        env.nav_reward(mode=1)
        snap = _snapshot(env)
        _assert_oracle(snap, want, "%s hint %s" % (name, h))
        np.testing.assert_allclose(_np(snap["INFO64"])[:, 6], brute[:, 0], rtol=0, atol=ATOL, err_msg="s, hint %s" % h)
        np.testing.assert_allclose(_np(snap["NAV64"])[:, nb.NAV_COLS], brute[:, 1:], rtol=0, atol=ATOL, err_msg="NAV64, hint %s" % h)
        for i in c.far_tie:
            _, ss = nb.tied_segments(c.bank, int(c.world[i]), c.poses[i][0], c.poses[i][1])
            assert float(snap["INFO64"][i, 6]) == ss.min(), (name, h, i, float(snap["INFO64"][i, 6]), ss)
        if first is None:
            first = snap
        for k in first:
            assert torch.equal(first[k], snap[k]), (name, k, "hint %s against hint %s" % (h, nb.HINTS[0]))
    env.close(), ora.close()


# 128, not 64: sub-batch slices are multiples of 64 environments, so two sub-batches need 128, and bit equality between the
# shapes needs one batch size for all of them
N_STEP, T_STEP = 128, 6


def _step_setup():
    """The step-shape batch: the first half rests on exact far ties (zero state, zero action: the pose stays, the tie comes
    back every step with the now-correct hint), the second half starts off the axis and takes random actions."""
    bank = nb.step_bank()
    ties = nb.step_tie_poses()
    rs = np.random.RandomState(11)
    world, poses = [], []
    for e in range(N_STEP // 2):
        w, x, y = ties[e % len(ties)]
        world.append(w), poses.append([x, y, 0.0])
    for e in range(N_STEP // 2, N_STEP):
        w, x, y = ties[e % len(ties)]
        world.append(w), poses.append([x + rs.uniform(-6, 6), y + rs.uniform(-10, 10), rs.uniform(-3, 3)])
    acts = rs.uniform([-1, -0.15], [1, 0.15], (T_STEP, N_STEP, 2))
    acts[:, :, 0] = np.abs(acts[:, :, 0])
    acts[:, :N_STEP // 2] = 0.0
    return bank, np.array(world, dtype=np.int32), np.array(poses), acts


@pytest.fixture(scope="module")
def step_reference():
    """The oracle's fields after each of the T_STEP steps, and the brute-force s of the resting half."""
    from gym_auv_amd._capi import make_config
    from oracle.pyoracle import Oracle
    bank, world, poses, acts = _step_setup()
    ora = Oracle(make_config(nb.nav_config(300)), N_STEP, bank)
    ora.reset(world_idx=world)
    ora.write("STATE", nb.nav_state(poses))
    rows = []
    for t in range(T_STEP):
        _, _, done = ora.step(acts[t])
        rows.append(_oracle_fields(ora, done))
    ora.close()
    tied = [nb.tied_segments(bank, int(world[e]), poses[e, 0], poses[e, 1])[1] for e in range(N_STEP // 2)]
    assert all(len(ss) >= 2 and ss.max() - ss.min() > 50.0 for ss in tied)
    return rows, np.array([ss.min() for ss in tied])


def _run_shape(shape):
    bank, world, poses, acts = _step_setup()
    env = _env(nb.nav_config(300), bank, N_STEP)
    if shape in ("one_launch", "side_by_side"):
        env.set_step_mode(shape)
    env.reset(world_idx=torch.as_tensor(world))
    env.write("STATE", nb.nav_state(poses))
    ring = torch.as_tensor(acts, device=DEV).contiguous()
    snaps, rec = [], None
    if shape == "multi":
        env.set_sub_batches(1, strict=True)
        torch.cuda.synchronize()
        rec = env.step_multi(ring, 0, T_STEP, record=True)
        snaps.append(_snapshot(env))
    else:
        if shape == "pipelined":
            env.set_sub_batches(2, probe_streams=False)
            assert env.sub_batches == 2
            torch.cuda.synchronize()
        for t in range(T_STEP):
            if shape == "pipelined":
                env.step_pipelined(ring[t])
            else:
                env.step(ring[t])
            snaps.append(_snapshot(env))
    assert env.health()["timeouts"] == 0
    env.close()
    return snaps, rec


@pytest.fixture(scope="module")
def one_launch_run():
    return _run_shape("one_launch")[0]


def _assert_step(snap, t, step_reference, bank, world):
    rows, s_tied = step_reference
    _assert_oracle(snap, rows[t], "step %d" % t)
    st, s = _np(snap["STATE"]), _np(snap["INFO64"])[:, 6]
    half = N_STEP // 2
    np.testing.assert_array_equal(s[:half], s_tied, err_msg="tied s, step %d" % t)       # the smaller tied arclength, outright
    want = [nb.brute_force_nav(bank, int(world[e]), st[0, e], st[1, e])[1] for e in range(half, N_STEP)]
    np.testing.assert_allclose(s[half:], want, rtol=0, atol=ATOL, err_msg="s against brute force, step %d" % t)


@pytest.mark.parametrize("shape", ["one_launch", "side_by_side", "pipelined"])
def test_ties_in_every_step_shape(shape, step_reference, one_launch_run):
    """Six steps in the one-launch, the side-by-side and the two-sub-batch shape: the oracle's fields and the brute-force s
    after every step, and the same bits as the one-launch shape."""
    bank, world, _, _ = _step_setup()
    snaps = one_launch_run if shape == "one_launch" else _run_shape(shape)[0]
    for t, snap in enumerate(snaps):
        _assert_step(snap, t, step_reference, bank, world)
        for k in snap:
            assert torch.equal(snap[k], one_launch_run[t][k]), (shape, k, t)


def test_ties_in_a_launch_of_six_steps(step_reference, one_launch_run):
    """One step_multi launch of six steps with every step recorded: row t of the record is step t of the one-launch shape,
    the fields after it are that shape's after its sixth step -- and the oracle's.

    This case found a defect outside the search: an environment at rest 4 m off its path (cumulative reward r, 2 r, ... beside a
    cross-track sum 4, 8, ...) ended the launch one step short in INFO64[4] and INFO64[7] in about one run of four, because the
    carry record's xor checksum let old sums pass beside a new mark (k_step_fused.hip: carry_mix).  It stays here as the case."""
    bank, world, _, _ = _step_setup()
    snaps, rec = _run_shape("multi")
    _assert_step(snaps[0], T_STEP - 1, step_reference, bank, world)
    for k in snaps[0]:
        assert torch.equal(snaps[0][k], one_launch_run[-1][k]), k
    rows, _ = step_reference
    for t in range(T_STEP):
        for j, k in enumerate(("obs", "reward", "done")):
            assert torch.equal(rec[j][t], one_launch_run[t][k]), (k, t)
        np.testing.assert_allclose(_np(rec[0][t]), rows[t]["OBS64"][:, :rec[0].shape[2]], rtol=0, atol=1e-6)
        np.testing.assert_array_equal(_np(rec[2][t]), rows[t]["done"])
