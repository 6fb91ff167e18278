"""-m gpu: on-device world generation (k5_generate.hip) on the crafted rows of tests/devgen_rows.py -- the edges of its
draws, which random rows never visit -- against the host builder consuming the same rows, at the tolerances of
tests/test_gpu_devgen.py (tables: atol 1e-9, coefficient rows rtol 1e-6 as well, P and segment counts exact; rollouts:
1e-8 on fp64 fields after loading the HOST-built bank into the oracle, flags bit-exact).  tests/test_devgen_edges.py (CPU)
holds the conditions on the rows themselves: every slope branch visited, lengths away from whole decimetres."""
import numpy as np
import pytest
import torch

import devgen_rows as R
from gym_auv_amd import devgen
from gym_auv_amd._capi import make_config
from gym_auv_amd.config import effective_reference_config
from gym_auv_amd.devgen import GeneratedWorlds
from gym_auv_amd.world import build_world, pack_bank

pytestmark = pytest.mark.gpu

NM, NS = 3, 16


def _np(t):
    return t.detach().cpu().numpy()


def _cfg():
    return effective_reference_config(use_lidar=True)


def _host(cfg, rows, nm, ns):
    return [build_world(devgen.world_from_draws(r, nm, ns, dt=cfg.simulation.t_step_size, vessel_width=cfg.vessel.vessel_width))
            for r in rows]


def _generate(cfg, rows, nm, ns, n_envs=None, auto_reset=False):
    """(env whose bank holds the worlds of `rows`, host-built worlds of the same rows)"""
    from gym_auv_amd.batched_env import BatchedAuvEnv
    rows = np.stack(rows)
    assert len(rows) <= 48
    spec = GeneratedWorlds(len(rows), nm, ns, seed=0)
    env = BatchedAuvEnv(cfg, spec, n_envs or len(rows), device="cuda:0", auto_reset=auto_reset)
    env.generate(spec, draws=torch.as_tensor(rows, device="cuda:0"))
    return env, _host(cfg, rows, nm, ns)


def _side(h):
    return "+pi" if h > 3.0 else "-pi" if h < -3.0 else "%.3g" % h


@pytest.mark.parametrize("fam", ["count", "slopes", "radii", "pool_k"])
def test_family_tables_match_host_builder(fam):
    cfg = _cfg()
    cases = R.family(fam, NM, NS)
    env, host = _generate(cfg, [r for _, r in cases], NM, NS)
    t = R.read_tables(env)
    for w, ((name, row), hw) in enumerate(zip(cases, host)):
        R.assert_world_tables(t, w, hw, NM, NS)
        if fam == "radii":
            want = np.maximum(1, R.CIRCLE_POISSON)
            np.testing.assert_array_equal(t["OBS_CULL"][w, :NS, 2], want)
            np.testing.assert_array_equal(t["OBS_META"][w, :NS, 2], hw.obs_meta[:NS, 2])
            assert sorted(set(t["OBS_META"][w, :NS, 2])) == [4, 8, 16, 32, 64]
            np.testing.assert_array_equal(t["MV_PARAM"][w, :, 0], [1, 1, 2])
        if fam == "pool_k":
            k = w + 1
            # the kept candidate is candidate k: its radius, and no rejected 6 km one
            assert t["MV_PARAM"][w, 0, 0] == 10 + k and t["OBS_CULL"][w, 0, 2] == 30 + k
            assert np.all(t["MV_PARAM"][w, :, 0] < 100) and np.all(t["OBS_CULL"][w, :NS, 2] < 100)
    env.close()


def test_cut_tables_match_host_builder():
    """Start headings on the +-pi cut (and at 0 through the wrap): one ulp in the device's atan2 may land on the other side,
    which is the same heading -- WORLD_SCALAR[5] is compared as an angle, everything else as it is."""
    cfg = _cfg()
    cases = R.family("cut", NM, NS)
    env, host = _generate(cfg, [r for _, r in cases], NM, NS)
    t = R.read_tables(env)
    for w, ((name, row), hw) in enumerate(zip(cases, host)):
        print("%s: row[10] = %r: start heading device %r (%s), host %r (%s)"
              % (name, row[10], t["WORLD_SCALAR"][w, 5], _side(t["WORLD_SCALAR"][w, 5]), hw.scalar[5], _side(hw.scalar[5])))
        R.assert_world_tables(t, w, hw, NM, NS, wrap_heading=True)
    env.close()


def test_collinear_tables():
    """All jitters 1/2, theta0 = 0: the waypoints lie on y = 0 and L is 800 up to the last bits, so P = int(10 L) may come out
    as 7999 or 8000 on either side; everything that does not hang on that is compared."""
    cfg = _cfg()
    cases = R.family("collinear", NM, NS)
    env, host = _generate(cfg, [r for _, r in cases], NM, NS)
    t = R.read_tables(env)
    for w, ((name, row), hw) in enumerate(zip(cases, host)):
        p = hw.path
        L, P, Ph = t["WORLD_SCALAR"][w, 0], int(t["POLY_CNT"][w]), len(p.points)
        print("%s: device L = %r P = %d; host L = %r P = %d%s" % (name, L, P, p.length, Ph, "" if P == Ph else "  (P differs)"))
        assert abs(L - p.length) <= 1e-9
        assert abs(P - Ph) <= 1
        assert abs(t["POLY_CUM"][w, P - 1] - L) <= 1e-9
        assert np.all(t["POLY_XY"][w, :P, 1] == 0.0)
        assert np.all(t["KNOT_COEF"][w, :, 4:8] == 0.0)
        np.testing.assert_allclose(t["KNOT_S"][w], p.knot_s, rtol=0, atol=1e-9)
        np.testing.assert_allclose(t["KNOT_COEF"][w, :-1, 0:4], p.cx.T, rtol=1e-6, atol=1e-9)
        keep = np.arange(8) != 5
        np.testing.assert_allclose(t["WORLD_SCALAR"][w, keep], hw.scalar[keep], rtol=0, atol=1e-9)
        assert abs(R.princip(t["WORLD_SCALAR"][w, 5] - hw.scalar[5])) <= 1e-9
        # the polyline is the segment from (400, 0) to (-400, 0), evenly divided
        np.testing.assert_allclose(t["POLY_XY"][w, :P, 0], 400.0 - t["POLY_CUM"][w, :P], rtol=0, atol=1e-9)
        np.testing.assert_allclose(t["POLY_CUM"][w, :P], np.arange(P) * (L / (P - 1)), rtol=0, atol=1e-9)
        R.assert_chunks_bound(t, w, t["POLY_XY"][w, :P])
        R.assert_obstacle_tables(t, w, hw, NM, NS)
        if P == Ph:
            R.assert_world_tables(t, w, hw, NM, NS, wrap_heading=True)
    env.close()


def _mixed(nm, ns):
    """one or two rows of every family but `collinear` (whose P is not pinned), <= 16"""
    rows = dict(R.all_rows(nm, ns))
    names = ["count3", "count7", "slopes0", "slopes3", "slopes4", "cut0", "cut1", "cut2", "radii5", "radii7", "pool1", "pool4", "pool7"]
    return [(n, rows[n]) for n in names]


@pytest.mark.parametrize("nm,ns", [(0, 16), (16, 0), (1, 1)])
def test_other_shapes_match_host_builder(nm, ns):
    cfg = _cfg()
    cases = _mixed(nm, ns)
    env, host = _generate(cfg, [r for _, r in cases], nm, ns)
    t = R.read_tables(env)
    for w, ((name, row), hw) in enumerate(zip(cases, host)):
        R.assert_world_tables(t, w, hw, nm, ns, wrap_heading=name.startswith("cut"))
        if name.startswith("pool"):
            k = int(name[4:])
            assert nm == 0 or t["MV_PARAM"][w, 0, 0] == 10 + k
            assert ns == 0 or t["OBS_CULL"][w, 0, 2] == 30 + k
    env.close()


@pytest.mark.parametrize("name", ["count7", "radii7"])
def test_single_world_bank(name):
    cfg = _cfg()
    row = dict(R.all_rows(NM, NS))[name]
    env, host = _generate(cfg, [row], NM, NS, n_envs=2)
    R.assert_world_tables(R.read_tables(env), 0, host[0], NM, NS)
    env.close()


def test_draws_outside_the_unit_interval_are_refused():
    from gym_auv_amd.batched_env import BatchedAuvEnv
    cfg = _cfg()
    spec = GeneratedWorlds(2, 1, 1, seed=0)
    env = BatchedAuvEnv(cfg, spec, 2, device="cuda:0", auto_reset=False)
    good = np.stack([r for _, r in R.family("cut", 1, 1)[:2]])
    for col, v in ((0, 1.0), (0, -0.25), (0, np.nan), (5, 1.5)):
        bad = good.copy()
        bad[1, col] = v
        with pytest.raises(ValueError):
            env.generate(spec, draws=torch.as_tensor(bad, device="cuda:0"))
    env.generate(spec, draws=torch.as_tensor(good, device="cuda:0"))
    env.close()


# ---- rollouts on the crafted worlds --------------------------------------------------------------------------------------------
def _rollout_vs_oracle(env, ora, n, steps, flipped):
    """the method of test_gpu_devgen.test_rollout_on_generated_worlds_vs_oracle; `flipped` [n] bool: environments whose start
    heading came out on the other side of the +-pi cut than the host's -- their STATE[2] is compared as an angle."""
    np.testing.assert_allclose(_np(env.reset()), ora.reset(), rtol=0, atol=1e-6)
    rs = np.random.RandomState(2)
    for t in range(steps):
        a = rs.uniform([-1, -0.15], [1, 0.15], (n, 2))
        obs, rew, done, _ = env.step(torch.as_tensor(a, device="cuda:0"))
        o_obs, o_rew, o_done = ora.step(a)
        np.testing.assert_array_equal(_np(done), o_done)
        for f in ("STATE", "LIDAR_D", "OBS64", "REWARD64", "INFO64", "NAV64", "MOVER_STATE"):
            dev, ref = _np(env.read(f)).copy(), ora.read(f)
            if f == "STATE" and flipped.any():
                d = dev[flipped, 2] - ref[flipped, 2]
                assert np.all(np.abs(R.princip(d)) <= 1e-8), "STATE[2] step %d" % t
                dev[flipped, 2] -= np.round(d / (2 * np.pi)) * 2 * np.pi
            np.testing.assert_allclose(dev, ref, rtol=0, atol=1e-8, err_msg="%s step %d" % (f, t))
        for f in ("WORLD_IDX", "NEARBY", "COLLISION"):
            np.testing.assert_array_equal(_np(env.read(f)), ora.read(f), err_msg="%s step %d" % (f, t))
        np.testing.assert_allclose(_np(obs), o_obs, rtol=0, atol=1e-6)


def _flipped(t, host):
    dev = t["WORLD_SCALAR"][:, 5]
    ref = np.array([hw.scalar[5] for hw in host])
    assert np.all(np.abs(R.princip(dev - ref)) <= 1e-9)
    return np.abs(dev - ref) > 1.0


def test_rollout_on_crafted_worlds_vs_oracle():
    """One environment per crafted world: the step kernels on 4-segment rings, width-1 movers, a -pi start heading, y = 0 paths."""
    from oracle.pyoracle import Oracle
    cfg = _cfg()
    cases = R.all_rows(NM, NS)
    n = len(cases)
    env, host = _generate(cfg, [r for _, r in cases], NM, NS, auto_reset=True)
    flipped = _flipped(R.read_tables(env), host)
    for (name, _), f in zip(cases, flipped):
        if f:
            print("%s: start heading on the other side of the cut than the host's" % name)
    ora = Oracle(make_config(cfg, auto_reset=True), n, pack_bank(host))
    _rollout_vs_oracle(env, ora, n, 30, flipped)
    np.testing.assert_array_equal(_np(env.read("WORLD_IDX")), np.arange(n))
    env.close()


def test_regenerate_long_to_short_in_place():
    """The longest crafted curve (P = 15093) into a slot, then a near-collinear one (P = 8000) into the same slot: the tables are
    the host's and a rollout equals the oracle's -- nothing reads the stale tail of the longer polyline."""
    from gym_auv_amd.batched_env import BatchedAuvEnv
    from oracle.pyoracle import Oracle
    cfg = _cfg()
    nm, ns, n = 1, 1, 2
    long_row = R.family("slopes", nm, ns)[R.LONGEST_SLOPES][1]
    short_row = R.family("cut", nm, ns)[1][1]
    spec = GeneratedWorlds(1, nm, ns, seed=0)
    env = BatchedAuvEnv(cfg, spec, n, device="cuda:0", auto_reset=True)
    env.generate(spec, draws=torch.as_tensor(long_row[None], device="cuda:0"))
    host_long = _host(cfg, [long_row], nm, ns)
    t = R.read_tables(env)
    R.assert_world_tables(t, 0, host_long[0], nm, ns)
    p_long = int(t["POLY_CNT"][0])
    env.generate(spec, draws=torch.as_tensor(short_row[None], device="cuda:0"))
    host = _host(cfg, [short_row], nm, ns)
    t = R.read_tables(env)
    R.assert_world_tables(t, 0, host[0], nm, ns, wrap_heading=True)
    assert p_long > 15000 and int(t["POLY_CNT"][0]) == 8000
    ora = Oracle(make_config(cfg, auto_reset=True), n, pack_bank(host))
    _rollout_vs_oracle(env, ora, n, 30, np.repeat(_flipped(t, host), n))
    env.close()
