"""CPU: running normalisation (gym_auv_amd/normalize.py, csrc/k16_policy_norm.hip) -- the new exports in header and binding, the NumPy
mirrors of the kernels against a plain float64 restatement of stable-baselines' RunningMeanStd and of VecNormalize's return recursion,
the edge rows, and the state's round trip.

Tolerances.  The fold and the return statistics are fp64 in the mirror and in the restatement, by different associations: 1e-12 relative
(the data keep the deviation within a few orders of the mean).  The f32 tile partials folded in fp64 against float64 batch moments: a
16-term f32 sum errs by at most 16 x 2^-24 ~ 1e-6 of the largest term; 1e-5 relative to the column's deviation leaves ten-fold slack."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("auv_policy_act_norm", "auv_policy_act_norm_arch", "auv_policy_rollout_norm", "auv_policy_rollout_norm_arch", "auv_norm_rows",
       "auv_norm_fold", "auv_norm_returns")


# ------------------------------------------------------------------------------ symbols
def test_the_new_exports_are_in_header_and_binding_and_the_abi_is_still_5():
    from gym_auv_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "auv_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _capi.load_library()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert re.search(r"#define\s+AUV_ABI_VERSION\s+5\b", hdr) and _capi.ABI_VERSION == 5 and lib.auv_abi_version() == 5
    s = _capi.AuvPolicyNorm                                # the plain io block first, then table, part, pcnt, part_ld, part_base, clip_obs
    assert s.io.offset == 0 and s.table.offset == C.sizeof(_capi.AuvPolicyIO) and s.part.offset == s.table.offset + 8
    assert s.pcnt.offset == s.part.offset + 8 and s.part_ld.offset == s.pcnt.offset + 8 and s.part_base.offset == s.part_ld.offset + 4
    assert s.clip_obs.offset == s.part_base.offset + 4 and C.sizeof(s) == C.sizeof(_capi.AuvPolicyIO) + 40


def test_struct_sizes_match_the_header_and_the_io_block_is_unchanged(tmp_path):
    from gym_auv_amd import _capi
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu %%d\\n", '
                   'sizeof(auv_policy_io_t), sizeof(auv_policy_norm_t), offsetof(auv_policy_norm_t, table), offsetof(auv_policy_norm_t, part), '
                   'offsetof(auv_policy_norm_t, pcnt), offsetof(auv_policy_norm_t, part_ld), offsetof(auv_policy_norm_t, clip_obs), '
                   'AUV_ABI_VERSION);return 0;}\n' % os.path.join(ROOT, "include", "auv_hip.h"))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    io, size, o_table, o_part, o_pcnt, o_ld, o_clip, abi = map(int, subprocess.check_output([str(exe)]).split())
    s = _capi.AuvPolicyNorm
    assert io == 184 == C.sizeof(_capi.AuvPolicyIO) and abi == 5          # (184: what sizeof(auv_policy_io_t) was before this struct came)
    assert (C.sizeof(s), s.table.offset, s.part.offset, s.pcnt.offset, s.part_ld.offset, s.clip_obs.offset) == (size, o_table, o_part, o_pcnt, o_ld, o_clip)


# ------------------------------------------------------------------------------ plain float64 restatements of stable-baselines
class RefRMS:
    """stable-baselines' RunningMeanStd: batch mean / variance / count merged into (mean, var, count), float64."""

    def __init__(self, shape):
        self.mean, self.var, self.count = np.zeros(shape), np.ones(shape), 1e-4

    def update(self, x):
        x = np.asarray(x, dtype=np.float64)
        bm, bv, bc = x.mean(axis=0), x.var(axis=0), x.shape[0]
        delta = bm - self.mean
        tot = self.count + bc
        m2 = self.var * self.count + bv * bc + np.square(delta) * self.count * bc / tot
        self.mean, self.var, self.count = self.mean + delta * bc / tot, m2 / tot, tot


def _ref_returns(R, Dn, ret, rms, gamma):
    """VecNormalize's recursion over a stored rollout: ret = ret * gamma + r, update, ret[done] = 0 -- one update per step."""
    ret = np.array(ret, dtype=np.float64)
    for t in range(R.shape[0]):
        ret = ret * gamma + R[t].astype(np.float64)
        rms.update(ret)
        ret[Dn[t] != 0] = 0.0
    return ret


def _init_mom(D):
    from gym_auv_amd.normalize import INIT_COUNT
    mom = np.zeros((D, 3))
    mom[:, 0], mom[:, 2] = INIT_COUNT, INIT_COUNT
    return mom


def _rows(D, n, seed):
    rs = np.random.RandomState(seed)
    scale = rs.uniform(0.1, 30.0, D)
    shift = rs.uniform(-5.0, 5.0, D)
    return (rs.standard_normal((n, D)) * scale + shift).astype(np.float32)


@pytest.mark.parametrize("D", [15, 186])
def test_fold_mirror_against_float64_running_mean_std(D):
    from gym_auv_amd.normalize import fold_moments, slice_partials
    bounds = [0, 24, 40]                                   # two slices: the first ends in a ragged tile of 8, the second is one full tile
    ref, mom, mom64 = RefRMS(D), _init_mom(D), _init_mom(D)
    for rollout in range(2):
        batches = [_rows(D, 40, 10 * rollout + t) for t in range(3)]
        parts = [slice_partials(x, bounds) for x in batches]
        part = np.concatenate([p for p, _ in parts])
        pcnt = np.concatenate([c for _, c in parts])
        assert pcnt.tolist() == [16, 8, 16] * 3
        # (a) fp64 statistics: exact float64 partials through the mirror's merge order, against one RunningMeanStd update per rollout
        allx = np.concatenate(batches).astype(np.float64)
        exact, at = np.zeros_like(part, dtype=np.float64), 0
        for t, x in enumerate(batches):
            for lo, hi in ((0, 16), (16, 24), (24, 40)):
                xs = x[lo:hi].astype(np.float64)
                exact[at, 0], exact[at, 1] = xs.mean(0), ((xs - xs.mean(0)) ** 2).sum(0)
                at += 1
        ref.update(allx)
        mom64, _ = _fold64(exact, pcnt, mom64)
        sd = np.sqrt(ref.var)
        assert np.abs(mom64[:, 1] - ref.mean).max() <= 1e-12 * np.abs(ref.mean).max()
        assert np.abs(mom64[:, 2] / mom64[:, 0] - ref.var).max() <= 1e-12 * ref.var.max()
        assert abs(mom64[0, 0] - ref.count) <= 1e-12 * ref.count
        # (b) the f32 tile partials folded in fp64
        mom, table = fold_moments(part, pcnt, mom, 1e-8)
        assert (np.abs(mom[:, 1] - ref.mean) <= 1e-5 * sd).all()
        assert (np.abs(np.sqrt(mom[:, 2] / mom[:, 0]) - sd) <= 1e-5 * sd).all()
        assert table.dtype == np.float32 and np.array_equal(table[:, 0], mom[:, 1].astype(np.float32))
        assert np.array_equal(table[:, 1], (1.0 / np.sqrt(mom[:, 2] / mom[:, 0] + 1e-8)).astype(np.float32))


def _fold64(part64, pcnt, mom):
    """fold_moments' merge order on float64 partials (fold_moments itself rounds its input to float32)."""
    from gym_auv_amd import normalize as nz
    D = part64.shape[2]
    n = np.repeat(pcnt.astype(np.float64)[:, None], D, axis=1)
    batch = nz._merge_lanes(n, part64[:, 0], part64[:, 1])
    rn, rm, rM = nz._merge((mom[:, 0], mom[:, 1], mom[:, 2]), batch)
    return np.stack([rn, rm, rM], axis=1), None


def test_return_mirror_against_float64_vecnormalize_recursion():
    from gym_auv_amd.normalize import INIT_COUNT, return_pass
    rs = np.random.RandomState(3)
    T, N, gamma = 7, 40, 0.99
    ref = RefRMS(())
    ret_ref, ret = np.zeros(N), np.zeros(N)
    rmom = np.array([INIT_COUNT, 0.0, INIT_COUNT])
    for call in range(2):
        R = (rs.standard_normal((T, N)) * 3.0 + 0.2).astype(np.float32)
        R[rs.uniform(size=(T, N)) < 0.05] = -5000.0        # the collision term beside step rewards of order 1
        Dn = (rs.uniform(size=(T, N)) < 0.2).astype(np.float32)
        ret_ref = _ref_returns(R, Dn, ret_ref, ref, gamma)
        ret, rmom, Rs = return_pass(R, Dn, ret, rmom, gamma, 1e-8, 10.0)
        assert np.abs(ret - ret_ref).max() <= 1e-12 * max(1.0, np.abs(ret_ref).max())
        assert abs(rmom[0] - ref.count) <= 1e-12 * ref.count
        assert abs(rmom[1] - ref.mean) <= 1e-12 * np.sqrt(ref.var)
        assert abs(rmom[2] / rmom[0] - ref.var) <= 1e-12 * ref.var
        want = np.clip(R.astype(np.float64) / np.sqrt(ref.var + 1e-8), -10.0, 10.0)
        assert Rs.dtype == np.float32 and np.abs(Rs - want).max() <= 4e-7 * 10.0      # (two f32 roundings of values up to the clip)
        # (a collision's -5000 sits a few deviations out: a tighter clip_reward cuts it, exactly)
        _, _, Rc = return_pass(R, Dn, ret, rmom, gamma, 1e-8, 1.0, update=False)
        assert (Rc == -1.0).any() and np.abs(Rc).max() == 1.0 and np.array_equal(Rc, np.clip(Rs, -1.0, 1.0))


# ------------------------------------------------------------------------------ edge rows
def test_a_constant_column_a_clipped_value_and_a_one_row_tile():
    from gym_auv_amd.normalize import fold_moments, norm_rows, slice_partials, tile_moments
    x = _rows(5, 17, 1)
    x[:, 2] = 3.25                                          # a constant column
    part, pcnt = slice_partials(x, [0, 17])                 # a full tile and a ONE-ROW tile
    assert pcnt.tolist() == [16, 1]
    assert not part[:, 1, 2].any() and (part[:, 0, 2] == np.float32(3.25)).all()
    m1, M21 = tile_moments(x[16:17])
    assert np.array_equal(m1, x[16]) and not M21.any()     # one row: the mean is the row, M2 = 0
    with pytest.raises(ValueError):
        tile_moments(x)
    mom = np.zeros((5, 3))                                  # count 0: the batch alone
    mom, table = fold_moments(part, pcnt, mom, 1e-8)
    assert mom[2, 0] == 17.0 and mom[2, 1] == 3.25 and mom[2, 2] == 0.0
    assert table[2, 1] == np.float32(1.0 / np.sqrt(1e-8))   # inv_std limited by eps alone
    # the constant column normalises to 0; a value far out hits the clip exactly, on both sides
    y = norm_rows(x, table, 10.0)
    assert not y[:, 2].any()
    z = x.copy()
    z[0, 0], z[1, 0] = 1e6, -1e6
    yz = norm_rows(z, table, 10.0)
    assert yz[0, 0] == 10.0 and yz[1, 0] == -10.0 and np.array_equal(yz[2:], y[2:])
    # empty slots are skipped, wherever they lie
    part2 = np.concatenate([np.full((1, 2, 5), 7.0, np.float32), part[:1], np.full((70, 2, 5), -3.0, np.float32), part[1:]])
    pcnt2 = np.concatenate([[0], pcnt[:1], np.zeros(70, np.int32), pcnt[1:]]).astype(np.int32)
    mom2, _ = fold_moments(part2, pcnt2, np.zeros((5, 3)), 1e-8)
    assert np.allclose(mom2, mom, rtol=1e-14, atol=0) and mom2[0, 0] == 17.0


def test_done_at_the_first_and_the_last_step_and_ret_carried_across_two_calls():
    from gym_auv_amd.normalize import INIT_COUNT, return_pass
    gamma = 0.5
    R = np.array([[1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [4.0, 4.0, 4.0]], dtype=np.float32)          # [T = 3, N = 3]
    Dn = np.zeros((3, 3), dtype=np.float32)
    Dn[0, 1] = 1.0                                          # environment 1: done at t = 0
    Dn[2, 2] = 1.0                                          # environment 2: done at t = T - 1
    rmom0 = np.array([INIT_COUNT, 0.0, INIT_COUNT])
    ret, rmom, _ = return_pass(R, Dn, np.zeros(3), rmom0, gamma, 1e-8, 10.0)
    # env 0: 1, 2.5, 5.25 carried on; env 1: 1 (taken BEFORE the zeroing), then 2, 5; env 2: as env 0, zeroed behind the last step
    assert ret.tolist() == [5.25, 5.0, 0.0]
    taken = np.array([1, 2.5, 5.25, 1, 2, 5, 1, 2.5, 5.25])
    assert abs(rmom[0] - (9 + INIT_COUNT)) < 1e-12 and abs(rmom[1] - taken.sum() / (9 + INIT_COUNT)) < 1e-12
    # the second call starts from the carried returns
    ret2, rmom2, _ = return_pass(R, np.zeros_like(Dn), ret, rmom, gamma, 1e-8, 10.0)
    assert ret2.tolist() == [0.5 * (0.5 * (0.5 * 5.25 + 1) + 2) + 4, 0.5 * (0.5 * (0.5 * 5.0 + 1) + 2) + 4, 5.25]
    # update = False: nothing moves, the rewards are scaled by the deviation as it stands
    ret3, rmom3, Rs = return_pass(R, Dn, ret2, rmom2, gamma, 1e-8, 10.0, update=False)
    assert np.array_equal(ret3, ret2) and np.array_equal(rmom3, rmom2)
    assert np.array_equal(Rs, np.clip(R / np.float32(np.sqrt(rmom2[2] / rmom2[0] + 1e-8)), -10, 10).astype(np.float32))


# ------------------------------------------------------------------------------ state
def test_initial_state_training_off_and_the_state_dict_round_trip_are_bit_identical():
    import torch
    from gym_auv_amd.normalize import RunningNorm
    a = RunningNorm(15, 0.99)
    assert a.obs_mom[:, 0].eq(1e-4).all() and a.obs_mom[:, 1].eq(0).all() and a.obs_mom[:, 2].eq(1e-4).all()      # mean 0, variance 1, count 1e-4
    assert a.ret_mom.tolist() == [1e-4, 0.0, 1e-4]
    assert a.table[:, 0].eq(0).all() and a.table[:, 1].eq(float(np.float32(1.0 / np.sqrt(1.0 + 1e-8)))).all()
    assert (a.clip_obs, a.clip_reward, a.eps) == (10.0, 10.0, 1e-8) and a.training and a.norm_obs and a.norm_reward
    g = torch.Generator().manual_seed(0)
    a.obs_mom.copy_(torch.rand((15, 3), generator=g, dtype=torch.float64) + 0.5)
    a.ret_mom.copy_(torch.rand(3, generator=g, dtype=torch.float64) + 0.5)
    a.table.copy_(torch.rand((15, 2), generator=g))
    a.bind(40, 3, [(0, 24), (24, 16)], "cpu")
    assert a.part_base == [0, 2] and a.part_ld == 3 and tuple(a.part.shape) == (9, 2, 15) and tuple(a.pcnt.shape) == (9,)
    a.ret.copy_(torch.rand(40, generator=g, dtype=torch.float64))
    before = a.state_dict()
    # training = False: fold() and the reward pass' update are not run (no launch is made: this runs without a GPU)
    a.training = False
    a.pcnt.fill_(16)
    a.fold()
    after = a.state_dict()
    for k in ("obs_mom", "ret_mom", "table", "ret"):
        assert torch.equal(before[k], after[k]), k
    assert int(a.pcnt.sum()) == 16 * 9                      # (the slots were not consumed either)
    # round trip into a fresh object, bound or not
    for bound in (False, True):
        b = RunningNorm(15, 0.99)
        if bound:
            b.bind(40, 3, [(0, 24), (24, 16)], "cpu")
        table_ptr = b.table.data_ptr()
        b.load_state_dict(before)
        assert b.table.data_ptr() == table_ptr             # in place: launches hold the table's address
        again = b.state_dict()
        for k in ("obs_mom", "ret_mom", "table", "ret"):
            assert torch.equal(before[k], again[k]) and again[k].dtype == before[k].dtype, k
    with pytest.raises(ValueError):
        RunningNorm(16, 0.99).load_state_dict(before)


def test_fused_actor_critic_refuses_frames_and_bf16_with_normalize():
    """The checks run before the environment is touched: a stand-in with the two attributes they read is enough."""
    import torch
    import torch.nn as nn
    from gym_auv_amd.normalize import RunningNorm
    from gym_auv_amd.policy import FusedActorCritic

    def mlp(i, out):
        return nn.Sequential(nn.Linear(i, 256), nn.Tanh(), nn.Linear(256, 128), nn.Tanh(), nn.Linear(128, 64), nn.Tanh(), nn.Linear(64, out))
    env = types.SimpleNamespace(obs_dim=26, device="cpu")
    net = nn.Module()
    net.pi, net.v, net.log_std = mlp(52, 2), mlp(52, 1), nn.Parameter(torch.zeros(2))
    with pytest.raises(ValueError, match="normalize"):
        FusedActorCritic(net, env, rollout=4, frames=2, normalize=RunningNorm(26, 0.99))
    net.pi, net.v = mlp(26, 2), mlp(26, 1)
    with pytest.raises(ValueError, match="normalize"):
        FusedActorCritic(net, env, rollout=4, bf16=True, normalize=RunningNorm(26, 0.99))
    with pytest.raises(ValueError, match="columns"):
        FusedActorCritic(net, env, rollout=4, normalize=RunningNorm(20, 0.99))
