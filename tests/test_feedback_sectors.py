"""CPU: the LiDAR sector inputs of the closed-loop launch's law (gym_auv_amd/feedback.py: default_sector_bounds, sector_inputs,
sector_action, check_sector_bounds, check_sector_args), the export of auv_step_feedback_sectors and the signature of
BatchedAuvEnv.step_feedback.  No GPU."""
import inspect
import os

import numpy as np
import pytest
import torch

from gym_auv_amd import _capi
from gym_auv_amd.config import effective_reference_config
from gym_auv_amd.feedback import (N_SECTOR_INPUTS, affine_action, check_feedback_args, check_sector_args, check_sector_bounds,
                                  default_sector_bounds, los_gains, sector_action, sector_inputs)
from gym_auv_amd.pooling import sector_starts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def _cfg(ns=9, nps=20, pooled=False, lidar=True):
    cfg = effective_reference_config(use_lidar=lidar)
    cfg.vessel.n_sectors, cfg.vessel.n_sensors_per_sector = ns, nps
    cfg.vessel.sensor_use_feasibility_pooling = pooled
    return cfg


def test_default_bounds_are_the_reference_partition_or_the_pooled_identity():
    assert N_SECTOR_INPUTS == 16
    b = default_sector_bounds(_cfg(9, 20))
    assert b.dtype == np.int32 and np.array_equal(b, sector_starts(9, 20)) and b[0] == 0 and b[-1] == 180
    assert len(set(np.diff(b).tolist())) > 1                       # the sigmoid partition is uneven
    assert np.array_equal(default_sector_bounds(_cfg(4, 8)), sector_starts(4, 8))
    assert np.array_equal(default_sector_bounds(_cfg(9, 20, pooled=True)), np.arange(10))
    with pytest.raises(ValueError):
        default_sector_bounds(_cfg(17, 4))                         # more sectors than inputs
    with pytest.raises(ValueError):
        default_sector_bounds(_cfg(lidar=False))


def test_sector_inputs_on_hand_made_rows():
    rows = np.zeros((3, 6 + 10))
    rows[:, :6] = 9.0                                              # the navigation columns are not looked at
    rows[0, 6:] = [0.1, 0.7, 0.2, 0.0, 0.0, 0.3, 0.9, 0.4, 0.0, 0.5]
    rows[1, 6:] = [0.0] * 10
    rows[2, 6:] = [1.0, 0.0, 0.0, 0.25, 0.5, 0.125, 0.0, 0.0, 0.75, 0.0]
    # K = 4: [0, 3), the empty [3, 3), [3, 9), [9, 10)
    z = sector_inputs(rows, [0, 3, 3, 9, 10])
    assert z.shape == (3, 16) and z.dtype == np.float64
    assert np.array_equal(z[:, :4], [[0.7, 0.0, 0.9, 0.5], [0.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.75, 0.0]])
    assert not z[:, 4:].any() and not np.signbit(z).any()          # K < 16: the rest is +0.0, and so is an empty range
    # sensors left out at both ends
    assert np.array_equal(sector_inputs(rows, [2, 2, 5, 8])[:, :3], [[0.0, 0.2, 0.9], [0.0, 0.0, 0.0], [0.0, 0.5, 0.125]])
    # the pooled identity bounds: z_k is the column itself
    assert np.array_equal(sector_inputs(rows, np.arange(11))[:, :10], rows[:, 6:])
    # the running maximum starts from the range's FIRST element (not from 0): a range of negative numbers keeps its largest
    neg = np.zeros((1, 9))
    neg[0, 6:] = [-3.0, -2.0, -5.0]
    assert sector_inputs(neg, [0, 3])[0, 0] == -2.0
    # sixteen sectors of one column each
    wide = np.zeros((1, 6 + 16))
    wide[0, 6:] = np.arange(16) / 16.0
    assert np.array_equal(sector_inputs(wide, np.arange(17))[0], np.arange(16) / 16.0)


def test_bounds_checks():
    assert check_sector_bounds([0, 4, 8], 8).dtype == np.int32
    assert np.array_equal(check_sector_bounds((2, 2, 5, 8), 32), [2, 2, 5, 8])
    assert len(check_sector_bounds(np.arange(17), 16)) == 17
    for bad, L in (([0], 8), ([], 8), (np.arange(18), 32), ([0, 5, 4], 8), ([-1, 4], 8), ([0, 9], 8), ([[0, 1]], 8), ([0.0, 4.0], 8)):
        with pytest.raises(ValueError):
            check_sector_bounds(bad, L)


def test_sector_action_keeps_the_association():
    x = np.zeros((1, 6 + 16))
    x[0, 6:] = 1.0
    g = np.zeros((2, 8))
    g[:, 6] = 0.5                                                  # s_j = 0.5
    b = np.arange(17)
    h = np.zeros((2, 16))
    # thrust, q = (1e16, 1, 1, 1, -1e16, 0, ...): pairwise ((1e16 + 1) + (1 + 1)) + ((-1e16 + 0) + 0) = (1e16 + 2) - 1e16 = 2
    # (1e16 + 1 rounds to 1e16, 1e16 + 2 is exact); left to right (((1e16 + 1) + 1) + 1) - 1e16 = 0
    h[0, :5] = [1e16, 1.0, 1.0, 1.0, -1e16]
    # rudder: the second group, and u + w before s: w = (1e16 + -1e16) + (3 + 0) = 3 in q_8..q_11
    h[1, 8:12] = [1e16, -1e16, 3.0, 0.0]
    h[1, 0] = 1e-20                                                # u = 1e-20: (u + w) = 3 exactly, then s + 3
    a = sector_action(x, g, h, b)
    assert a.shape == (1, 2) and a[0, 0] == 0.5 + 2.0 and a[0, 1] == 3.5
    left_to_right = 0.5 + float(np.cumsum(h[0] * x[0, 6:])[-1])
    assert left_to_right != a[0, 0]                                # the association matters on these inputs
    # a_j = s_j + (u_j + w_j), not (s_j + u_j) + w_j: s = 1, u = 1e16, w = -1e16
    g2 = np.zeros((2, 8))
    g2[0, 6] = 1.0
    h2 = np.zeros((2, 16))
    h2[0, 0], h2[0, 8] = 1e16, -1e16
    assert sector_action(x, g2, h2, b)[0, 0] == 1.0                # ((1 + 1e16) - 1e16 would be 0)
    # per-environment tables and the [2, 16] form agree; the ring goes through
    rs = np.random.RandomState(3)
    xs = rs.uniform(0, 1, (5, 6 + 16))
    hs, gs, ring = rs.normal(size=(2, 16)), rs.normal(size=(5, 2, 8)), rs.normal(size=(5, 2)).astype(np.float32)
    one = sector_action(xs, gs, hs, b, ring)
    assert np.array_equal(one, sector_action(xs, gs, np.broadcast_to(hs, (5, 2, 16)), b, ring))
    z = sector_inputs(xs, b)
    q = hs[0] * z
    want = affine_action(xs, gs, ring)[:, 0] + ((((q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3])) + ((q[:, 4] + q[:, 5]) + (q[:, 6] + q[:, 7])))
                                                + (((q[:, 8] + q[:, 9]) + (q[:, 10] + q[:, 11])) + ((q[:, 12] + q[:, 13]) + (q[:, 14] + q[:, 15]))))
    assert np.array_equal(one[:, 0].view(np.uint64), want.view(np.uint64))
    with pytest.raises(ValueError):
        sector_action(xs, gs, np.zeros((2, 15)), b)


def test_zero_sector_gains_return_the_affine_action():
    rs = np.random.RandomState(5)
    x = rs.uniform(-1, 1, (7, 6 + 32))
    x[:, 6:] = np.abs(x[:, 6:])
    g, ring = rs.normal(size=(7, 2, 8)), rs.normal(size=(7, 2))
    a = sector_action(x, g, np.zeros((2, 16)), sector_starts(4, 8), ring)
    assert np.array_equal(a, affine_action(x, g, ring))            # as numbers (s + 0.0 may turn -0.0 into +0.0)


def test_sector_argument_checks():
    n = 4
    h = torch.zeros((n, 2, 16), dtype=torch.float64)
    cfg = _cfg(4, 8)
    sg, b = check_sector_args(cfg, n, CPU, h)
    assert sg.shape == (n, 2, 16) and sg.is_contiguous() and np.array_equal(b, sector_starts(4, 8))
    sg, b = check_sector_args(cfg, n, CPU, torch.ones((2, 16), dtype=torch.float64), (2, 2, 5, 8))
    assert sg.shape == (n, 2, 16) and sg.is_contiguous() and b.tolist() == [2, 2, 5, 8] and b.dtype == np.int32
    _, b = check_sector_args(_cfg(9, 20, pooled=True), n, CPU, h)
    assert b.tolist() == list(range(10))
    bad = [dict(sector_gains=h.float()), dict(sector_gains=h[:, :, :15]), dict(sector_gains=h[:2]), dict(sector_gains=h.numpy()),
           dict(sector_gains=h, sector_bounds=(0, 33)), dict(sector_gains=h, sector_bounds=(0, 5, 4)), dict(sector_gains=h, sector_bounds=(-1, 4)),
           dict(sector_gains=h, sector_bounds=(0,)), dict(sector_gains=h, sector_bounds=tuple(range(18)))]
    for kw in bad:
        with pytest.raises(ValueError):
            check_sector_args(cfg, n, CPU, **kw)
    with pytest.raises(ValueError):
        check_sector_args(_cfg(9, 20, pooled=True), n, CPU, h, (0, 10))       # pooled: L = n_sectors = 9
    with pytest.raises(ValueError):
        check_sector_args(_cfg(4, 8, lidar=False), n, CPU, h)                  # use_lidar is off
    with pytest.raises(ValueError):
        check_sector_args(_cfg(17, 4), n, CPU, h)                              # no default bounds for 17 sectors ...
    assert len(check_sector_args(_cfg(17, 4), n, CPU, h, (0, 30, 68))[1]) == 3     # ... the caller's own are fine


def test_present_check_feedback_args_calls_answer_as_before():
    n = 4
    g = torch.zeros((n, 2, 8), dtype=torch.float64)
    assert check_feedback_args(n, CPU, g, 3).shape == (n, 2, 8)
    assert check_feedback_args(n, CPU, torch.as_tensor(los_gains(0.5, 1.0, 0.5)), 1024, None, 0, "reward").shape == (n, 2, 8)
    ring = torch.zeros((3, n, 2))
    assert check_feedback_args(n, CPU, g, 2, ring, 2, True) is not None
    for args in ((n, CPU, g.float(), 2), (n, CPU, g, 0), (n, CPU, g, 1025), (n, CPU, g, 2, ring, 3), (n, CPU, g, 2, None, 1),
                 (n, CPU, g, 2, None, 0, "obs"), (n, CPU, g[:, :, :7], 2)):
        with pytest.raises(ValueError):
            check_feedback_args(*args)
    assert list(inspect.signature(check_feedback_args).parameters) == ["n_envs", "device", "gains", "n_steps", "ring", "first_slot", "record"]


def test_the_new_call_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "auv_hip.h")).read()
    assert "int auv_step_feedback_sectors(" in hdr and "auv_step_feedback_sectors" in _capi.EXPORTED_SYMBOLS
    lib = _capi.load_library()
    assert len(lib.auv_step_feedback_sectors.argtypes) == len(lib.auv_step_feedback.argtypes) + 3
    from gym_auv_amd.batched_env import BatchedAuvEnv
    p = inspect.signature(BatchedAuvEnv.step_feedback).parameters
    assert p["sector_gains"].default is None and p["sector_bounds"].default is None
    src = open(os.path.join(ROOT, "gym_auv_amd", "csrc", "k_step_fused.hip")).read()
    assert "k_step_sector_feedback(AuvDev dk," in src             # the descriptor is the kernel's first argument (AUV_KERNARG_DESC)
