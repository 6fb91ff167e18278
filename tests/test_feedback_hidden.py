"""CPU: the hidden layer of the closed-loop launch's law (gym_auv_amd/feedback.py: pack_hidden, hidden_inputs, hidden_action,
check_hidden_args), the export of auv_step_feedback_hidden and the signature of BatchedAuvEnv.step_feedback.  No GPU.

`hidden_action` is held against an independent restatement of the law: plain Python floats (IEEE fp64, one rounding per
operation), one environment at a time, the association written out -- compared as uint64 bit patterns."""
import inspect
import os

import numpy as np
import pytest
import torch

from gym_auv_amd import _capi
from gym_auv_amd.feedback import (N_HIDDEN, N_HIDDEN_INPUTS, check_hidden_args, hidden_action, hidden_inputs, pack_hidden,
                                  sector_action)
from gym_auv_amd.pooling import sector_starts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def _restated(row, G, H, bounds, W1, b1, V, activation, ring):
    """The law for ONE environment in plain Python floats.  row: the OBS64 row (list); G [2][8], H [2][16], W1 [16][24], b1 [16],
    V [2][16] nested lists; ring: (r0, r1) or None."""
    z = []
    for k in range(16):
        if k + 1 < len(bounds) and bounds[k] < bounds[k + 1]:
            m = row[6 + bounds[k]]
            for i in range(bounds[k] + 1, bounds[k + 1]):
                m = row[6 + i] if row[6 + i] > m else m
            z.append(m)
        else:
            z.append(0.0)
    r = (0.0, 0.0) if ring is None else (float(ring[0]), float(ring[1]))
    v = list(row[:6]) + [r[0], r[1]] + z
    y = []
    for h in range(16):
        s = b1[h]
        for i in range(24):
            s = s + (W1[h][i] * v[i])
        if activation == "relu":
            y.append(s if s > 0.0 else 0.0)
        else:
            y.append(1.0 if s > 1.0 else (-1.0 if s < -1.0 else s))
    out = []
    for j in range(2):
        x = list(row[:6]) + [1.0, r[j]]
        p = [G[j][c] * x[c] for c in range(8)]
        sj = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))
        q = [H[j][k] * z[k] for k in range(16)]
        u = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]))
        w = ((q[8] + q[9]) + (q[10] + q[11])) + ((q[12] + q[13]) + (q[14] + q[15]))
        rr = [V[j][k] * y[k] for k in range(16)]
        ha = ((rr[0] + rr[1]) + (rr[2] + rr[3])) + ((rr[4] + rr[5]) + (rr[6] + rr[7]))
        hb = ((rr[8] + rr[9]) + (rr[10] + rr[11])) + ((rr[12] + rr[13]) + (rr[14] + rr[15]))
        out.append((sj + (u + w)) + (ha + hb))
    return out


def _random_case(seed, n, L, scale=1.0):
    rs = np.random.RandomState(seed)
    x = rs.uniform(-1, 1, (n, 6 + L))
    x[:, 6:] = np.abs(x[:, 6:]) * (rs.uniform(size=(n, L)) < 0.5)       # closeness columns: many exact zeros
    return dict(x=x, G=rs.normal(size=(n, 2, 8)), H=rs.normal(size=(n, 2, 16)), W1=rs.normal(0, scale, (n, 16, 24)),
                b1=rs.normal(0, scale, (n, 16)), V=rs.normal(size=(n, 2, 16)), ring=rs.normal(size=(n, 2)).astype(np.float32))


@pytest.mark.parametrize("activation", ["relu", "hardtanh"])
@pytest.mark.parametrize("bounds", [tuple(sector_starts(9, 20).tolist()), (2, 2, 5, 8), tuple(range(17))])
def test_hidden_action_is_the_restated_law_bit_for_bit(activation, bounds):
    """Random rows; (2, 2, 5, 8) has an empty first sector and twelve padding sectors."""
    n, L = 40, 180
    c = _random_case(11, n, L, scale=2.0 if activation == "hardtanh" else 1.0)
    for ring in (c["ring"], None):
        got = hidden_action(c["x"], c["G"], c["H"], bounds, pack_hidden(c["W1"], c["b1"], c["V"]), activation, ring)
        want = np.array([_restated(c["x"][e].tolist(), c["G"][e].tolist(), c["H"][e].tolist(), bounds, c["W1"][e].tolist(),
                                   c["b1"][e].tolist(), c["V"][e].tolist(), activation, None if ring is None else ring[e]) for e in range(n)])
        assert got.shape == (n, 2) and got.dtype == np.float64
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    # the [16, 28] form: every environment alike
    one = pack_hidden(c["W1"][0], c["b1"][0], c["V"][0])
    assert np.array_equal(hidden_action(c["x"], c["G"], c["H"], bounds, one, activation).view(np.uint64),
                          hidden_action(c["x"], c["G"], c["H"], bounds, np.broadcast_to(one, (n, 16, 28)), activation).view(np.uint64))


def test_a_nan_preactivation_is_zero_under_relu_and_passes_under_hard_tanh():
    c = _random_case(12, 3, 32)
    b = tuple(sector_starts(4, 8).tolist())
    c["W1"][1, 5, 3] = np.nan                                          # environment 1, unit 5
    c["b1"][2, 9] = np.inf                                             # environment 2, unit 9: +inf
    c["W1"][2, 9, 0], c["x"][2, 0] = 1.0, 0.25
    blk = pack_hidden(c["W1"], c["b1"], c["V"])
    for activation in ("relu", "hardtanh"):
        got = hidden_action(c["x"], c["G"], c["H"], b, blk, activation, c["ring"])
        want = np.array([_restated(c["x"][e].tolist(), c["G"][e].tolist(), c["H"][e].tolist(), b, c["W1"][e].tolist(), c["b1"][e].tolist(),
                                   c["V"][e].tolist(), activation, c["ring"][e]) for e in range(3)])
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64))
        assert np.isfinite(got[0]).all()
        # relu: the NaN unit gives +0.0, the action stays a number; hard tanh: the NaN reaches both outputs
        assert np.isnan(got[1]).all() == (activation == "hardtanh") and np.isnan(got[1]).any() == (activation == "hardtanh")
        # +inf: relu keeps it, hard tanh saturates at 1
        assert np.isinf(got[2]).all() == (activation == "relu")


def test_zero_output_weights_give_the_sector_action():
    c = _random_case(13, 9, 180)
    b = sector_starts(9, 20)
    for activation in ("relu", "hardtanh"):
        a = hidden_action(c["x"], c["G"], c["H"], b, pack_hidden(c["W1"], c["b1"], np.zeros((9, 2, 16))), activation, c["ring"])
        assert np.array_equal(a, sector_action(c["x"], c["G"], c["H"], b, c["ring"]))      # as numbers (a + 0.0 may turn -0.0 into +0.0)


def test_one_relu_unit_gates_a_rudder_term_on_a_sector():
    """rudder = 2 * relu(z_3 - 0.5): nothing until the nearest return in sector 3 is closer than 0.5, then proportional -- not an
    affine function of z_3: the second difference over three equally spaced inputs is not zero."""
    b = np.arange(17)
    W1, b1, V = np.zeros((16, 24)), np.zeros(16), np.zeros((2, 16))
    W1[11, 8 + 3], b1[11], V[1, 11] = 1.0, -0.5, 2.0                  # unit 11 (the second group sum) looks at v_11 = z_3
    blk = pack_hidden(W1, b1, V)
    rows = np.zeros((3, 6 + 16))
    rows[:, 6 + 3] = [0.25, 0.5, 0.75]
    a = hidden_action(rows, np.zeros((2, 8)), np.zeros((2, 16)), b, blk)
    assert a[:, 0].tolist() == [0.0, 0.0, 0.0] and a[:, 1].tolist() == [0.0, 0.0, 0.5]
    assert a[0, 1] - 2.0 * a[1, 1] + a[2, 1] != 0.0                    # an affine law has a zero second difference
    # the affine sector law on the same rows IS affine in z_3
    H = np.zeros((2, 16))
    H[1, 3] = 2.0
    s = sector_action(rows, np.zeros((2, 8)), H, b)
    assert s[0, 1] - 2.0 * s[1, 1] + s[2, 1] == 0.0
    # the other sectors are not looked at
    rows[:, 6 + 4] = 1.0
    assert np.array_equal(hidden_action(rows, np.zeros((2, 8)), np.zeros((2, 16)), b, blk), a)


def test_hidden_inputs_and_the_packed_layout():
    assert (N_HIDDEN, N_HIDDEN_INPUTS) == (16, 24)
    rs = np.random.RandomState(14)
    W1, b1, V = rs.normal(size=(5, 16, 24)), rs.normal(size=(5, 16)), rs.normal(size=(5, 2, 16))
    blk = pack_hidden(W1, b1, V)
    assert blk.shape == (5, 16, 28) and blk.dtype == np.float64 and blk.flags["C_CONTIGUOUS"]
    assert blk.strides[-2] == 224                                      # a row is 224 bytes: every row 16-byte aligned
    for e, h in ((0, 0), (3, 7), (4, 15)):
        assert np.array_equal(blk[e, h, :24], W1[e, h]) and blk[e, h, 24] == b1[e, h]
        assert blk[e, h, 25] == V[e, 0, h] and blk[e, h, 26] == V[e, 1, h] and blk[e, h, 27] == 0.0
    assert pack_hidden(W1[0], b1[0], V[0]).shape == (16, 28)
    for bad in ((W1[:, :15], b1, V), (W1, b1[:, :15], V), (W1, b1, V[:, :, :15]), (W1, b1[0], V), (W1[0], b1, V)):
        with pytest.raises(ValueError):
            pack_hidden(*bad)
    rows = np.zeros((2, 6 + 10))
    rows[:, :6] = [[1, 2, 3, 4, 5, 6], [-1, -2, -3, -4, -5, -6]]
    rows[0, 6:] = [0.1, 0.7, 0.2, 0.0, 0.0, 0.3, 0.9, 0.4, 0.0, 0.5]
    v = hidden_inputs(rows, [0, 3, 3, 9, 10], np.array([[0.5, -0.25], [1.5, 2.0]], dtype=np.float32))
    assert v.shape == (2, 24)
    assert v[0].tolist() == [1, 2, 3, 4, 5, 6, 0.5, -0.25, 0.7, 0.0, 0.9, 0.5] + [0.0] * 12
    assert v[1].tolist() == [-1, -2, -3, -4, -5, -6, 1.5, 2.0] + [0.0] * 16
    assert hidden_inputs(rows, [0, 10])[:, 6:8].tolist() == [[0.0, 0.0], [0.0, 0.0]]        # no ring
    with pytest.raises(ValueError):
        hidden_action(rows, np.zeros((2, 8)), np.zeros((2, 16)), [0, 10], np.zeros((16, 27)))
    with pytest.raises(ValueError):
        hidden_action(rows, np.zeros((2, 8)), np.zeros((2, 16)), [0, 10], np.zeros((16, 28)), "tanh")


def test_hidden_argument_checks():
    n = 4
    hd = torch.zeros((n, 16, 28), dtype=torch.float64)
    sg = torch.zeros((n, 2, 16), dtype=torch.float64)
    t, code = check_hidden_args(n, CPU, hd, "relu", sg)
    assert t.shape == (n, 16, 28) and t.is_contiguous() and code == 0
    t, code = check_hidden_args(n, CPU, torch.ones((16, 28), dtype=torch.float64), "hardtanh", sg)
    assert t.shape == (n, 16, 28) and t.is_contiguous() and code == 1 and bool((t == 1).all())
    bad = [dict(hidden=hd, sector_gains=None),                          # hidden without sector gains
           dict(hidden=hd.float(), sector_gains=sg), dict(hidden=hd.numpy(), sector_gains=sg), dict(hidden=hd[:, :, :27], sector_gains=sg),
           dict(hidden=hd[:2], sector_gains=sg), dict(hidden=hd[:, :15], sector_gains=sg), dict(hidden=hd.to("meta"), sector_gains=sg),
           dict(hidden=hd, sector_gains=sg, activation="tanh"), dict(hidden=hd, sector_gains=sg, activation=0),
           dict(hidden=hd, sector_gains=sg, activation=None)]
    for kw in bad:
        with pytest.raises(ValueError):
            check_hidden_args(n, CPU, **kw)


def test_the_new_call_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "auv_hip.h")).read()
    assert "int auv_step_feedback_hidden(" in hdr and "auv_step_feedback_hidden" in _capi.EXPORTED_SYMBOLS
    assert _capi.ABI_VERSION == 5                                   # the new entry is an addition: the version stays
    lib = _capi.load_library()
    assert len(lib.auv_step_feedback_hidden.argtypes) == len(lib.auv_step_feedback_sectors.argtypes) + 2
    assert lib.auv_step_feedback_hidden.argtypes[:len(lib.auv_step_feedback_sectors.argtypes)] == lib.auv_step_feedback_sectors.argtypes
    from gym_auv_amd.batched_env import BatchedAuvEnv
    p = inspect.signature(BatchedAuvEnv.step_feedback).parameters
    assert p["hidden"].default is None and p["activation"].default == "relu"
    assert list(p)[:9] == ["self", "gains", "n_steps", "ring", "first_slot", "record", "record_actions", "sector_gains", "sector_bounds"]
    src = open(os.path.join(ROOT, "gym_auv_amd", "csrc", "k_step_fused.hip")).read()
    assert "k_step_hidden_feedback(AuvDev dk," in src             # the descriptor is the kernel's first argument (AUV_KERNARG_DESC)
