"""The affine feedback law of a closed-loop launch (auv_step_feedback / k_step_feedback, BatchedAuvEnv.step_feedback).

Per environment e there is a gain row G[e][2][8] in fp64.  For output j in {0 thrust, 1 rudder} of step t:

    x_c = OBS64[e][c] for c = 0..5   the six navigation columns as step t - 1 left them (after an auto-reset the new episode's
                                     reset row; for the launch's first step what the arrays hold)
    x_6 = 1.0
    x_7 = component j of the ring's action in slot (first_slot + t) % n_slots, as fp64; 0.0 when no ring is passed
    p_c = G[e][j][c] * x_c
    a_j = ((p_0 + p_1) + (p_2 + p_3)) + ((p_4 + p_5) + (p_6 + p_7))

in fp64, no fused multiply-add, exactly this association.  `a` is the step's action; the NaN rule and the clip to the action range
stay in the dynamics.  Column 7 = 1 makes the law a residual on an open-loop sequence, column 7 = 0 pure feedback; columns
0..6 = 0 with column 7 = 1 is the open-loop launch.

The navigation columns (environment.py:276-280, vessel.py:461-541; each clipped to [-1, 1]):

    0  surge velocity u            1  sway velocity v              2  yaw rate r
    3  look-ahead heading error: direction of the path at the look-ahead point - heading, wrapped to (-pi, pi]
    4  heading error: direction from the vessel TO the look-ahead point - heading, wrapped to (-pi, pi]
    5  cross-track error / 100: positive when the path lies to the left of the vessel (seen along the path)

`affine_action` is the host mirror the GPU tests step one-step launches with: NumPy fp64, the same association, bit for bit the
kernel's.

LiDAR sector inputs (auv_step_feedback_sectors / k_step_sector_feedback, step_feedback(..., sector_gains=)).  The same OBS64 row
carries L closeness columns from column 6 on: L = n_sensors in the plain configuration, n_sectors in the feasibility-pooled one.
A bounds table b[0..K], 1 <= K <= 16, 0 <= b[0] <= b[1] <= ... <= b[K] <= L, cuts them into sectors:

    z_k = max of OBS64[e][6 + i] over b[k] <= i < b[k+1]    the closeness of the nearest return in sector k, k < K: from the first
                                                            element on with m = v > m ? v : m (a closeness is never NaN);
                                                            +0.0 for an empty range
    z_k = +0.0 for K <= k < 16

Default bounds: plain, pooling.sector_starts(n_sectors, n_sensors_per_sector) -- the reference's own sigmoid partition, needs
n_sectors <= 16; pooled, arange(n_sectors + 1): z_k is the pooled column itself.  With sector gains H[e][2][16] in fp64, output j is

    s_j = the eight-term sum above (unchanged, same association)
    q_k = H[e][j][k] * z_k
    u_j = ((q_0 + q_1) + (q_2 + q_3)) + ((q_4 + q_5) + (q_6 + q_7))
    w_j = the same association over q_8 ... q_15
    a_j = s_j + (u_j + w_j)

fp64, no fused multiply-add, exactly this association.  `sector_action` is its host mirror.

One hidden layer (auv_step_feedback_hidden / k_step_hidden_feedback, step_feedback(..., hidden=)).  Per environment 16 hidden units
over 24 inputs, the same for both outputs:

    v_0..5  = x_0..5 above                  v_6, v_7 = the two components of the ring's action for the step (0.0 without a ring)
    v_8..23 = z_0..15 above (the same bounds table, the same maxima)

Hidden unit h has weights w_h[0..23] and a bias b_h:

    s = b_h;  for i = 0, 1, ..., 23 in this order:  s = s + (w_h[i] * v_i)        every product and every sum rounded once
    y_h = s > 0.0 ? s : +0.0                               activation 0, "relu" (a NaN gives +0.0)
    y_h = s > 1.0 ? 1.0 : (s < -1.0 ? -1.0 : s)            activation 1, "hardtanh" (a NaN passes on to the dynamics' NaN rule)

and with output weights V[2][16], r_k = V[j][k] * y_k:

    ha_j = ((r_0 + r_1) + (r_2 + r_3)) + ((r_4 + r_5) + (r_6 + r_7))       hb_j = the same association over r_8 ... r_15
    a_j  = (s_j + (u_j + w_j)) + (ha_j + hb_j)

The first bracket is the law with sector inputs, unchanged: the affine part stays as a skip connection, and V = 0 gives its values.
Smaller nets are rows of zeros.  The parameters travel as one block [N][16][28] (`pack_hidden`): row h = (w_h[0..23], b_h, V[0][h],
V[1][h], one pad word).  `hidden_action` is the host mirror.
"""
import numpy as np

N_INPUTS = 8
N_SECTOR_INPUTS = 16
N_HIDDEN = 16
N_HIDDEN_INPUTS = 24
HIDDEN_ROW = 28                                                 # doubles per hidden unit in the packed block: 24 weights, bias, V[0], V[1], pad
ACTIVATIONS = {"relu": 0, "hardtanh": 1}
COL_U, COL_V, COL_R, COL_LOOKAHEAD_ERR, COL_HEADING_ERR, COL_CROSS_TRACK, COL_BIAS, COL_RING = range(8)


def affine_action(obs64_nav, gains, ring_action=None) -> np.ndarray:
    """a[N, 2] of the law above.  obs64_nav: [N, >= 6] fp64 (the first six columns of OBS64 rows); gains: [N, 2, 8] or [2, 8]
    fp64; ring_action: [N, 2] (any float dtype, converted to fp64 as the kernels convert an action) or None (x_7 = 0)."""
    x = np.asarray(obs64_nav, dtype=np.float64)
    if x.ndim != 2 or x.shape[1] < 6:
        raise ValueError("obs64_nav must be [N, >= 6]")
    n = x.shape[0]
    g = np.asarray(gains, dtype=np.float64)
    if g.shape == (2, N_INPUTS):
        g = np.broadcast_to(g, (n, 2, N_INPUTS))
    if g.shape != (n, 2, N_INPUTS):
        raise ValueError("gains must be [%d, 2, 8] or [2, 8], got %s" % (n, g.shape))
    if ring_action is None:
        ring = np.zeros((n, 2), dtype=np.float64)
    else:
        ring = np.asarray(ring_action).astype(np.float64)
        if ring.shape != (n, 2):
            raise ValueError("ring_action must be [%d, 2]" % n)
    out = np.empty((n, 2), dtype=np.float64)
    for j in range(2):
        xs = np.empty((n, N_INPUTS), dtype=np.float64)
        xs[:, :6] = x[:, :6]
        xs[:, 6] = 1.0
        xs[:, 7] = ring[:, j]
        p = g[:, j, :] * xs                                    # eight products, each rounded once
        out[:, j] = ((p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3])) + ((p[:, 4] + p[:, 5]) + (p[:, 6] + p[:, 7]))
    return out


def _lidar_columns(cfg) -> int:
    """L: the LiDAR closeness columns of an OBS64 row."""
    v = cfg.vessel
    return int(v.n_sectors if v.feasibility_pooled else v.n_sensors)


def default_sector_bounds(cfg) -> np.ndarray:
    """The bounds table [K + 1] (int32) a closed-loop launch with sector inputs uses when its caller gives none: the reference's
    sigmoid sector partition over the beams (plain), one pooled column per sector (feasibility-pooled)."""
    from .pooling import sector_starts
    v = cfg.vessel
    if not v.use_lidar:
        raise ValueError("sector inputs need the LiDAR (use_lidar is off)")
    if not 1 <= v.n_sectors <= N_SECTOR_INPUTS:
        raise ValueError("default sector bounds need 1 <= n_sectors <= %d, got %d" % (N_SECTOR_INPUTS, v.n_sectors))
    if v.feasibility_pooled:
        return np.arange(v.n_sectors + 1, dtype=np.int32)
    return sector_starts(v.n_sectors, v.n_sensors_per_sector).astype(np.int32)


def check_sector_bounds(bounds, n_columns) -> np.ndarray:
    """`bounds` as an int32 array [K + 1], 1 <= K <= 16, ascending within [0, n_columns]; ValueError otherwise."""
    b = np.asarray(bounds)
    if b.ndim != 1 or not np.issubdtype(b.dtype, np.integer) or not 2 <= b.size <= N_SECTOR_INPUTS + 1:
        raise ValueError("sector_bounds must be a 1-D integer table of K + 1 entries, 1 <= K <= %d" % N_SECTOR_INPUTS)
    b = b.astype(np.int64)
    if b[0] < 0 or b[-1] > int(n_columns) or (np.diff(b) < 0).any():
        raise ValueError("sector_bounds must be ascending within [0, %d], got %s" % (int(n_columns), b.tolist()))
    return b.astype(np.int32)


def sector_inputs(obs64_rows, bounds) -> np.ndarray:
    """z[N, 16] of the module docstring.  obs64_rows: [N, 6 + L] fp64 (whole OBS64 rows, or their first 6 + L columns); bounds:
    [K + 1]."""
    x = np.asarray(obs64_rows, dtype=np.float64)
    if x.ndim != 2 or x.shape[1] < 6:
        raise ValueError("obs64_rows must be [N, >= 6]")
    b = check_sector_bounds(bounds, x.shape[1] - 6)
    z = np.zeros((x.shape[0], N_SECTOR_INPUTS), dtype=np.float64)
    for k in range(b.size - 1):
        lo, hi = int(b[k]), int(b[k + 1])
        if lo < hi:
            m = x[:, 6 + lo].copy()
            for i in range(lo + 1, hi):
                v = x[:, 6 + i]
                m = np.where(v > m, v, m)
            z[:, k] = m
    return z


def sector_action(obs64_rows, gains, sector_gains, bounds, ring_action=None) -> np.ndarray:
    """a[N, 2] of the law with sector inputs: NumPy fp64, the same association, bit for bit the kernel's.  sector_gains:
    [N, 2, 16] or [2, 16] fp64; the rest as affine_action's and sector_inputs'."""
    x = np.asarray(obs64_rows, dtype=np.float64)
    z = sector_inputs(x, bounds)
    n = x.shape[0]
    h = np.asarray(sector_gains, dtype=np.float64)
    if h.shape == (2, N_SECTOR_INPUTS):
        h = np.broadcast_to(h, (n, 2, N_SECTOR_INPUTS))
    if h.shape != (n, 2, N_SECTOR_INPUTS):
        raise ValueError("sector_gains must be [%d, 2, 16] or [2, 16], got %s" % (n, h.shape))
    s = affine_action(x, gains, ring_action)
    out = np.empty((n, 2), dtype=np.float64)
    for j in range(2):
        q = h[:, j, :] * z                                     # sixteen products, each rounded once
        u = ((q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3])) + ((q[:, 4] + q[:, 5]) + (q[:, 6] + q[:, 7]))
        w = ((q[:, 8] + q[:, 9]) + (q[:, 10] + q[:, 11])) + ((q[:, 12] + q[:, 13]) + (q[:, 14] + q[:, 15]))
        out[:, j] = s[:, j] + (u + w)
    return out


def pack_hidden(W1, b1, V) -> np.ndarray:
    """The parameter block [..., 16, 28] (fp64) of the hidden layer: row h = (W1[..., h, 0:24], b1[..., h], V[..., 0, h], V[..., 1, h],
    0.0).  W1: [..., 16, 24], b1: [..., 16], V: [..., 2, 16] with the same leading dimensions."""
    W1, b1, V = (np.asarray(a, dtype=np.float64) for a in (W1, b1, V))
    lead = W1.shape[:-2]
    if W1.shape[-2:] != (N_HIDDEN, N_HIDDEN_INPUTS) or b1.shape != lead + (N_HIDDEN,) or V.shape != lead + (2, N_HIDDEN):
        raise ValueError("W1 must be [..., 16, 24], b1 [..., 16] and V [..., 2, 16] with the same leading dimensions, got %s, %s, %s"
                         % (W1.shape, b1.shape, V.shape))
    out = np.zeros(lead + (N_HIDDEN, HIDDEN_ROW), dtype=np.float64)
    out[..., :N_HIDDEN_INPUTS] = W1
    out[..., 24] = b1
    out[..., 25] = V[..., 0, :]
    out[..., 26] = V[..., 1, :]
    return out


def hidden_inputs(obs64_rows, bounds, ring_action=None) -> np.ndarray:
    """v[N, 24] of the module docstring.  obs64_rows: [N, 6 + L] fp64; bounds: [K + 1]; ring_action: [N, 2] (converted to fp64 as
    the kernels convert an action) or None (v_6 = v_7 = 0)."""
    x = np.asarray(obs64_rows, dtype=np.float64)
    z = sector_inputs(x, bounds)
    n = x.shape[0]
    v = np.zeros((n, N_HIDDEN_INPUTS), dtype=np.float64)
    v[:, :6] = x[:, :6]
    if ring_action is not None:
        ring = np.asarray(ring_action).astype(np.float64)
        if ring.shape != (n, 2):
            raise ValueError("ring_action must be [%d, 2]" % n)
        v[:, 6:8] = ring
    v[:, 8:] = z
    return v


def _activation_code(activation) -> int:
    if isinstance(activation, str) and activation in ACTIVATIONS:
        return ACTIVATIONS[activation]
    raise ValueError("activation must be \"relu\" or \"hardtanh\", got %r" % (activation,))


def hidden_preactivations(obs64_rows, bounds, hidden, ring_action=None) -> np.ndarray:
    """s[N, 16] of the module docstring: the hidden units' sums before the activation, in the law's order of operations."""
    v = hidden_inputs(obs64_rows, bounds, ring_action)
    n = v.shape[0]
    p = np.asarray(hidden, dtype=np.float64)
    if p.shape == (N_HIDDEN, HIDDEN_ROW):
        p = np.broadcast_to(p, (n, N_HIDDEN, HIDDEN_ROW))
    if p.shape != (n, N_HIDDEN, HIDDEN_ROW):
        raise ValueError("hidden must be [%d, 16, 28] or [16, 28], got %s" % (n, p.shape))
    s = p[:, :, 24].copy()
    for i in range(N_HIDDEN_INPUTS):
        s = s + p[:, :, i] * v[:, i, None]                     # one product and one sum per input, in the order of the inputs
    return s


def hidden_action(obs64_rows, gains, sector_gains, bounds, hidden, activation="relu", ring_action=None) -> np.ndarray:
    """a[N, 2] of the law with the hidden layer: NumPy fp64, the same association, bit for bit the kernel's.  hidden: [N, 16, 28]
    or [16, 28] (pack_hidden); activation: "relu" or "hardtanh"; the rest as sector_action's."""
    code = _activation_code(activation)
    x = np.asarray(obs64_rows, dtype=np.float64)
    n = x.shape[0]
    s = hidden_preactivations(x, bounds, hidden, ring_action)
    p = np.broadcast_to(np.asarray(hidden, dtype=np.float64), (n, N_HIDDEN, HIDDEN_ROW))
    with np.errstate(invalid="ignore"):
        if code == 0:
            y = np.where(s > 0.0, s, 0.0)
        else:
            y = np.where(s > 1.0, 1.0, np.where(s < -1.0, -1.0, s))
        a = sector_action(x, gains, sector_gains, bounds, ring_action)
        out = np.empty((n, 2), dtype=np.float64)
        for j in range(2):
            r = p[:, :, 25 + j] * y                                # sixteen products, each rounded once
            ha = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
            hb = ((r[:, 8] + r[:, 9]) + (r[:, 10] + r[:, 11])) + ((r[:, 12] + r[:, 13]) + (r[:, 14] + r[:, 15]))
            out[:, j] = a[:, j] + (ha + hb)
    return out


def los_gains(thrust, k_heading, k_yaw_rate, k_cross_track=0.0) -> np.ndarray:
    """The line-of-sight autopilot as a [2, 8] gain row: constant thrust, rudder = -k_heading * e_psi - k_yaw_rate * r with the
    heading error e_psi = heading - direction to the look-ahead point.  Column 4 of the observation holds -e_psi (target - heading,
    see the module docstring), so its gain is +k_heading: a positive k_heading turns the vessel towards the look-ahead point, a
    positive k_yaw_rate damps the turn, a positive k_cross_track steers towards the path.
        thrust row:  [6] = thrust                                   (the bias column)
        rudder row:  [2] = -k_yaw_rate   [4] = +k_heading   [5] = +k_cross_track   (column 5 is the error / 100)
    every other entry 0, column 7 included: pure feedback (residual_gains turns it into a residual)."""
    g = np.zeros((2, N_INPUTS), dtype=np.float64)
    g[0, COL_BIAS] = thrust
    g[1, COL_R] = -float(k_yaw_rate)
    g[1, COL_HEADING_ERR] = float(k_heading)
    g[1, COL_CROSS_TRACK] = float(k_cross_track)
    return g


def residual_gains(base) -> np.ndarray:
    """A copy of `base` ([..., 2, 8]) with column 7 = 1: the ring's action is added to what the law gives."""
    g = np.array(base, dtype=np.float64, copy=True)
    if g.shape[-2:] != (2, N_INPUTS):
        raise ValueError("gains must be [..., 2, 8]")
    g[..., COL_RING] = 1.0
    return g


def check_feedback_args(n_envs, device, gains, n_steps, ring=None, first_slot=0, record=None):
    """What BatchedAuvEnv.step_feedback checks before the C call (torch tensors; no GPU needed to evaluate it).  Returns the
    gain table as a contiguous [N, 2, 8] fp64 tensor."""
    import torch
    if not isinstance(gains, torch.Tensor) or gains.dtype != torch.float64 or gains.device != device:
        raise ValueError("gains must be a float64 tensor on %s" % (device,))
    if tuple(gains.shape) == (2, N_INPUTS):
        gains = gains.expand(n_envs, 2, N_INPUTS)
    if tuple(gains.shape) != (n_envs, 2, N_INPUTS):
        raise ValueError("gains must have shape (%d, 2, 8) or (2, 8), got %s" % (n_envs, tuple(gains.shape)))
    gains = gains.contiguous()
    if int(n_steps) < 1 or int(n_steps) > 1024:
        raise ValueError("1 <= n_steps <= 1024")
    if ring is not None:
        if not isinstance(ring, torch.Tensor) or ring.dim() != 3 or tuple(ring.shape[1:]) != (n_envs, 2) or ring.device != device \
                or not ring.is_contiguous() or ring.dtype not in (torch.float32, torch.float64) or ring.shape[0] < 1:
            raise ValueError("ring must be a contiguous [slots, %d, 2] float32 / float64 tensor on %s" % (n_envs, device))
        if not 0 <= int(first_slot) < ring.shape[0]:
            raise ValueError("0 <= first_slot < %d" % ring.shape[0])
    elif int(first_slot) != 0:
        raise ValueError("first_slot without a ring")
    if not (record is None or record is True or (isinstance(record, str) and record == "reward")):
        raise ValueError("record must be None, True or \"reward\"")
    return gains


def check_sector_args(cfg, n_envs, device, sector_gains, sector_bounds=None):
    """What BatchedAuvEnv.step_feedback checks of its sector arguments before the C call (no GPU needed to evaluate it).  Returns
    (the sector gains as a contiguous [N, 2, 16] fp64 tensor, the bounds as an int32 array [K + 1])."""
    import torch
    if not cfg.vessel.use_lidar:
        raise ValueError("sector_gains need the LiDAR (use_lidar is off)")
    if not isinstance(sector_gains, torch.Tensor) or sector_gains.dtype != torch.float64 or sector_gains.device != device:
        raise ValueError("sector_gains must be a float64 tensor on %s" % (device,))
    if tuple(sector_gains.shape) == (2, N_SECTOR_INPUTS):
        sector_gains = sector_gains.expand(n_envs, 2, N_SECTOR_INPUTS)
    if tuple(sector_gains.shape) != (n_envs, 2, N_SECTOR_INPUTS):
        raise ValueError("sector_gains must have shape (%d, 2, 16) or (2, 16), got %s" % (n_envs, tuple(sector_gains.shape)))
    bounds = default_sector_bounds(cfg) if sector_bounds is None else check_sector_bounds(sector_bounds, _lidar_columns(cfg))
    return sector_gains.contiguous(), bounds


def check_hidden_args(n_envs, device, hidden, activation="relu", sector_gains=True):
    """What BatchedAuvEnv.step_feedback checks of its hidden-layer arguments before the C call (no GPU needed to evaluate it).
    `sector_gains`: what the caller passed as sector gains (None: the hidden layer needs them).  Returns (the block as a contiguous
    [N, 16, 28] fp64 tensor, the activation's code)."""
    import torch
    if sector_gains is None:
        raise ValueError("hidden needs sector_gains (zeros switch the affine sector terms off)")
    code = _activation_code(activation)
    if not isinstance(hidden, torch.Tensor) or hidden.dtype != torch.float64 or hidden.device != device:
        raise ValueError("hidden must be a float64 tensor on %s" % (device,))
    if tuple(hidden.shape) == (N_HIDDEN, HIDDEN_ROW):
        hidden = hidden.expand(n_envs, N_HIDDEN, HIDDEN_ROW)
    if tuple(hidden.shape) != (n_envs, N_HIDDEN, HIDDEN_ROW):
        raise ValueError("hidden must have shape (%d, 16, 28) or (16, 28), got %s" % (n_envs, tuple(hidden.shape)))
    return hidden.contiguous(), code
