"""Rendering: the NumPy mirror of the device renderer's pixel rule, the default palette and the argument checks.

`BatchedAuvEnv.render` draws frames on the device (csrc/k10_render.hip, two launches).  `render_reference` restates the pixel
rule of include/auv_hip.h (auv_render) in NumPy, operation for operation in IEEE fp64, brute force over every primitive with no
cull: fed with the geometry a call returned (`return_geometry=True`) and the bank's host tables it gives the call's frames bit
for bit.  It is the contract the kernel is tested against, not a product path.
"""
from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np

VIEWS = {"heading_up": 0, "north_up": 1}
MAX_SIDE = 4096
MAX_FRAMES = 65535

# background, path, trail, obstacle, marker, mover, beam lo (far), beam hi (close), vessel
DEFAULT_PALETTE = np.array([[12, 28, 48], [88, 200, 120], [240, 220, 90], [168, 172, 180], [255, 255, 255],
                            [200, 110, 200], [40, 90, 160], [255, 70, 50], [255, 150, 30]], dtype=np.uint8)
BG, PATH, TRAIL, OBSTACLE, MARKER, MOVER, RAY_LO, RAY_HI, VESSEL = range(9)


class WorldTables(NamedTuple):
    """The static tables of one world the renderer reads: the dense path polyline and every static obstacle's boundary."""
    path_xy: np.ndarray             # [P, 2]
    shapes: List[np.ndarray]        # per static obstacle [nseg, 4] ax, ay, bx, by


def world_tables(bank: Dict[str, np.ndarray], w: int) -> WorldTables:
    """World `w` of a packed bank (world.pack_bank)."""
    p0, p1 = int(bank["poly_off"][w]), int(bank["poly_off"][w + 1])
    k0, k1 = int(bank["obs_off"][w]), int(bank["obs_off"][w + 1])
    seg = np.asarray(bank["seg"], dtype=np.float64).reshape(-1, 4)
    shapes = [seg[off:off + n] for kind, off, n, _ in np.asarray(bank["obs_meta"]).reshape(-1, 4)[k0:k1] if kind != 2]
    return WorldTables(np.asarray(bank["poly_xy"], dtype=np.float64).reshape(-1, 2)[p0:p1], shapes)


def check_palette(palette) -> np.ndarray:
    if palette is None:
        return DEFAULT_PALETTE
    p = np.asarray(palette)
    if p.shape != (9, 3) or p.dtype.kind not in "ui" or p.min() < 0 or p.max() > 255:
        raise ValueError("palette: uint8 [9][3] expected (background, path, trail, obstacle, marker, mover, beam lo, beam hi, vessel)")
    return np.ascontiguousarray(p, dtype=np.uint8)


def check_render_args(n_envs: int, envs, size, zoom, view, line_px=1.0) -> np.ndarray:
    """The refusals of auv_render, raised as ValueError before anything reaches the library; returns the index list."""
    idx = np.arange(min(n_envs, 16), dtype=np.int64) if envs is None else np.asarray(envs).reshape(-1)
    if idx.dtype.kind not in "iu":
        raise ValueError("render: envs must be integers")
    B = len(idx)
    H, W = (int(size[0]), int(size[1]))
    if B < 1 or H < 1 or W < 1:
        raise ValueError("render: B = %d, H = %d, W = %d: each must be >= 1" % (B, H, W))
    if H > MAX_SIDE or W > MAX_SIDE or B > MAX_FRAMES:
        raise ValueError("render: H = %d, W = %d (at most %d), B = %d (at most %d)" % (H, W, MAX_SIDE, B, MAX_FRAMES))
    if (idx < 0).any() or (idx >= n_envs).any():
        raise ValueError("render: an index of %s is outside the handle's %d environments" % (idx.tolist(), n_envs))
    for name, v in (("zoom", zoom), ("line_px", line_px)):
        if not (np.isfinite(float(v)) and float(v) > 0.0):
            raise ValueError("render: %s = %r must be finite and > 0" % (name, v))
    if view not in VIEWS:
        raise ValueError("render: view %r is not one of %s" % (view, sorted(VIEWS)))
    return idx.astype(np.int32)


_CHUNK = 32       # segments looked at per NumPy pass ([_CHUNK, H * W] temporaries)


def _line_chunk(px, py, s, h2):
    with np.errstate(all="ignore"):
        ax, ay, bx, by = (s[:, k:k + 1] for k in range(4))
        ex, ey = bx - ax, by - ay
        dxa, dya = px[None, :] - ax, py[None, :] - ay
        len2 = ex * ex + ey * ey
        dot = dxa * ex + dya * ey
        t = dot / len2
        t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
        t = np.where(len2 > 0.0, t, 0.0)
        cx, cy = dxa - t * ex, dya - t * ey
        return ((cx * cx + cy * cy) <= h2).any(axis=0)


def _line_lit(px, py, seg, h2):
    """[H*W] bool: some segment of seg [n, 4] within h of the pixel centre (the line rule)."""
    lit = np.zeros(px.shape, dtype=bool)
    for c0 in range(0, len(seg), _CHUNK):
        lit |= _line_chunk(px, py, seg[c0:c0 + _CHUNK], h2)
    return lit


def _ray_hit(px, py, seg, h2):
    """[H*W] int: the highest index of a lit segment, -1 where none."""
    best = np.full(px.shape, -1, dtype=np.int64)
    for i in range(len(seg)):
        best[_line_lit(px, py, seg[i:i + 1], h2)] = i
    return best


def _fill_lit(px, py, seg):
    """[H*W] bool: an odd number of the shape's boundary segments crossed (the even-odd rule)."""
    count = np.zeros(px.shape, dtype=np.int64)
    with np.errstate(all="ignore"):
        for c0 in range(0, len(seg), _CHUNK):
            s = seg[c0:c0 + _CHUNK]
            ax, ay, bx, by = (s[:, k:k + 1] for k in range(4))
            strad = (ay > py[None, :]) != (by > py[None, :])
            xi = ax + (py[None, :] - ay) * (bx - ax) / (by - ay)
            count += (strad & (px[None, :] < xi)).sum(axis=0)
    return (count & 1) == 1


def polyline_segments(pts: np.ndarray) -> np.ndarray:
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    return np.concatenate([pts[:-1], pts[1:]], axis=1) if len(pts) > 1 else np.zeros((0, 4))


def trail_rows(trail: np.ndarray) -> int:
    """Rows of a trail [L, 2] before its first row with a NaN."""
    bad = np.isnan(trail).any(axis=1)
    return int(np.argmax(bad)) if bad.any() else len(trail)


def render_reference(cam, dyn_seg, ray_seg, ray_q, worlds: Sequence[WorldTables], trail=None, markers=None, palette=None,
                     H: int = 600, W: int = 720, line_px: float = 1.0) -> np.ndarray:
    """uint8 [B, H, W, 3]: the frames auv_render paints from this geometry, by the pixel rule alone (no cull).
    cam [B, 8], dyn_seg [B, 5 Mmax + 5, 4], ray_seg [B, S, 4], ray_q [B, S], worlds: B WorldTables, trail [B, L, 2] or None,
    markers [B, M, 3] or None."""
    pal = check_palette(palette).astype(np.int64)
    cam = np.asarray(cam, dtype=np.float64).reshape(-1, 8)
    B = len(cam)
    dyn_seg = np.asarray(dyn_seg, dtype=np.float64).reshape(B, -1, 4)
    ray_seg = np.asarray(ray_seg, dtype=np.float64).reshape(B, -1, 4)
    ray_q = np.asarray(ray_q).reshape(B, -1).astype(np.int64)
    out = np.zeros((B, H, W, 3), dtype=np.uint8)
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    sx, sy = ((jj + 0.5) - 0.5 * W).reshape(-1), ((ii + 0.5) - 0.5 * H).reshape(-1)
    for b in range(B):
        x, y, m00, m01, m10, m11, zoom = cam[b, :7]
        px, py = x + (m00 * sx + m01 * sy), y + (m10 * sx + m11 * sy)
        h = 0.5 * float(line_px) / zoom
        h2 = h * h
        col = np.zeros(H * W, dtype=np.int64)
        col[_line_lit(px, py, polyline_segments(worlds[b].path_xy), h2)] = PATH
        if trail is not None:
            tr = np.asarray(trail[b], dtype=np.float64).reshape(-1, 2)
            col[_line_lit(px, py, polyline_segments(tr[:trail_rows(tr)]), h2)] = TRAIL
        for shape in worlds[b].shapes:
            col[_fill_lit(px, py, np.asarray(shape, dtype=np.float64))] = OBSTACLE
        if markers is not None:
            for mx, my, mr in np.asarray(markers[b], dtype=np.float64).reshape(-1, 3):
                dx, dy = px - mx, py - my
                col[(dx * dx + dy * dy) <= mr * mr] = MARKER
        n_mv = len(dyn_seg[b]) // 5 - 1
        for m in range(n_mv):
            col[_fill_lit(px, py, dyn_seg[b, 5 * m:5 * m + 5])] = MOVER
        hit = _ray_hit(px, py, ray_seg[b], h2)
        col[hit >= 0] = RAY_LO
        vessel = _fill_lit(px, py, dyn_seg[b, 5 * n_mv:5 * n_mv + 5])
        col[vessel] = VESSEL
        rgb = pal[col]
        rays = (hit >= 0) & ~vessel
        q = ray_q[b][np.maximum(hit, 0)][:, None]
        mixed = (pal[RAY_LO][None, :] * (255 - q) + pal[RAY_HI][None, :] * q + 127) // 255
        rgb = np.where(rays[:, None], mixed, rgb)
        out[b] = rgb.reshape(H, W, 3).astype(np.uint8)
    return out


def tile_frames(frames: np.ndarray) -> np.ndarray:
    """[B, H, W, 3] -> one image of ceil(sqrt(B)) columns, as stable-baselines' tile_images lays a VecEnv's frames out."""
    B, H, W, C = frames.shape
    cols = int(np.ceil(np.sqrt(B)))
    rows = int(np.ceil(B / cols))
    big = np.zeros((rows * cols, H, W, C), dtype=frames.dtype)
    big[:B] = frames
    return big.reshape(rows, cols, H, W, C).transpose(0, 2, 1, 3, 4).reshape(rows * H, cols * W, C)


def write_ppm(path: str, frame: np.ndarray) -> None:
    """A binary PPM (P6) of one [H, W, 3] uint8 frame: readable by any image viewer, no image library needed."""
    frame = np.ascontiguousarray(frame, dtype=np.uint8)
    if frame.ndim != 3 or frame.shape[2] != 3:
        raise ValueError("write_ppm: [H, W, 3] expected")
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (frame.shape[1], frame.shape[0]))
        f.write(frame.tobytes())
