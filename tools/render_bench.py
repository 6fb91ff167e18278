#!/usr/bin/env python3
"""What rendering costs, and whether the kernel earns its place (measured, not gated):
    python tools/render_bench.py [--out profiles/render] [--envs 4096] [--frames 64] [--size 600x720] [--zoom 1.5] [--eager-frames 2]
One process; the benchmark's polygons50 handle (4096 environments x 180 beams), stepped between frames.  HIP events on the
stream, warmed, median of --reps calls (measuring-on-mi355x: warm-up, repeats, a session that also does the step work).
    render_ms / frame_ms    one BatchedAuvEnv.render call of --frames frames of --size, and that per frame
    eager_frame_ms          THE YARDSTICK: the pixel rule restated in eager torch on the same GPU (eager_frames below: brute force over
                            every primitive, no cull, fp64), per frame, over the first --eager-frames frames of the same call; its
                            frames are compared with the kernel's, every pixel (differing_pixels must be 0)
    ratio                   eager_frame_ms / frame_ms: the kernel has to be no slower than tensor ops, i.e. ratio >= 1
    loop_us_plain / _render a loop of 256 env.step() calls on one chain, without and with a render call every 16 steps; per_render_us is
                            the difference per inserted call
    cull_share              share of (tile, segment) tests the tile cull removes: from the counter of the diagnostic build
                            (tools/build_variant.sh render_diag "-DAUV_RENDER_DIAG"), run in a child process; null if that build is absent
Writes README.md and render_bench.jsonl under --out."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_auv_amd import _capi  # noqa: E402
from gym_auv_amd import render as R  # noqa: E402
from gym_auv_amd.batched_env import BatchedAuvEnv  # noqa: E402
from gym_auv_amd.config import effective_reference_config  # noqa: E402
from gym_auv_amd.world import build_bank_parallel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/render")
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--size", default="600x720")
ap.add_argument("--zoom", type=float, default=1.5)
ap.add_argument("--eager-frames", type=int, default=2)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--diag-child", action="store_true", help="(internal) print the cull counter of the diagnostic build and exit")
args = ap.parse_args()
dev = torch.device("cuda:0")
H, W = (int(v) for v in args.size.split("x"))
DIAG_LIB = os.path.join(ROOT, "gym_auv_amd", "csrc_render_diag", "libauv_hip.so")


def seg_chunks(seg, n=64):
    return [seg[i:i + n] for i in range(0, len(seg), n)]


def line_lit(px, py, seg, h2):
    lit = torch.zeros_like(px, dtype=torch.bool)
    for s in seg_chunks(seg):
        ax, ay, bx, by = (s[:, k:k + 1] for k in range(4))
        ex, ey = bx - ax, by - ay
        dxa, dya = px[None, :] - ax, py[None, :] - ay
        len2 = ex * ex + ey * ey
        t = (dxa * ex + dya * ey) / len2
        t = torch.where(t < 0.0, 0.0, torch.where(t > 1.0, 1.0, t))
        t = torch.where(len2 > 0.0, t, 0.0)
        cx, cy = dxa - t * ex, dya - t * ey
        lit |= ((cx * cx + cy * cy) <= h2).any(dim=0)
    return lit


def ray_hit(px, py, seg, h2):
    best = torch.full(px.shape, -1, dtype=torch.int64, device=px.device)
    for c0 in range(0, len(seg), 32):
        s = seg[c0:c0 + 32]
        ax, ay, bx, by = (s[:, k:k + 1] for k in range(4))
        ex, ey = bx - ax, by - ay
        dxa, dya = px[None, :] - ax, py[None, :] - ay
        len2 = ex * ex + ey * ey
        t = (dxa * ex + dya * ey) / len2
        t = torch.where(t < 0.0, 0.0, torch.where(t > 1.0, 1.0, t))
        t = torch.where(len2 > 0.0, t, 0.0)
        cx, cy = dxa - t * ex, dya - t * ey
        lit = (cx * cx + cy * cy) <= h2
        idx = torch.where(lit, torch.arange(c0, c0 + len(s), device=px.device)[:, None], -1).max(dim=0).values
        best = torch.maximum(best, idx)
    return best


def fill_lit(px, py, seg):
    count = torch.zeros(px.shape, dtype=torch.int64, device=px.device)
    for s in seg_chunks(seg):
        ax, ay, bx, by = (s[:, k:k + 1] for k in range(4))
        strad = (ay > py[None, :]) != (by > py[None, :])
        xi = ax + (py[None, :] - ay) * (bx - ax) / (by - ay)
        count += (strad & (px[None, :] < xi)).sum(dim=0)
    return (count & 1) == 1


def eager_frames(cam, dyn_seg, ray_seg, ray_q, tables, pal, line_px=1.0):
    """The pixel rule of include/auv_hip.h in eager torch, fp64, brute force (no trail, no markers: the workload has none)."""
    out = []
    jj, ii = torch.meshgrid(torch.arange(W, dtype=torch.float64, device=dev), torch.arange(H, dtype=torch.float64, device=dev), indexing="xy")
    sx, sy = ((jj + 0.5) - 0.5 * W).reshape(-1), ((ii + 0.5) - 0.5 * H).reshape(-1)
    for b in range(len(cam)):
        x, y, m00, m01, m10, m11, zoom = (float(v) for v in cam[b, :7])
        px, py = x + (m00 * sx + m01 * sy), y + (m10 * sx + m11 * sy)
        h = 0.5 * line_px / zoom
        col = torch.zeros(H * W, dtype=torch.int64, device=dev)
        path, shapes = tables[b]
        col[line_lit(px, py, path, h * h)] = R.PATH
        for s in shapes:
            col[fill_lit(px, py, s)] = R.OBSTACLE
        n_mv = dyn_seg.shape[1] // 5 - 1
        for m in range(n_mv):
            col[fill_lit(px, py, dyn_seg[b, 5 * m:5 * m + 5])] = R.MOVER
        hit = ray_hit(px, py, ray_seg[b], h * h)
        vessel = fill_lit(px, py, dyn_seg[b, 5 * n_mv:])
        col[hit >= 0] = R.RAY_LO
        col[vessel] = R.VESSEL
        rgb = pal[col]
        q = ray_q[b].to(torch.int64)[hit.clamp(min=0)][:, None]
        mixed = torch.div(pal[R.RAY_LO][None, :] * (255 - q) + pal[R.RAY_HI][None, :] * q + 127, 255, rounding_mode="floor")
        rgb = torch.where(((hit >= 0) & ~vessel)[:, None], mixed, rgb)
        out.append(rgb.reshape(H, W, 3).to(torch.uint8))
    return torch.stack(out)


def timed(fn, reps, warm=3, between=None):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        if between:
            between()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms))


n_worlds = 2 * args.envs
bank = build_bank_parallel("polygon_world", 1000 + np.arange(n_worlds), procs=16, n_polygons=50)
cfg = effective_reference_config(use_lidar=True)
env = BatchedAuvEnv(cfg, bank, args.envs, device=dev, auto_reset=True)
env.reset()
gen = torch.Generator(device=dev).manual_seed(0)
lo, hi = torch.tensor([0.0, -0.15], device=dev), torch.tensor([1.0, 0.15], device=dev)
actions = lo + (hi - lo) * torch.rand((args.envs, 2), generator=gen, device=dev)


def steps(k):
    for _ in range(k):
        env.step(actions)


steps(64)
idx = list(range(min(args.frames, args.envs)))

if args.diag_child:
    lib = _capi.load_library()
    assert hasattr(lib, "auv_render_diag"), "needs the -DAUV_RENDER_DIAG build (AUV_HIP_LIB)"
    out2 = (C.c_uint64 * 2)()
    lib.auv_render_diag(env._h, out2)
    env.render(envs=idx, size=(H, W), zoom=args.zoom)
    lib.auv_render_diag(env._h, out2)
    print(json.dumps(dict(offered=int(out2[0]), kept=int(out2[1]))))
    sys.exit(0)

row = dict(envs=args.envs, frames=len(idx), size=[H, W], zoom=args.zoom, library_sha256=hashlib.sha256(open(_capi.LIB_PATH, "rb").read()).hexdigest())
row["render_ms"], row["render_ms_min"] = timed(lambda: env.render(envs=idx, size=(H, W), zoom=args.zoom), args.reps, between=lambda: steps(4))
row["frame_ms"] = row["render_ms"] / len(idx)

# the yardstick: eager torch on the first frames of one call, compared with the kernel's frames
E = max(1, min(args.eager_frames, len(idx)))
frames, geo = env.render(envs=idx, size=(H, W), zoom=args.zoom, return_geometry=True)
widx = env.read("WORLD_IDX").cpu().numpy()
tabs = []
for e in idx[:E]:
    t = R.world_tables(bank, int(widx[e]))
    tabs.append((torch.as_tensor(R.polyline_segments(t.path_xy), device=dev), [torch.as_tensor(np.ascontiguousarray(s), device=dev) for s in t.shapes]))
pal = torch.as_tensor(R.DEFAULT_PALETTE.astype(np.int64), device=dev)
eager = lambda: eager_frames(geo["cam"][:E], geo["dyn_seg"][:E], geo["ray_seg"][:E], geo["ray_q"][:E], tabs, pal)   # noqa: E731
ref = eager()
row["eager_frames"] = E
row["differing_pixels"] = int((ref != frames[:E]).any(dim=3).sum())
ms, _ = timed(eager, max(3, args.reps // 3), warm=1)
row["eager_frame_ms"] = ms / E
row["ratio"] = row["eager_frame_ms"] / row["frame_ms"]

# a render call every 16 steps of the one-chain step() loop
def loop(with_render):
    for k in range(256):
        env.step(actions)
        if with_render and k % 16 == 15:
            env.render(envs=idx, size=(H, W), zoom=args.zoom)


plain, _ = timed(lambda: loop(False), 5, warm=1)
withr, _ = timed(lambda: loop(True), 5, warm=1)
row["loop_us_plain"], row["loop_us_render"] = plain * 1e3, withr * 1e3
row["per_render_us"] = (withr - plain) * 1e3 / 16

row["cull_share"] = None
if os.path.exists(DIAG_LIB):
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--diag-child", "--envs", str(args.envs), "--frames", str(args.frames),
                            "--size", args.size, "--zoom", str(args.zoom)], env=dict(os.environ, AUV_HIP_LIB=DIAG_LIB),
                           capture_output=True, text=True, timeout=600)
    last = [ln for ln in child.stdout.splitlines() if ln.startswith("{")]
    if child.returncode == 0 and last:
        c = json.loads(last[-1])
        row.update(cull_offered=c["offered"], cull_kept=c["kept"], cull_share=1.0 - c["kept"] / max(1, c["offered"]))
    else:
        row["cull_error"] = (child.stderr or child.stdout)[-400:]

os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, "render_bench.jsonl"), "a") as f:
    f.write(json.dumps(row) + "\n")
with open(os.path.join(args.out, "README.md"), "w") as f:
    f.write("# Rendering on the device: what it costs\n\n`python tools/render_bench.py` (its docstring defines every column).  %d frames of %d x %d "
            "at zoom %g from the polygons50 handle (%d environments x 180 beams), stepped between calls.\n\n" % (len(idx), H, W, args.zoom, args.envs))
    f.write("| figure | value |\n|---|---|\n")
    for k in ("render_ms", "frame_ms", "eager_frame_ms", "ratio", "differing_pixels", "eager_frames", "loop_us_plain", "loop_us_render",
              "per_render_us", "cull_share"):
        v = row.get(k)
        f.write("| %s | %s |\n" % (k, "not measured" if v is None else ("%.4g" % v if isinstance(v, float) else v)))
    f.write("\nThe bar: `ratio` (eager torch per frame / kernel per frame, same session) must be at least 1, and `differing_pixels` 0.  "
            "The eager restatement is timed on the first `eager_frames` frames of the call and compared per frame.\n")
print(json.dumps(row))
env.close()
