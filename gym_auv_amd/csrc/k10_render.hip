// K10 — batched rgb_array frames of environments, rendered where their state lives (the reference draws one environment
// with pygame on the host: BaseEnvironment.render, gym_auv/environment.py:410-437; a vessel-centred top view).
//
// Two launches per call, on the caller's stream:
//   k10_frame_geometry   ONE WAVE PER FRAME.  What moves, in world coordinates: the camera (cam[8] = vessel x, y, the 2 x 2
//                        matrix pixel offset -> metres, zoom, view), every mover's pentagon (MoverSegs: the sweep's own
//                        vertices) and the vessel's, one segment per LiDAR beam and its colour weight q, and the length of
//                        the NaN-terminated trail.
//   k10_raster           ONE 256-THREAD WORKGROUP PER 16 x 16 TILE, a thread per pixel.  Per layer: the layer's primitives
//                        (path chunks, trail segments, obstacles, markers, movers, beams, the vessel) are culled against the
//                        tile's bounding circle, the survivors compacted in order into an LDS list (wave prefix sums by DPP,
//                        the four waves' totals through LDS), their segments staged in LDS 256 at a time, and every thread
//                        runs the pixel rule of the layer over the staged batch.
// The pixel rule (restated bit for bit by gym_auv_amd/render.py: render_reference) -- fp64, no contraction, no square root:
//   p = (x, y) + M (j + 0.5 - W / 2, i + 0.5 - H / 2)
//   line      e = b - a, t = clamp(((p - a) . e) / (e . e), 0, 1) (0 for a == b), lit when |p - a - t e|^2 <= h^2, h = line_px / 2 / zoom
//   filled    odd number of boundary segments with (ay > py) != (by > py) and px < ax + (py - ay) * (bx - ax) / (by - ay)
//   disc      (px - x)^2 + (py - y)^2 <= r^2
// Layers in painting order: path, trail, static obstacles, markers, movers, beams (the highest lit beam index wins), vessel.
// The cull is conservative by a slack (1e-6 m) that is ~1e6 times the rounding of its own distances, so no primitive that
// could light a pixel of the tile is ever dropped: the image does not depend on it (the mirror culls nothing).
#include "auv_device.h"
#include "auv_mover_segs.h"
#include "auv_render.h"

namespace {

#define K10_TILE 16
#define K10_BLOCK (K10_TILE * K10_TILE)
#define K10_WAVES (K10_BLOCK / AUV_WAVE)
#define K10_SLACK 1e-6

__global__ void __launch_bounds__(AUV_WAVE) k10_frame_geometry(const AuvDev d, const AuvRenderArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int e = auv_uniform(a.env_idx[b]);
  const size_t n = (size_t)d.n;
  const int S = d.cfg.n_sensors, m_max = d.m_max;
  const EnvDesc ed = d.env_desc[e];
  const double x = d.state[e], y = d.state[n + e], psi = d.state[2 * n + e];
  double s, c;
  sincos(psi, &s, &c);
  if (lane == 0) {
    double* cam = a.cam + (size_t)b * 8;
    cam[0] = x, cam[1] = y;
    if (a.view == AUV_VIEW_HEADING_UP) {      // screen up = the heading, screen right = the heading turned clockwise
      cam[2] = s / a.zoom, cam[3] = -c / a.zoom;
      cam[4] = -c / a.zoom, cam[5] = -s / a.zoom;
    } else {                                  // north up: world x to the right, world y upwards
      cam[2] = 1.0 / a.zoom, cam[3] = 0.0;
      cam[4] = 0.0, cam[5] = -1.0 / a.zoom;
    }
    cam[6] = a.zoom, cam[7] = (double)a.view;
  }
  double4* dyn = a.dyn_seg + (size_t)b * (5 * m_max + 5);
  for (int m = lane; m < m_max; m += AUV_WAVE) {
    if (m < ed.M) {
      const double4 st = d.mover[(size_t)e * m_max + m];
      const double wd = d.mv_param[ed.m0 + m].x;
      double ms_, mc;
      sincos(st.z, &ms_, &mc);
      if (fabs(mc) < 2.5e-16) mc = 0.0;       // (as the sweep's phase A: shapely.affinity.rotate snaps tiny cos / sin)
      if (fabs(ms_) < 2.5e-16) ms_ = 0.0;
      const MoverSegs ms = mover_segs(make_double4(mc, ms_, st.x, st.y), wd);
      for (int k = 0; k < AUV_MOVER_NSEG; k++) dyn[5 * m + k] = ms[k];
    } else {
      for (int k = 0; k < AUV_MOVER_NSEG; k++) dyn[5 * m + k] = make_double4(0.0, 0.0, 0.0, 0.0);
    }
  }
  if (lane < 5) {
    // the vessel's pentagon: body-frame vertices turned by (c, s), the values the camera matrix is made of
    const double w = d.cfg.vessel_width;
    double vx[2], vy[2];
    for (int q = 0; q < 2; q++) {
      const int k = (lane + q) % 5;
      const double bx = (k <= 1) ? -w / 2 : (k == 3 ? 3.0 / 2 * w : w / 2);
      const double by = (k == 0 || k == 4) ? -w / 2 : (k == 3 ? 0.0 : w / 2);
      vx[q] = x + (c * bx - s * by);
      vy[q] = y + (s * bx + c * by);
    }
    dyn[5 * m_max + lane] = make_double4(vx[0], vy[0], vx[1], vy[1]);
  }
  const double R = d.cfg.sensor_range;
  const bool stored = d.cfg.use_lidar && d.pool_ns == 0;   // the per-beam closeness columns exist (pooled: the linear rule on the range)
  for (int i = lane; i < S; i += AUV_WAVE) {
    const double2 bt = d.beam_cs[i];
    const double dx = c * bt.x - s * bt.y, dy = s * bt.x + c * bt.y;
    const double r = d.cfg.use_lidar ? d.lidar_d[(size_t)e * S + i] : 0.0;   // LiDAR off: nothing was measured, no beam is drawn (a dot under the vessel)
    a.ray_seg[(size_t)b * S + i] = make_double4(x, y, x + dx * r, y + dy * r);
    double cl = stored ? d.obs64[(size_t)e * (6 + S) + 6 + i] : 1 - auv_clip(r / R, 0.0, 1.0);
    cl = cl > 0.0 ? cl : 0.0;
    const int q = (int)(cl * 255 + 0.5);
    a.ray_q[(size_t)b * S + i] = (uint8_t)(q > 255 ? 255 : q);
  }
  // rows of the trail before its first NaN row
  int len = 0;
  if (a.trail) {
    len = a.L;
    const double2* tr = (const double2*)a.trail + (size_t)b * a.L;
    for (int base = 0; base < a.L; base += AUV_WAVE) {
      const int i = base + lane;
      bool bad = false;
      if (i < a.L) {
        const double2 p = tr[i];
        bad = (p.x != p.x) || (p.y != p.y);
      }
      const unsigned long long mask = __ballot(bad);
      if (mask) {
        len = base + (int)__ffsll((long long)mask) - 1;
        break;
      }
    }
  }
  if (lane == 0) a.trail_len[b] = len;
}

// ---- the pixel rule ----
__device__ __forceinline__ double seg_dist2(const double px, const double py, const double4 s) {
  const double ex = s.z - s.x, ey = s.w - s.y;
  const double dxa = px - s.x, dya = py - s.y;
  const double len2 = ex * ex + ey * ey;
  const double dot = dxa * ex + dya * ey;
  double t = 0.0;
  if (len2 > 0.0) {
    t = dot / len2;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  }
  const double cx = dxa - t * ex, cy = dya - t * ey;
  return cx * cx + cy * cy;
}
__device__ __forceinline__ bool edge_crosses(const double px, const double py, const double4 s) {
  if ((s.y > py) != (s.w > py)) return px < s.x + (py - s.y) * (s.z - s.x) / (s.w - s.y);
  return false;
}

enum { LY_PATH = 1, LY_TRAIL = 2, LY_OBS = 3, LY_MARK = 4, LY_MOVER = 5, LY_RAY = 6, LY_VESSEL = 8 };

struct Tile {
  double cx, cy, reach;    // the tile's bounding circle in the world, its radius grown by the line half-width and the slack
  __device__ __forceinline__ bool near_circle(const double x, const double y, const double r) const {
    const double dx = x - cx, dy = y - cy;
    return !(sqrt(dx * dx + dy * dy) > reach + r);          // (a NaN anywhere keeps the primitive)
  }
  __device__ __forceinline__ bool near_seg(const double4 s) const { return !(seg_dist2(cx, cy, s) > reach * reach); }
};

struct Frame {              // what the layers of one frame read (block-uniform)
  const AuvDev* d;
  const AuvRenderArgs* a;
  EnvDesc ed;
  int b, S, m_max, tlen;
  const double4* dyn;
  const double4* rays;
  const double2* trail;
  const double* marks;     // [M][3] x, y, radius
};

template <int LY> __device__ __forceinline__ int layer_count(const Frame& f) {
  if (LY == LY_PATH) return f.ed.nch;
  if (LY == LY_TRAIL) return f.tlen > 1 ? f.tlen - 1 : 0;
  if (LY == LY_OBS) return f.ed.K;
  if (LY == LY_MARK) return f.marks ? f.a->M : 0;
  if (LY == LY_MOVER) return f.ed.M;
  if (LY == LY_RAY) return f.S;
  return 1;
}
// a pentagon of dyn_seg: kept when the circle around its first vertex through its farthest one reaches the tile
__device__ __forceinline__ int pentagon_near(const Tile& t, const double4* p) {
  const double4 s0 = p[0];
  double r2 = 0.0;
  for (int k = 1; k < 5; k++) {
    const double4 s = p[k];
    const double dx = s.x - s0.x, dy = s.y - s0.y;
    r2 = fmax(r2, dx * dx + dy * dy);
  }
  return t.near_circle(s0.x, s0.y, sqrt(r2)) ? 5 : 0;
}
// segments of candidate i that must be looked at (0: culled)
template <int LY> __device__ __forceinline__ int layer_cull(const Frame& f, const Tile& t, const int i) {
  const AuvDev& d = *f.d;
  if (LY == LY_PATH) {
    const double4 cb = d.chunk_bound[f.ed.c0 + i];
    const int left = f.ed.P - 1 - i * AUV_CHUNK;
    return t.near_circle(cb.x, cb.y, cb.z) ? (left < AUV_CHUNK ? left : AUV_CHUNK) : 0;
  }
  if (LY == LY_TRAIL) {
    const double2 p = f.trail[i], q = f.trail[i + 1];
    return t.near_seg(make_double4(p.x, p.y, q.x, q.y)) ? 1 : 0;
  }
  if (LY == LY_OBS) {
    const int4 meta = d.obs_meta[f.ed.k0 + i];
    if (meta.x == AUV_OBS_MOVER) return 0;
    const double* cu = d.obs_cull + 3 * (f.ed.k0 + i);
    return t.near_circle(cu[0], cu[1], cu[2]) ? meta.z : 0;
  }
  if (LY == LY_MARK) {
    const double* mk = f.marks + 3 * i;
    return t.near_circle(mk[0], mk[1], fabs(mk[2])) ? 1 : 0;        // (the disc rule squares the radius: its sign does not matter)
  }
  if (LY == LY_MOVER) return pentagon_near(t, f.dyn + 5 * i);
  if (LY == LY_RAY) return t.near_seg(f.rays[i]) ? 1 : 0;
  return pentagon_near(t, f.dyn + 5 * f.m_max);
}
template <int LY> __device__ __forceinline__ double4 layer_fetch(const Frame& f, const int i, const int k) {
  const AuvDev& d = *f.d;
  if (LY == LY_PATH) {
    const double2* v = d.poly_xy + f.ed.p0 + (long long)i * AUV_CHUNK + k;
    const double2 p = v[0], q = v[1];
    return make_double4(p.x, p.y, q.x, q.y);
  }
  if (LY == LY_TRAIL) {
    const double2 p = f.trail[i], q = f.trail[i + 1];
    return make_double4(p.x, p.y, q.x, q.y);
  }
  if (LY == LY_OBS) return d.seg[d.obs_meta[f.ed.k0 + i].y + k];
  if (LY == LY_MARK) return make_double4(f.marks[3 * i], f.marks[3 * i + 1], f.marks[3 * i + 2], 0.0);
  if (LY == LY_MOVER) return f.dyn[5 * i + k];
  if (LY == LY_RAY) return f.rays[i];
  return f.dyn[5 * f.m_max + k];
}

struct Pixel {
  double x, y, h2;
  int col;        // palette row of the topmost layer so far (LY_RAY: mixed between rows 6 and 7 by the beam's q)
  int ray;        // the lit beam with the highest index
};

struct Lds {
  double4 stage[K10_BLOCK];
  int owner[K10_BLOCK];
  int surv[K10_BLOCK];
  int spre[K10_BLOCK + 1];
  int wtot[2][K10_WAVES];
#ifdef AUV_RENDER_DIAG
  unsigned long long diag[2];
#endif
};

template <int LY> __device__ __forceinline__ void paint_layer(const Frame& f, const Tile& tile, Pixel& px, Lds& L, const int t) {
  constexpr bool FILL = (LY == LY_OBS || LY == LY_MOVER || LY == LY_VESSEL);
  const int lane = t & (AUV_WAVE - 1), wave = t / AUV_WAVE;
  const int ncand = layer_count<LY>(f);
  int cur = -1, parity = 0;
  bool lit = false;
  for (int base = 0; base < ncand; base += K10_BLOCK) {
    const int idx = base + t;
    const int n = idx < ncand ? layer_cull<LY>(f, tile, idx) : 0;
    const int flag = n > 0 ? 1 : 0;
    const int inc_f = auv_wave_scan_incl(flag), inc_n = auv_wave_scan_incl(n);
    if (lane == AUV_WAVE - 1) L.wtot[0][wave] = inc_f, L.wtot[1][wave] = inc_n;
    __syncthreads();
    int off_f = 0, off_n = 0, tot_f = 0, tot_n = 0;
    for (int w = 0; w < K10_WAVES; w++) {
      const int wf = L.wtot[0][w], wn = L.wtot[1][w];
      if (w < wave) off_f += wf, off_n += wn;
      tot_f += wf, tot_n += wn;
    }
    if (flag) {
      const int pos = off_f + inc_f - 1;
      L.surv[pos] = idx;
      L.spre[pos] = off_n + inc_n - n;
    }
    if (t == 0) L.spre[tot_f] = tot_n;
#ifdef AUV_RENDER_DIAG
    {
      int all = 0;                                  // segments of this pass before the cull (counted by the thread of each candidate)
      if (idx < ncand) {
        Tile open = tile;
        open.reach = 1e300;
        all = layer_cull<LY>(f, open, idx);
      }
      if (all) atomicAdd(&L.diag[0], (unsigned long long)all);
      if (n) atomicAdd(&L.diag[1], (unsigned long long)n);
    }
#endif
    __syncthreads();
    for (int sb = 0; sb < tot_n; sb += K10_BLOCK) {
      const int fl = sb + t;
      if (fl < tot_n) {
        int lo = 0, hi = tot_f - 1;                 // the survivor whose run of segments holds the flat index fl
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (L.spre[mid] <= fl) lo = mid; else hi = mid - 1;
        }
        const int cand = L.surv[lo];
        L.stage[t] = layer_fetch<LY>(f, cand, fl - L.spre[lo]);
        L.owner[t] = cand;
      }
      __syncthreads();
      const int cnt = tot_n - sb < K10_BLOCK ? tot_n - sb : K10_BLOCK;
      for (int k = 0; k < cnt; k++) {
        const double4 s = L.stage[k];
        if (FILL) {
          const int o = L.owner[k];
          if (o != cur) lit |= (parity & 1) != 0, parity = 0, cur = o;
          parity += edge_crosses(px.x, px.y, s) ? 1 : 0;
        } else if (LY == LY_MARK) {
          const double dx = px.x - s.x, dy = px.y - s.y;
          lit |= dx * dx + dy * dy <= s.z * s.z;
        } else if (LY == LY_RAY) {
          if (seg_dist2(px.x, px.y, s) <= px.h2) lit = true, px.ray = L.owner[k];
        } else {
          lit |= seg_dist2(px.x, px.y, s) <= px.h2;
        }
      }
      __syncthreads();
    }
  }
  if (FILL) lit |= (parity & 1) != 0;
  if (lit) px.col = LY;
}

__global__ void __launch_bounds__(K10_BLOCK) k10_raster(const AuvDev d, const AuvRenderArgs a) {
  __shared__ Lds L;
  const int t = threadIdx.x, b = blockIdx.z;
  const int j = blockIdx.x * K10_TILE + (t & (K10_TILE - 1)), i = blockIdx.y * K10_TILE + t / K10_TILE;
  const int e = a.env_idx[b];
  const double* cam = a.cam + (size_t)b * 8;
  const double cx = cam[0], cy = cam[1], m00 = cam[2], m01 = cam[3], m10 = cam[4], m11 = cam[5], zoom = cam[6];
  Frame f;
  f.d = &d, f.a = &a, f.ed = d.env_desc[e], f.b = b, f.S = d.cfg.n_sensors, f.m_max = d.m_max;
  f.tlen = a.trail_len[b];
  f.dyn = a.dyn_seg + (size_t)b * (5 * d.m_max + 5);
  f.rays = a.ray_seg + (size_t)b * f.S;
  f.trail = a.trail ? (const double2*)a.trail + (size_t)b * a.L : nullptr;
  f.marks = a.markers ? a.markers + (size_t)b * a.M * 3 : nullptr;
  const double h = 0.5 * a.line_px / zoom;
  Tile tile;
  {
    const double sx = (double)(blockIdx.x * K10_TILE + K10_TILE / 2) - 0.5 * a.W, sy = (double)(blockIdx.y * K10_TILE + K10_TILE / 2) - 0.5 * a.H;
    tile.cx = cx + (m00 * sx + m01 * sy), tile.cy = cy + (m10 * sx + m11 * sy);
    tile.reach = 11.32 / zoom + h + K10_SLACK;     // 8 sqrt(2) pixels: every pixel centre of the tile, and some
  }
  Pixel px;
  {
    const double sx = ((double)j + 0.5) - 0.5 * a.W, sy = ((double)i + 0.5) - 0.5 * a.H;
    px.x = cx + (m00 * sx + m01 * sy), px.y = cy + (m10 * sx + m11 * sy);
    px.h2 = h * h, px.col = 0, px.ray = 0;
  }
#ifdef AUV_RENDER_DIAG
  if (t == 0) L.diag[0] = L.diag[1] = 0;
  __syncthreads();
#endif
  paint_layer<LY_PATH>(f, tile, px, L, t);
  paint_layer<LY_TRAIL>(f, tile, px, L, t);
  paint_layer<LY_OBS>(f, tile, px, L, t);
  paint_layer<LY_MARK>(f, tile, px, L, t);
  paint_layer<LY_MOVER>(f, tile, px, L, t);
  paint_layer<LY_RAY>(f, tile, px, L, t);
  paint_layer<LY_VESSEL>(f, tile, px, L, t);
#ifdef AUV_RENDER_DIAG
  __syncthreads();
  if (t == 0 && a.diag) atomicAdd(a.diag, L.diag[0]), atomicAdd(a.diag + 1, L.diag[1]);
#endif
  if (j < a.W && i < a.H) {
    uint8_t* out = a.frames + (((size_t)b * a.H + i) * a.W + j) * 3;
    if (px.col == LY_RAY) {
      const int q = a.ray_q[(size_t)b * f.S + px.ray];
      for (int ch = 0; ch < 3; ch++) out[ch] = (uint8_t)((a.palette[18 + ch] * (255 - q) + a.palette[21 + ch] * q + 127) / 255);
    } else {
      for (int ch = 0; ch < 3; ch++) out[ch] = a.palette[3 * px.col + ch];
    }
  }
}

}  // namespace

void auv_launch_render(const AuvDev& d, const AuvRenderArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k10_frame_geometry, dim3(a.B), dim3(AUV_WAVE), 0, st, d, a);
  const dim3 grid((a.W + K10_TILE - 1) / K10_TILE, (a.H + K10_TILE - 1) / K10_TILE, a.B);
  hipLaunchKernelGGL(k10_raster, grid, dim3(K10_BLOCK), 0, st, d, a);
}
