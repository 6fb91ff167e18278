// auv_capi_aux.hip — the C ABI's entries beside the step (include/auv_hip.h): pooled observations and feasibility pooling, the
// device renderer, snapshot / restore of environments, and the planner's scores, sampler and refit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <initializer_list>

#include "auv_host.h"
#include "auv_render.h"
#include "auv_snapshot.h"

using namespace auv_host;

extern "C" {

int auv_set_obs_pooling(auv_handle_t* h, int32_t n_sectors, const int32_t* sector_start_host, double width) {
  if (!h) return fail(AUV_EINVAL, "null handle");
  if (h->bank_seen) return fail(AUV_ESTATE, "auv_set_obs_pooling: only before the first bank is loaded (the reset rows depend on it)");
  const int S = h->d.cfg.n_sensors;
  if (n_sectors == 0) {
    h->d.pool_ns = 0, h->d.pool_width = 0.0;
    h->pool_word_host.clear();
    return AUV_OK;
  }
  if (n_sectors < 1 || !sector_start_host) return fail(AUV_EINVAL, "auv_set_obs_pooling: n_sectors must be >= 1 (0: off) with a table");
  if (!std::isfinite(width) || !(width > 0.0)) return fail(AUV_EINVAL, "auv_set_obs_pooling: width must be finite and > 0");
  if (sector_start_host[0] != 0 || sector_start_host[n_sectors] != S)
    return fail(AUV_EINVAL, "auv_set_obs_pooling: the sector table must run from 0 to n_sensors (%d)", S);
  for (int k = 0; k < n_sectors; k++)
    if (sector_start_host[k + 1] <= sector_start_host[k]) return fail(AUV_EINVAL, "auv_set_obs_pooling: sector %d is empty", k);
  // with the LiDAR off the observation has no LiDAR columns to pool (the reference never calls perceive): accepted, ignored
  if (!h->d.cfg.use_lidar) return AUV_OK;
  h->pool_word_host.assign((size_t)S, 0u);
  for (int k = 0; k < n_sectors; k++) {
    const int s0 = sector_start_host[k], s1 = sector_start_host[k + 1];
    for (int i = s0; i < s1; i++) h->pool_word_host[(size_t)i] = (uint32_t)s0 | ((uint32_t)(s1 - s0) << 16);   // (S <= 4096)
  }
  h->d.pool_ns = n_sectors, h->d.pool_width = width;
  return AUV_OK;
}

int auv_feasibility_pooling(auv_handle_t* h, const int32_t* sector_start_dev, int32_t n_sectors, double width,
                            double* out_dist_dev, float* out_closeness_dev, void* stream) {
  REQUIRE_READY(h);
  if (!sector_start_dev || n_sectors < 1 || n_sectors > h->d.cfg.n_sensors || !(width >= 0.0))
    return fail(AUV_EINVAL, "auv_feasibility_pooling: bad arguments");
  auv_launch_k4(h->d, sector_start_dev, n_sectors, width, out_dist_dev, out_closeness_dev, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

int auv_render(auv_handle_t* h, void* stream, const int32_t* env_idx_host, int32_t B, int32_t H, int32_t W, double zoom, int32_t view,
               double line_px, const double* trail_dev, int32_t L, const double* markers_dev, int32_t M, const uint8_t* palette_host,
               uint8_t* frames_dev, double* cam_out, double* dyn_seg_out, double* ray_seg_out, uint8_t* ray_q_out) {
  if (!h) return fail(AUV_EINVAL, "auv_render: null handle");
  if (!h->worlds_loaded) return fail(AUV_EINVAL, "auv_render: no world bank loaded");
  if (B < 1 || H < 1 || W < 1) return fail(AUV_EINVAL, "auv_render: B = %d, H = %d, W = %d: each must be >= 1", B, H, W);
  if (H > 4096 || W > 4096 || B > 65535) return fail(AUV_EINVAL, "auv_render: H = %d, W = %d (at most 4096), B = %d (at most 65535)", H, W, B);
  if (!(std::isfinite(zoom) && zoom > 0.0)) return fail(AUV_EINVAL, "auv_render: zoom = %g must be finite and > 0", zoom);
  if (!(std::isfinite(line_px) && line_px > 0.0)) return fail(AUV_EINVAL, "auv_render: line_px = %g must be finite and > 0", line_px);
  if (view != AUV_VIEW_HEADING_UP && view != AUV_VIEW_NORTH_UP) return fail(AUV_EINVAL, "auv_render: unknown view %d", view);
  if (!env_idx_host || !palette_host || !frames_dev) return fail(AUV_EINVAL, "auv_render: null index list, palette or frame buffer");
  if (L < 0 || M < 0) return fail(AUV_EINVAL, "auv_render: L = %d, M = %d must not be negative", L, M);
  for (int j = 0; j < B; j++)
    if (env_idx_host[j] < 0 || env_idx_host[j] >= h->d.n)
      return fail(AUV_EINVAL, "auv_render: env_idx[%d] = %d is outside the handle's %d environments", j, env_idx_host[j], h->d.n);
  HIP_TRY(hipSetDevice(h->device));
  const AuvDev& d = h->d;
  const size_t S = (size_t)(d.cfg.n_sensors > 0 ? d.cfg.n_sensors : 1), nd = 5 * (size_t)d.m_max + 5;
  hipStream_t st = (hipStream_t)stream;
  if (B > h->render_cap) {
    // grow: the old scratch may still be read by renders in flight, so the device is drained first (a host synchronisation, on
    // the first call and on a call with more frames than any before it only)
    HIP_TRY(hipDeviceSynchronize());
    free_pool(h->render_allocs);
    if (h->r_pin) (void)hipHostFree(h->r_pin);
    h->r_pin = nullptr;
    h->render_cap = 0;
    int cap = 16;
    while (cap < B) cap *= 2;
    int rc = 0;
    rc |= dev_alloc(h->render_allocs, &h->r_idx, (size_t)cap);
    rc |= dev_alloc(h->render_allocs, &h->r_cam, (size_t)cap * 8);
    rc |= dev_alloc(h->render_allocs, &h->r_dyn, (size_t)cap * nd);
    rc |= dev_alloc(h->render_allocs, &h->r_ray, (size_t)cap * S);
    rc |= dev_alloc(h->render_allocs, &h->r_q, (size_t)cap * S);
    rc |= dev_alloc(h->render_allocs, &h->r_tlen, (size_t)cap);
    if (rc) return AUV_EHIP;
    HIP_TRY(hipHostMalloc((void**)&h->r_pin, 4 * (size_t)cap * sizeof(int32_t), hipHostMallocDefault));
    for (int k = 0; k < 4; k++)
      if (!h->r_pin_ev[k]) HIP_TRY(hipEventCreateWithFlags(&h->r_pin_ev[k], hipEventDisableTiming));
    h->render_cap = cap;
    h->r_seq = 0;
  }
  const unsigned slot = h->r_seq & 3;
  if (h->r_seq >= 4) HIP_TRY(hipEventSynchronize(h->r_pin_ev[slot]));   // (returns at once unless four renders are still queued)
  h->r_seq++;
  int32_t* pin = h->r_pin + (size_t)slot * h->render_cap;
  memcpy(pin, env_idx_host, (size_t)B * sizeof(int32_t));
  HIP_TRY(hipMemcpyAsync(h->r_idx, pin, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st));
  HIP_TRY(hipEventRecord(h->r_pin_ev[slot], st));
  AuvRenderArgs a;
  memset(&a, 0, sizeof(a));
  a.env_idx = h->r_idx, a.B = B, a.H = H, a.W = W, a.view = view, a.zoom = zoom, a.line_px = line_px;
  a.trail = L > 0 ? trail_dev : nullptr, a.L = L;
  a.markers = M > 0 ? markers_dev : nullptr, a.M = M;
  memcpy(a.palette, palette_host, 27);
  a.frames = frames_dev;
  a.cam = cam_out ? cam_out : h->r_cam;
  a.dyn_seg = dyn_seg_out ? (double4*)dyn_seg_out : h->r_dyn;
  a.ray_seg = ray_seg_out ? (double4*)ray_seg_out : h->r_ray;
  a.ray_q = ray_q_out ? ray_q_out : h->r_q;
  a.trail_len = h->r_tlen;
#ifdef AUV_RENDER_DIAG
  if (!h->r_diag) {
    HIP_TRY(hipMalloc((void**)&h->r_diag, 2 * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(h->r_diag, 0, 2 * sizeof(unsigned long long)));
  }
  a.diag = h->r_diag;
#endif
  auv_launch_render(d, a, st);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

#ifdef AUV_RENDER_DIAG
// Only in the diagnostic build (tools/build_variant.sh render_diag "-DAUV_RENDER_DIAG"; tools/render_bench.py): segments the
// rasteriser's tiles were offered / kept after the tile cull since the last call (synchronises the device; resets the counts).
int auv_render_diag(auv_handle_t* h, uint64_t* out2);   // (the product's header does not declare this build's entry)
int auv_render_diag(auv_handle_t* h, uint64_t* out2) {
  if (!h || !out2) return fail(AUV_EINVAL, "auv_render_diag: null argument");
  out2[0] = out2[1] = 0;
  if (!h->r_diag) return AUV_OK;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out2, h->r_diag, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(h->r_diag, 0, 2 * sizeof(uint64_t)));
  return AUV_OK;
}
#endif

// ---- snapshot / restore of environments (layout: include/auv_hip.h; kernels: k7_snapshot.hip) ----
static void snap_args(const auv_handle_t* h, AuvSnapArgs* a) {
  const AuvDev& d = h->d;
  const uint32_t S = (uint32_t)d.cfg.n_sensors, K = (uint32_t)d.k_max, M = (uint32_t)d.m_max, ns = (uint32_t)d.pool_ns;
  const struct { void* base; uint32_t bytes; } rows[AUV_SNAP_SEGS] = {
      {d.info64, 64}, {d.nav64, 64}, {d.step_info, 32}, {d.episode, 32}, {d.lidar_d, 8 * S}, {d.obs64, 8 * (6 + S)},
      {d.mover, 32 * M}, {d.limits, 8 * K}, {d.nearby, K}, {ns ? d.sector_d : nullptr, 8 * ns}};
  uint32_t off = AUV_SNAP_HEAD;
  for (int i = 0; i < AUV_SNAP_SEGS; i++) {
    a->seg[i].base = (char*)rows[i].base, a->seg[i].bytes = rows[i].bytes, a->seg[i].off = off;
    if (i == 5) a->obs_off = off;
    off += (rows[i].bytes + 15u) & ~15u;
  }
  a->row_bytes = off;
  a->counters = d.counters, a->state = (unsigned long long*)d.state, a->reward64 = (unsigned long long*)d.reward64;
  a->rew_path = (unsigned long long*)d.rew_path, a->rew_lidar = (unsigned long long*)d.rew_lidar;
  a->world_idx = d.world_idx, a->collision = d.collision, a->skipped = h->snap_skipped;
  a->n = d.n, a->n_worlds = d.n_worlds;
}

size_t auv_snapshot_row_bytes(const auv_handle_t* h) {
  if (!h || !h->worlds_loaded) return 0;
  AuvSnapArgs a;
  snap_args(h, &a);
  return a.row_bytes;
}

uint64_t auv_snapshot_layout(const auv_handle_t* h) {
  if (!h || !h->worlds_loaded) return 0;
  const AuvDev& d = h->d;
  const uint64_t v[11] = {AUV_ABI_VERSION, AUV_SNAP_FORMAT, (uint64_t)d.cfg.n_sensors, (uint64_t)d.k_max, (uint64_t)d.m_max, (uint64_t)d.pool_ns,
                          (uint64_t)d.cfg.obs_channels, (uint64_t)(d.cfg.use_lidar != 0), (uint64_t)d.n_worlds, (uint64_t)auv_snapshot_row_bytes(h), 0};
  uint64_t x = 0xcbf29ce484222325ull;                    // FNV-1a over the bytes of the ten numbers
  for (int i = 0; i < 10; i++)
    for (int b = 0; b < 8; b++) x = (x ^ ((v[i] >> (8 * b)) & 0xff)) * 0x100000001b3ull;
  return x ? x : 1;                                      // (0 is "no bank yet")
}

// what auv_snapshot and auv_restore refuse, before anything is enqueued
static int snap_check(auv_handle_t* h, void* stream, float* obs, const char* who) {
  REQUIRE_READY(h);
  if (h->fw.on)
    return fail(AUV_ESTATE, "%s: not with a fresh world per reset (a bank slot belongs to ONE environment and is rebuilt when that environment "
                            "leaves it: a copy of the environment would share the slot)", who);
  if (h->async_pending) return fail(AUV_ESTATE, "%s: a step_async is pending (auv_step_wait first)", who);
  PAIR_CHECK_ON(h, stream, true, obs);
  return AUV_OK;
}

int auv_snapshot(auv_handle_t* h, const int32_t* env_idx_dev, int32_t m, void* rows_dev, void* stream) {
  int rc = snap_check(h, stream, nullptr, "auv_snapshot");
  if (rc) return rc;
  if (m < 0 || !rows_dev || ((uintptr_t)rows_dev & 15)) return fail(AUV_EINVAL, "auv_snapshot: m >= 0 and rows_dev 16-byte aligned");
  if (!env_idx_dev && m > h->d.n) return fail(AUV_EINVAL, "auv_snapshot: %d rows of %d environments (env_idx_dev == NULL: row j is environment j)", m, h->d.n);
  if (m == 0) return AUV_OK;
  AuvSnapArgs a;
  snap_args(h, &a);
  auv_launch_snapshot(a, env_idx_dev, m, rows_dev, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

int auv_restore(auv_handle_t* h, uint64_t layout, const void* rows_dev, int32_t n_rows, const int32_t* row_idx_dev, const int32_t* env_idx_dev,
                int32_t m, float* obs_dev, void* stream) {
  int rc = snap_check(h, stream, obs_dev, "auv_restore");
  if (rc) return rc;
  if (layout != auv_snapshot_layout(h))
    return fail(AUV_EINVAL, "auv_restore: layout %016llx is not this handle's (%016llx): the rows were taken from a handle of another shape",
                (unsigned long long)layout, (unsigned long long)auv_snapshot_layout(h));
  if (m < 0 || n_rows < 0 || !rows_dev || ((uintptr_t)rows_dev & 15)) return fail(AUV_EINVAL, "auv_restore: m, n_rows >= 0 and rows_dev 16-byte aligned");
  if ((!row_idx_dev && m > n_rows) || (!env_idx_dev && m > h->d.n))
    return fail(AUV_EINVAL, "auv_restore: %d pairs, %d rows, %d environments (a NULL index array stands for 0 .. m - 1)", m, n_rows, h->d.n);
  const int D = auv_obs_cols(h->d.cfg, h->d.pool_ns);
  if (obs_dev && ((uintptr_t)obs_dev & 3)) return fail(AUV_EINVAL, "auv_restore: obs_dev must be 4-byte aligned (rows of %d floats)", D);
  if (m == 0) return AUV_OK;
  AuvSnapArgs a;
  snap_args(h, &a);
  auv_launch_restore(a, h->d, rows_dev, n_rows, row_idx_dev, env_idx_dev, m, obs_dev, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

int auv_snapshot_skipped(auv_handle_t* h, int64_t* out_skipped, void* stream) {
  REQUIRE_READY(h);
  if (!out_skipped) return fail(AUV_EINVAL, "auv_snapshot_skipped: null output");
  unsigned int v = 0;
  HIP_TRY(hipMemcpyAsync(&v, h->snap_skipped, sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  *out_skipped = (int64_t)v;
  return AUV_OK;
}

int auv_plan_score(auv_handle_t* h, const float* reward_rec, const uint8_t* done_rec, int32_t n_steps, int32_t n, int32_t group, float gamma,
                   float* score_dev, int32_t* best_dev, void* stream) {
  if (!h) return fail(AUV_EINVAL, "null handle");
  if (!reward_rec || !done_rec || !score_dev || !best_dev || n_steps < 1 || n < 1 || group < 1 || n % group)
    return fail(AUV_EINVAL, "auv_plan_score: bad arguments (n_steps, n, group >= 1; n a multiple of group)");
  HIP_TRY(hipSetDevice(h->device));
  auv_launch_plan_score(reward_rec, done_rec, n_steps, n, group, gamma, score_dev, best_dev, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

int auv_plan_score_v(auv_handle_t* h, const float* reward_rec, const uint8_t* done_rec, int32_t n_steps, int32_t n, int32_t group, float gamma,
                     const float* terminal_value, float* score_dev, int32_t* best_dev, void* stream) {
  if (!terminal_value) return auv_plan_score(h, reward_rec, done_rec, n_steps, n, group, gamma, score_dev, best_dev, stream);
  if (!h) return fail(AUV_EINVAL, "null handle");
  if (!reward_rec || !done_rec || !score_dev || !best_dev || n_steps < 1 || n < 1 || group < 1 || n % group)
    return fail(AUV_EINVAL, "auv_plan_score_v: bad arguments (n_steps, n, group >= 1; n a multiple of group)");
  if ((uintptr_t)terminal_value & 3) return fail(AUV_EINVAL, "auv_plan_score_v: terminal_value must be 4-byte aligned");
  HIP_TRY(hipSetDevice(h->device));
  auv_launch_plan_score_v(reward_rec, done_rec, terminal_value, n_steps, n, group, gamma, score_dev, best_dev, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

// ---- the planner's sampler and refit (kernels: k15_plan.hip) ----
// the sizes both calls share
static int plan_shape_check(const auv_handle_t* h, int32_t n_steps, int32_t n, int32_t group, const char* who) {
  if (!h) return fail(AUV_EINVAL, "null handle");
  if (n_steps < 1 || n < 1 || group < 1 || n % group)
    return fail(AUV_EINVAL, "%s: bad arguments (n_steps, n, group >= 1; n a multiple of group)", who);
  if (group > AUV_PLAN_MAX_GROUP) return fail(AUV_EINVAL, "%s: group = %d, at most %d candidates per group", who, group, AUV_PLAN_MAX_GROUP);
  if (2ll * n_steps * n > 0x7fffffffll) return fail(AUV_EINVAL, "%s: n_steps * n * 2 = %lld does not fit 31 bits", who, 2ll * n_steps * n);
  return AUV_OK;
}

static bool plan_misaligned(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if ((uintptr_t)p & 3) return true;
  return false;
}

int auv_plan_sample(auv_handle_t* h, const float* mean_dev, const float* sigma_dev, const float* mean0_dev, const float* sigma0_dev,
                    const uint8_t* reset_dev, int32_t n_steps, int32_t n, int32_t group, int32_t shift, const float* lo_host, const float* hi_host,
                    uint64_t seed, uint64_t draw, float* ring_dev, void* stream) {
  int rc = plan_shape_check(h, n_steps, n, group, "auv_plan_sample");
  if (rc) return rc;
  if (!mean_dev || !sigma_dev || !ring_dev || !lo_host || !hi_host) return fail(AUV_EINVAL, "auv_plan_sample: null mean, sigma, ring or bounds");
  if (shift != 0 && shift != 1) return fail(AUV_EINVAL, "auv_plan_sample: shift = %d must be 0 or 1", shift);
  if (reset_dev && (!mean0_dev || !sigma0_dev)) return fail(AUV_EINVAL, "auv_plan_sample: a reset mask needs mean0 and sigma0");
  if (plan_misaligned({mean_dev, sigma_dev, mean0_dev, sigma0_dev, ring_dev}))
    return fail(AUV_EINVAL, "auv_plan_sample: mean, sigma, mean0, sigma0 and the ring must be 4-byte aligned");
  HIP_TRY(hipSetDevice(h->device));
  AuvPlanSample a;
  a.mean = mean_dev, a.sigma = sigma_dev, a.mean0 = mean0_dev, a.sigma0 = sigma0_dev, a.reset = reset_dev, a.ring = ring_dev;
  a.T = n_steps, a.n = n, a.group = group, a.shift = shift;
  a.lo[0] = lo_host[0], a.lo[1] = lo_host[1], a.hi[0] = hi_host[0], a.hi[1] = hi_host[1];
  a.seed = seed, a.draw = draw;
  auv_launch_plan_sample(a, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

int auv_plan_refit(auv_handle_t* h, const float* ring_dev, const float* score_dev, const int32_t* best_dev, int32_t n_steps, int32_t n, int32_t group,
                   int32_t method, int32_t n_elite, float sigma_min, float lambda, const float* mean_in_dev, const float* sigma_in_dev,
                   float* mean_out_dev, float* sigma_out_dev, float* chosen_dev, float* predicted_dev, void* stream) {
  int rc = plan_shape_check(h, n_steps, n, group, "auv_plan_refit");
  if (rc) return rc;
  if (!ring_dev || !score_dev || !best_dev) return fail(AUV_EINVAL, "auv_plan_refit: null ring, score or best");
  if (method != AUV_PLAN_CEM && method != AUV_PLAN_MPPI) return fail(AUV_EINVAL, "auv_plan_refit: unknown method %d", method);
  if ((mean_out_dev == nullptr) != (sigma_out_dev == nullptr)) return fail(AUV_EINVAL, "auv_plan_refit: mean_out and sigma_out go together");
  if (mean_out_dev && method == AUV_PLAN_CEM && (n_elite < 1 || n_elite > group))
    return fail(AUV_EINVAL, "auv_plan_refit: n_elite = %d must be in [1, group = %d]", n_elite, group);
  if (mean_out_dev && method == AUV_PLAN_MPPI) {
    if (!std::isfinite(lambda) || !(lambda > 0.0f)) return fail(AUV_EINVAL, "auv_plan_refit: lambda = %g must be finite and > 0", (double)lambda);
    if (!mean_in_dev || !sigma_in_dev) return fail(AUV_EINVAL, "auv_plan_refit: MPPI needs mean_in and sigma_in");
    if (mean_in_dev == mean_out_dev || sigma_in_dev == sigma_out_dev) return fail(AUV_EINVAL, "auv_plan_refit: the outputs must not be the inputs");
  }
  if (plan_misaligned({ring_dev, score_dev, best_dev, mean_in_dev, sigma_in_dev, mean_out_dev, sigma_out_dev, chosen_dev, predicted_dev}))
    return fail(AUV_EINVAL, "auv_plan_refit: every buffer must be 4-byte aligned");
  HIP_TRY(hipSetDevice(h->device));
  AuvPlanRefit a;
  a.ring = ring_dev, a.score = score_dev, a.best = best_dev, a.mean_in = mean_in_dev, a.sigma_in = sigma_in_dev;
  a.mean_out = mean_out_dev, a.sigma_out = sigma_out_dev, a.chosen = chosen_dev, a.predicted = predicted_dev;
  a.T = n_steps, a.n = n, a.group = group, a.method = method, a.n_elite = n_elite, a.sigma_min = sigma_min, a.lambda = lambda;
  auv_launch_plan_refit(a, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

}  // extern "C"
