// k7_snapshot.hip — copy an environment out of a handle and back in (auv_snapshot / auv_restore), and score the candidate
// action sequences of a shooting planner (auv_plan_score).
//
// A snapshot row is every per-environment buffer a later step or a later auv_read can observe, packed (layout: include/auv_hip.h,
// auv_snapshot.h).  One wave moves one row: the row segments with the widest access the handle-side row stride allows (16 bytes
// in the usual shapes; the snapshot row's own offsets are always multiples of 16), the six state doubles as a strided gather /
// scatter.  Plain loads and stores: the calls are stream-ordered behind and in front of whole launches.  A pair whose environment,
// row or world index is out of range is skipped and counted, never accessed.
#include "auv_device.h"
#include "auv_launch.h"
#include "auv_plan.h"
#include "auv_snapshot.h"

namespace {

template <typename T>
__device__ __forceinline__ void snap_copy_as(char* __restrict__ dst, const char* __restrict__ src, const uint32_t bytes, const int lane) {
  T* __restrict__ o = (T*)dst;
  const T* __restrict__ s = (const T*)src;
  const uint32_t cnt = bytes / (uint32_t)sizeof(T);
  for (uint32_t i = lane; i < cnt; i += AUV_WAVE) o[i] = s[i];
}

// `bytes` is the row's length AND its stride in the handle's buffer, whose base is aligned to 256: the widest unit that divides
// it is aligned on both sides
__device__ __forceinline__ void snap_copy(char* __restrict__ dst, const char* __restrict__ src, const uint32_t bytes, const int lane) {
  if ((bytes & 15u) == 0) snap_copy_as<uint4>(dst, src, bytes, lane);
  else if ((bytes & 7u) == 0) snap_copy_as<uint2>(dst, src, bytes, lane);
  else if ((bytes & 3u) == 0) snap_copy_as<uint32_t>(dst, src, bytes, lane);
  else snap_copy_as<uint8_t>(dst, src, bytes, lane);
}

// the nine 64-bit words behind the counters: x, y, psi, u, v, r (a column of the [6][N] state), reward64, rew_path, rew_lidar
__device__ __forceinline__ unsigned long long* snap_head_word(const AuvSnapArgs& a, const int e, const int lane) {
  if (lane < 6) return a.state + (size_t)lane * (size_t)a.n + e;
  if (lane == 6) return a.reward64 + e;
  if (lane == 7) return a.rew_path + e;
  return a.rew_lidar + e;
}

__device__ __forceinline__ void snap_skip(const AuvSnapArgs& a, const int lane) {
  if (lane == 0) atomicAdd(a.skipped, 1u);
}

// row j <- environment env_idx[j] (NULL: j)
__global__ void __launch_bounds__(AUV_BLOCK) k7_snapshot(const AuvSnapArgs a, const int32_t* __restrict__ env_idx, const int m, char* __restrict__ rows) {
  const int wave = threadIdx.x / AUV_WAVE, lane = threadIdx.x % AUV_WAVE;
  const int j = auv_uniform(blockIdx.x * AUV_ENVS_PER_BLOCK + wave);
  if (j >= m) return;
  const int e = auv_uniform(env_idx ? env_idx[j] : j);
  if (e < 0 || e >= a.n) return snap_skip(a, lane);
  char* row = rows + (size_t)j * a.row_bytes;
  if (lane == 0) *(int4*)row = a.counters[e];
  if (lane < 9) ((unsigned long long*)(row + 16))[lane] = *snap_head_word(a, e, lane);
  if (lane == 9) *(unsigned long long*)(row + 88) = (unsigned long long)(uint32_t)a.world_idx[e] | ((unsigned long long)a.collision[e] << 32);
#pragma unroll
  for (int s = 0; s < AUV_SNAP_SEGS; s++) {
    const uint32_t bytes = a.seg[s].bytes;
    if (!bytes) continue;
    char* dst = row + a.seg[s].off;
    snap_copy(dst, a.seg[s].base + (size_t)e * bytes, bytes, lane);
    if ((uint32_t)lane < ((0u - bytes) & 15u)) dst[bytes + lane] = 0;     // the padding is part of the row: rows compare equal
  }
}

// environment env_idx[j] <- row row_idx[j] (either NULL: j).  The world descriptor is rebuilt from the row's world index and THIS
// handle's bank tables (auv_make_desc: what restore_env binds with); with `obs_out` the caller's float32 observation row is written as
// the step writes it: the first min(D, 6 + S) columns of the fp64 row, cast (k3_nav_reward.hip, restore_env / nav_tail; k2_lidar.hip)
__global__ void __launch_bounds__(AUV_BLOCK) k7_restore(const AuvSnapArgs a, const AuvDev d, const char* __restrict__ rows, const int n_rows,
                                                        const int32_t* __restrict__ row_idx, const int32_t* __restrict__ env_idx, const int m,
                                                        float* __restrict__ obs_out) {
  const int wave = threadIdx.x / AUV_WAVE, lane = threadIdx.x % AUV_WAVE;
  const int j = auv_uniform(blockIdx.x * AUV_ENVS_PER_BLOCK + wave);
  if (j >= m) return;
  const int r = auv_uniform(row_idx ? row_idx[j] : j);
  const int e = auv_uniform(env_idx ? env_idx[j] : j);
  if (r < 0 || r >= n_rows || e < 0 || e >= a.n) return snap_skip(a, lane);
  const char* row = rows + (size_t)r * a.row_bytes;
  const unsigned long long wc = *(const unsigned long long*)(row + 88);
  const int w = auv_uniform((int)(uint32_t)wc);
  if (w < 0 || w >= a.n_worlds) return snap_skip(a, lane);
  if (lane == 0) a.counters[e] = *(const int4*)row;
  if (lane < 9) *snap_head_word(a, e, lane) = ((const unsigned long long*)(row + 16))[lane];
  if (lane == 9) a.world_idx[e] = w, a.collision[e] = (uint8_t)(wc >> 32);
  if (lane == 10) d.env_desc[e] = auv_make_desc(d, w);
#pragma unroll
  for (int s = 0; s < AUV_SNAP_SEGS; s++) {
    const uint32_t bytes = a.seg[s].bytes;
    if (bytes) snap_copy(a.seg[s].base + (size_t)e * bytes, row + a.seg[s].off, bytes, lane);
  }
  if (obs_out) {
    const int S = d.cfg.n_sensors;
    const int D = auv_obs_cols(d.cfg, d.pool_ns);
    const int DL = D < 6 + S ? D : 6 + S;
    const double* ob = (const double*)(row + a.obs_off);
    for (int i = lane; i < DL; i += AUV_WAVE) obs_out[(size_t)e * D + i] = (float)ob[i];
  }
}

// ---- scoring the candidates of a shooting planner ----
// score[e] = sum over t of disc_t * reward[t][e], up to and including the first t with done[t][e]; disc_0 = 1, disc_{t+1} = disc_t * gamma;
// every product and every sum rounded to float32, in increasing t (part of the contract: a plain float32 loop reproduces the bits).
__device__ __forceinline__ float plan_score_env(const float* __restrict__ reward, const uint8_t* __restrict__ done, const int T, const int n,
                                                const int e, const float gamma) {
  float s = 0.0f, disc = 1.0f;
  for (int t = 0; t < T; t++) {
    s = __fadd_rn(s, __fmul_rn(disc, reward[(size_t)t * n + e]));
    if (done[(size_t)t * n + e]) break;
    disc = __fmul_rn(disc, gamma);
  }
  return s;
}

// (plan_beats, the order of (score, index) pairs: auv_plan.h, shared with the refit of k15_plan.hip)

// Lanes run across environments (row t of the record is read coalesced); a wave reduction gives the argmax.  A group of 1, 2, .. 64
// (a power of two) environments shares its wave with 64 / group - 1 others (`span` = group: the butterfly stays inside the group's
// lanes); any other group size has a wave to itself, every lane taking the environments lane, lane + 64, .. of it (`span` = 64).
__global__ void __launch_bounds__(AUV_WAVE) k7_plan_score(const float* __restrict__ reward, const uint8_t* __restrict__ done, const int T,
                                                          const int n, const int group, const int span, const float gamma,
                                                          float* __restrict__ score, int32_t* __restrict__ best) {
  const int lane = threadIdx.x;
  float bs = 0.0f;
  int bi = PLAN_NONE;
  int g;                                  // this lane's group
  if (span < AUV_WAVE || group == AUV_WAVE) {
    const int e = blockIdx.x * AUV_WAVE + lane;
    g = e / group;
    if (e < n) {
      const float s = plan_score_env(reward, done, T, n, e, gamma);
      score[e] = s;
      if (s == s) bs = s, bi = e - g * group;
    }
  } else {
    g = blockIdx.x;
    for (int k = lane; k < group; k += AUV_WAVE) {
      const int e = g * group + k;
      const float s = plan_score_env(reward, done, T, n, e, gamma);
      score[e] = s;
      if (s == s && plan_beats(s, k, bs, bi)) bs = s, bi = k;
    }
  }
  for (int off = 1; off < span; off <<= 1) {
    const float os = __shfl_xor(bs, off, AUV_WAVE);
    const int oi = __shfl_xor(bi, off, AUV_WAVE);
    if (plan_beats(os, oi, bs, bi)) bs = os, bi = oi;
  }
  const int first = span < AUV_WAVE ? (lane % span) : lane;
  if (first == 0 && (long long)g * group < n) best[g] = bi == PLAN_NONE ? 0 : bi;
}

}  // namespace

void auv_launch_snapshot(const AuvSnapArgs& a, const int32_t* env_idx, int m, void* rows, hipStream_t st) {
  hipLaunchKernelGGL(k7_snapshot, dim3((m + AUV_ENVS_PER_BLOCK - 1) / AUV_ENVS_PER_BLOCK), dim3(AUV_BLOCK), 0, st, a, env_idx, m, (char*)rows);
}

void auv_launch_restore(const AuvSnapArgs& a, const AuvDev& d, const void* rows, int n_rows, const int32_t* row_idx, const int32_t* env_idx, int m,
                        float* obs, hipStream_t st) {
  hipLaunchKernelGGL(k7_restore, dim3((m + AUV_ENVS_PER_BLOCK - 1) / AUV_ENVS_PER_BLOCK), dim3(AUV_BLOCK), 0, st, a, d, (const char*)rows, n_rows, row_idx,
                     env_idx, m, obs);
}

void auv_launch_plan_score(const float* reward, const uint8_t* done, int T, int n, int group, float gamma, float* score, int32_t* best, hipStream_t st) {
  const bool packed = group <= AUV_WAVE && (group & (group - 1)) == 0;
  const int span = packed ? group : AUV_WAVE;
  const int grid = packed ? (n + AUV_WAVE - 1) / AUV_WAVE : n / group;
  hipLaunchKernelGGL(k7_plan_score, dim3(grid), dim3(AUV_WAVE), 0, st, reward, done, T, n, group, span, gamma, score, best);
}
