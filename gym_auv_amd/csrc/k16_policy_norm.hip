// K16 -- running observation and reward normalisation in the policy launch (auv_policy_act_norm, auv_policy_rollout_norm), the same
// normalising expression on arbitrary rows (auv_norm_rows), the fold of the observation moments (auv_norm_fold) and the return pass
// over a stored rollout (auv_norm_returns).  What stable-baselines ships as VecNormalize: running mean and variance of the
// observations, and rewards divided by the running deviation of the discounted return.
//
// DEVIATION from stable-baselines, on purpose (include/auv_hip.h): stable-baselines updates its statistics at every
// step_wait, before it normalises that step's batch -- here a reduction over all N environments between the environment's launch and
// the policy launch of every step, a barrier across chains that are deliberately not ordered against each other.  So the statistics
// are FROZEN while launches run and FOLDED between rollouts: a launch normalises with a table nobody writes during the rollout and
// leaves the moments of its RAW rows as a partial per tile; one fold behind the rollout merges the partials in a fixed order.  The
// rewards of a rollout are scaled behind it, by the deviation that already holds that rollout's returns.
//
// k16_norm_act<A> is k6_policy_act<A, false> with another tile step: both are pol_act_body (auv_policy_forward.h, which states the
// Tile contract), and this file holds only NormTile -- what goes between the tile's fill and the trunk.  The raw
// tile goes to LDS (pol_act_fill_obs without the copy into O); behind a barrier thread c < obs_dim owns column c of the tile's
// rows <= 16 rows, in row order 0 .. rows - 1 (consecutive threads on consecutive LDS words: no bank conflict):
//   moments      s = the sequential f32 sum, m = s / rows, M2 = sum of (x_r - m)^2 sequential; every operation separately rounded
//   normalise    x' = min(max((x - mean[c]) * inv_std[c], -clip_obs), clip_obs), written back into the tile
//   stores       policy workgroup only (blockIdx.y == 0): x' into O[t]'s rows, (m, M2) into part[t * part_ld + part_base + tile][2]
//                [obs_dim], the row count into pcnt[t * part_ld + part_base + tile].  The value workgroup normalises its own copy of
//                the tile and stores nothing.
// The trunk's first barrier is the one behind this step: one barrier more than k6.  The table is requested ahead of the tile's
// zeroing (k6's rule: requests first, stores last).  The flush launch (t == T) stores R[T - 1] / Dn[T - 1] only.
//
// k16_norm_fold: one wave per column.  Lane l merges the partials l, l + 64, ... of the n_slots slots in that order (slots with
// pcnt == 0 are skipped) by Chan's pairwise formula in fp64 (norm_merge); the 64 lane results merge as a tree -- for o = 32, 16, 8, 4, 2,
// 1: lane l < o takes merge(a = lane l, b = lane l + o) -- so lane 0 ends with ((0 + 32) + (16 + 48)) + ... ; that result merges into
// the running (count, mean, M2) as b.  No atomics anywhere: a rerun is bit-identical.
//
// k16_return_env / _merge / _scale: the reward pass.  One thread per environment walks t = 0 .. T - 1 as k6_gae does (forwards):
// ret = ret * gamma + r in fp64, the return taken into a Welford recursion over the environment's T returns, then ret = 0 where done
// (stable-baselines' order).  One wave merges the N per-environment partials (lane l: environments l, l + 64, ...; the same tree) into
// the running return moments.  The third launch scales: r' = min(max(r / (float)sqrt(M2 / count + eps), -clip), clip) in f32.
#include "auv_launch.h"
#include "auv_policy_forward.h"

namespace {

// THE normalising expression: the act launch and k16_norm_rows give the same bits
__device__ __forceinline__ float norm_apply(const float x, const float mean, const float inv_std, const float clip) {
  return fminf(fmaxf(__fmul_rn(__fsub_rn(x, mean), inv_std), -clip), clip);
}

// column c of the raw tile: its moments, and the normalised values written back (and into dstO, nullable: O[t]'s rows of the tile)
// (dstO and part_m point at column c already: per-thread addresses, so that the bases need no scalar registers across the step)
__device__ __forceinline__ void norm_tile_column(float* col, const int ldx, const int rows, const int K0, const float2 tb, const float clip,
                                                 float* dstO, float* part_m) {
  // (per-thread addresses that move on row by row: no scalar offset per row)
  float s = 0.0f, M2 = 0.0f;
  const float* q = col;
  for (int r = 0; r < rows; r++, q += ldx) s = __fadd_rn(s, *q);
  const float m = __fdiv_rn(s, (float)rows);
  q = col;
  for (int r = 0; r < rows; r++, q += ldx) {
    const float d = __fsub_rn(*q, m);
    M2 = __fadd_rn(M2, __fmul_rn(d, d));
  }
  for (int r = 0; r < rows; r++, col += ldx) {
    const float y = norm_apply(*col, tb.x, tb.y, clip);
    *col = y;
    if (dstO) *dstO = y, dstO += K0;
  }
  if (part_m) part_m[0] = m, part_m[K0] = M2;
}

// the normalising tile (Tile contract: auv_policy_forward.h): the plain tile, raw, and behind a barrier of its own the column step
struct NormTile : PolPlainTile {
  const auv_policy_norm_t& s;
  struct Req {
    float2 tb;                       // (mean, inv_std) of this thread's first column
    __device__ __forceinline__ explicit Req(const PolAct&) {}
  };
  __device__ __forceinline__ explicit NormTile(const auv_policy_norm_t& s_) : PolPlainTile(s_.io), s(s_) {}
  template <class A>
  __device__ __forceinline__ void request(A, Req& r, float*, const PolAct&, const int) const {
    const int tid = threadIdx.x;
    r.tb = make_float2(0.0f, 1.0f);
    if (tid < io.obs_dim) r.tb = *(const float2*)(s.table + 2 * tid);
  }
  template <class A>
  __device__ __forceinline__ void fill(A, float* X, const PolAct& p, const Req& r, const int rows) const {
    const int K0 = io.obs_dim, ldx = pol_ldx(K0), tid = threadIdx.x, net = blockIdx.y;
    // ---- raw tile -> LDS ----
    pol_act_fill_obs(X, io, p, nullptr, rows);
    __syncthreads();
    // ---- moments of the raw rows, the normalised rows into the tile and the rollout ----
    float2 tb = r.tb;
    float* dstO = pol_act_obs_out(io, p, K0);
    const size_t slot = (size_t)p.t * (size_t)s.part_ld + (size_t)s.part_base + blockIdx.x;
    float* part_m = net == 0 ? s.part + slot * 2 * (size_t)K0 : nullptr;
    for (int c = tid; c < K0; c += POL_THREADS) {
      if (c != tid) tb = *(const float2*)(s.table + 2 * c);
      norm_tile_column(X + c, ldx, rows, K0, tb, s.clip_obs, dstO ? dstO + c : nullptr, part_m ? part_m + c : nullptr);
    }
    if (net == 0 && tid == 0) s.pcnt[slot] = rows;
  }
};

// grid (ceil(ne / 16), 2): blockIdx.y = 0 the policy net, 1 the value net
template <class A>
__global__ void __launch_bounds__(POL_THREADS, (POL_WAVES >= 8 ? 4 : 2)) k16_norm_act(PolActArgs<auv_policy_norm_t> pa) {   // (two workgroups per CU, as k6)
  pol_act_body<A, false, false>(pa, NormTile(pa.io));
}

// ---- the normalising expression on arbitrary rows, no network: out[j][c] = norm(X[idx ? idx[j] : j][c]) ----
struct NormRowsArgs {
  const float* X;
  const int64_t* idx;                // nullable
  const float* table;
  float* out;
  long long ldx, ldo;
  int32_t M, D;
  float clip;
};

__global__ void __launch_bounds__(256) k16_norm_rows(NormRowsArgs a) {
  const size_t total = (size_t)a.M * (size_t)a.D;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t j = i / (size_t)a.D;
    const int c = (int)(i - j * (size_t)a.D);
    const size_t row = a.idx ? (size_t)a.idx[j] : j;
    const float2 tb = *(const float2*)(a.table + 2 * c);
    a.out[j * (size_t)a.ldo + c] = norm_apply(a.X[row * (size_t)a.ldx + c], tb.x, tb.y, a.clip);
  }
}

// ---- Chan's pairwise merge of two sets of moments (count, mean, M2), fp64, every operation separately rounded ----
struct NormMom {
  double n, mean, M2;
};
__device__ __forceinline__ NormMom norm_merge(const NormMom a, const NormMom b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  NormMom r;
  const double tot = a.n + b.n;
  const double delta = b.mean - a.mean;
  r.n = tot;
  r.mean = a.mean + __ddiv_rn(delta * b.n, tot);
  r.M2 = (a.M2 + b.M2) + __ddiv_rn(((delta * delta) * a.n) * b.n, tot);
  return r;
}
// the 64 lane results as a tree (header comment): lane 0 holds the result
__device__ __forceinline__ NormMom norm_merge_wave(NormMom a) {
  for (int o = AUV_WAVE / 2; o >= 1; o >>= 1) {
    NormMom b;
    b.n = __shfl_down(a.n, o, AUV_WAVE), b.mean = __shfl_down(a.mean, o, AUV_WAVE), b.M2 = __shfl_down(a.M2, o, AUV_WAVE);
    a = norm_merge(a, b);                                          // (lanes >= o compute along; nobody reads them again)
  }
  return a;
}
__device__ __forceinline__ double norm_deviation(const NormMom m, const double eps) {
  return __dsqrt_rn(__ddiv_rn(m.M2, m.n) + eps);
}

// one wave per column: part [n_slots][2][D], pcnt [n_slots]; mom [D][3] = (count, mean, M2); table [D][2] = (mean, inv_std)
__global__ void __launch_bounds__(AUV_WAVE) k16_norm_fold(const float* __restrict__ part, const int32_t* __restrict__ pcnt, const int n_slots,
                                                         const int D, const double eps, double* __restrict__ mom, float* __restrict__ table) {
  const int c = blockIdx.x, lane = threadIdx.x;
  NormMom a = {0.0, 0.0, 0.0};
  for (int s = lane; s < n_slots; s += AUV_WAVE) {
    const int cnt = pcnt[s];
    if (cnt <= 0) continue;
    const float* q = part + (size_t)s * 2 * (size_t)D;
    const NormMom b = {(double)cnt, (double)q[c], (double)q[D + c]};
    a = norm_merge(a, b);
  }
  a = norm_merge_wave(a);
  if (lane == 0) {
    const NormMom run = {mom[3 * c], mom[3 * c + 1], mom[3 * c + 2]};
    const NormMom r = norm_merge(run, a);
    mom[3 * c] = r.n, mom[3 * c + 1] = r.mean, mom[3 * c + 2] = r.M2;
    table[2 * c] = (float)r.mean;
    table[2 * c + 1] = (float)__ddiv_rn(1.0, norm_deviation(r, eps));
  }
}

// ---- the reward pass ----
// one thread per environment, forwards in time: ret [N] carried across calls; rpart [N][2] = (mean, M2) of the environment's T returns
__global__ void __launch_bounds__(256) k16_return_env(const float* __restrict__ R, const float* __restrict__ Dn, const double gamma,
                                                    double* __restrict__ ret, double* __restrict__ rpart, const int T, const int N) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N) return;
  double g = ret[e], mean = 0.0, M2 = 0.0;
  for (int t = 0; t < T; t++) {
    const size_t q = (size_t)t * N + e;
    g = g * gamma + (double)R[q];
    const double d = g - mean;
    mean = mean + __ddiv_rn(d, (double)(t + 1));
    M2 = M2 + d * (g - mean);
    if (Dn[q] != 0.0f) g = 0.0;
  }
  ret[e] = g;
  rpart[2 * (size_t)e] = mean, rpart[2 * (size_t)e + 1] = M2;
}

// one wave: the N per-environment partials (T returns each) into the running return moments rmom [3] = (count, mean, M2)
__global__ void __launch_bounds__(AUV_WAVE) k16_return_merge(const double* __restrict__ rpart, const int T, const int N, double* __restrict__ rmom) {
  const int lane = threadIdx.x;
  NormMom a = {0.0, 0.0, 0.0};
  for (int e = lane; e < N; e += AUV_WAVE) {
    const NormMom b = {(double)T, rpart[2 * (size_t)e], rpart[2 * (size_t)e + 1]};
    a = norm_merge(a, b);
  }
  a = norm_merge_wave(a);
  if (lane == 0) {
    const NormMom run = {rmom[0], rmom[1], rmom[2]};
    const NormMom r = norm_merge(run, a);
    rmom[0] = r.n, rmom[1] = r.mean, rmom[2] = r.M2;
  }
}

// out[i] = min(max(R[i] / sd, -clip), clip), sd = (float)sqrt(M2 / count + eps); out may be R
__global__ void __launch_bounds__(256) k16_return_scale(const float* R, float* out, const size_t total, const double* __restrict__ rmom,
                                                      const double eps, const float clip) {
  const NormMom m = {rmom[0], rmom[1], rmom[2]};
  const float sd = (float)norm_deviation(m, eps);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256)
    out[i] = fminf(fmaxf(__fdiv_rn(R[i], sd), -clip), clip);
}

}  // namespace

// (h1, h2, h3): a listed hidden-width triple (the caller has checked); the LDS is k6's (auv_policy_lds_bytes)
static auto k16_act = [](auto a) { return k16_norm_act<decltype(a)>; };

hipError_t auv_policy_norm_prepare(int h1, int h2, int h3, int obs_dim) {
  return pol_act_prepare(h1, h2, h3, pol_lds_bytes_h(h1, h2, h3, obs_dim), k16_act);
}

void auv_launch_policy_norm(int h1, int h2, int h3, const auv_policy_norm_t& s, int e0, int ne, hipStream_t st, long long t_host,
                            long long gstep_host) {
  const PolActArgs<auv_policy_norm_t> pa = {s, e0, ne, t_host, gstep_host};
  pol_act_launch(h1, h2, h3, pa, pol_lds_bytes_h(h1, h2, h3, s.io.obs_dim), st, k16_act);
}

void auv_launch_norm_rows(const float* X, const int64_t* idx, long long ldx, const float* table, float clip_obs, float* out, long long ldo,
                          int M, int obs_dim, hipStream_t st) {
  NormRowsArgs a;
  a.X = X, a.idx = idx, a.table = table, a.out = out, a.ldx = ldx, a.ldo = ldo, a.M = M, a.D = obs_dim, a.clip = clip_obs;
  const size_t total = (size_t)M * (size_t)obs_dim;
  const size_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(k16_norm_rows, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, a);
}

void auv_launch_norm_fold(const float* part, const int32_t* pcnt, int n_slots, int obs_dim, double eps, double* mom, float* table,
                          hipStream_t st) {
  hipLaunchKernelGGL(k16_norm_fold, dim3(obs_dim), dim3(AUV_WAVE), 0, st, part, pcnt, n_slots, obs_dim, eps, mom, table);
}

void auv_launch_norm_returns(const float* R, const float* Dn, float* out, int T, int N, double gamma, float clip_reward, double eps, double* ret,
                             double* rpart, double* rmom, bool update, hipStream_t st) {
  if (update) {
    hipLaunchKernelGGL(k16_return_env, dim3((N + 255) / 256), dim3(256), 0, st, R, Dn, gamma, ret, rpart, T, N);
    hipLaunchKernelGGL(k16_return_merge, dim3(1), dim3(AUV_WAVE), 0, st, (const double*)rpart, T, N, rmom);
  }
  const size_t total = (size_t)T * (size_t)N;
  const size_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(k16_return_scale, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, R, out, total, (const double*)rmom,
                     eps, clip_reward);
}
