// K9 -- the policy outside the rollout: actor and / or critic of k6_policy.hip evaluated for M arbitrary observation rows by ONE
// launch (auv_policy_eval): no environment, no rollout position, no counters, no sampling.  What the reference asks of a trained
// agent in its enjoy / play / test modes -- agent.predict(obs, deterministic=True), scripts/run.py:175, 273, 567 -- plus the two
// questions a planner and an update ask: what is this state worth, how likely was this action.
//
// The matrix part is the forward pass k6_policy_act runs (auv_policy_forward.h: pol_trunk<false>, the same workgroup of 16 rows of ONE
// net and eight waves, the same LDS tiles) -- so the mean and the value of a row are the same k-ordered fmaf chains, bit for bit, as
// the rollout launch computes for that row (tests/test_gpu_policy_eval.py).  What this file holds is what differs: where rows come from
// (a strided matrix, optionally gathered through an index) and what is stored: the mean itself, the deterministic action (the shared
// action map applied to a = mu), the value, and log pi(a) of GIVEN actions (pol_logp, the function the rollout launch calls).
//
// Also here: the value-terminated score of a shooting planner's candidates (auv_plan_score_v), auv_plan_score's loop with one
// more term for a candidate that saw no done.
#include "auv_launch.h"
#include "auv_policy_forward.h"

namespace {

struct EvalArgs {
  auv_policy_eval_t ev;
  int32_t net0;                      // blockIdx.y = 0 evaluates this net (0 policy, 1 value): only the nets asked for are launched
  int32_t vec2;                      // every source row starts 8-byte aligned and holds an even number of floats (host-proven)
};

// rows of a strided matrix, optionally gathered through ev.idx, -> the tile.  V = float2: ldx and obs_dim even and the base 8-byte
// aligned, so no pair straddles two rows or an 8-byte boundary
template <class V>
__device__ __forceinline__ void eval_fill_rows(float* X, const int ldx, const auv_policy_eval_t& ev, const int r0, const int rows, const int tid) {
  constexpr int W = sizeof(V) / sizeof(float);
  const int K0 = ev.obs_dim;
  const size_t lds = (size_t)ev.ldx;
  for (int i = W * tid; i < rows * K0; i += W * POL_THREADS) {
    const int row = i / K0, c = i - row * K0;
    const size_t srow = ev.idx ? (size_t)ev.idx[r0 + row] : (size_t)(r0 + row);
    *(V*)(X + row * ldx + c) = *(const V*)(ev.X + srow * lds + c);
  }
}

// The launch's body, written once for every hidden-width triple A (PolArch, auv_policy_mfma.h).
template <class A>
__device__ __forceinline__ void policy_eval_body(const EvalArgs& ea) {
  extern __shared__ __align__(16) unsigned char smem[];
  const auv_policy_eval_t& ev = ea.ev;
  const int tid = threadIdx.x, wave = tid / AUV_WAVE, lane = tid % AUV_WAVE;
  const int net = ea.net0 + blockIdx.y;
  const int M = ev.M;
  const int r0 = blockIdx.x * POL_ROWS;                          // first row of the tile (M <= 2^31 - 1: no overflow)
  const int K0 = ev.obs_dim, K0p = pol_pad16(K0);
  float* X = (float*)smem;
  const int ldx = pol_ldx(K0);
  const PolNet nw = pol_net_ptrs<A>(ev.params + (size_t)net * pol_net_floats<A>(K0), K0);
  PolW<A::H1 / 16, false> w1;
  pol_prefetch(w1, nw.W1, nw.b1, K0p, wave, lane);                 // (in flight while the rows are fetched)
  // ---- the tile's rows -> LDS; padding columns and the rows past M stay zero ----
  const int rows = (M - r0 < POL_ROWS) ? M - r0 : POL_ROWS;
  pol_zero_tile(X, ldx, tid);
  __syncthreads();
  if (ea.vec2) eval_fill_rows<float2>(X, ldx, ev, r0, rows, tid);
  else eval_fill_rows<float>(X, ldx, ev, r0, rows, tid);
  const bool want_lp = ev.logp != nullptr;                       // (uniform)
  f32x4 o[1][POL_MT];
  const float ls = pol_trunk<false, A>(X, K0, nw, w1, (wave == 0 && net == 0 && want_lp) ? ev.params + 2 * pol_net_floats<A>(K0) : nullptr, wave, lane, o);
  if (wave != 0) return;
  const int n = lane & 15, g = lane >> 4;
  if (net == 0) {
    const float sigma = expf(ls);
    const PolActMap map = pol_act_map(ev, pol_comp(lane));
#pragma unroll
    for (int u = 0; u < POL_MT; u++)
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int rr = 16 * u + 4 * g + i;                       // row inside the tile
        const int row = r0 + rr;
        const bool live = n < 2 && rr < rows;
        const float mu = o[0][u][i];
        float lp = 0.0f;
        if (want_lp) {
          // log pi(a): the rollout launch's own function (the bits of LP[t] for the a the rollout stored)
          const float a = live ? ev.A[2 * (size_t)row + n] : mu;
          lp = pol_logp(a, mu, sigma, ls);
        }
        if (live) {
          if (ev.mu) ev.mu[2 * (size_t)row + n] = mu;
          if (ev.action) ev.action[(size_t)row * (size_t)ev.action_ld + n] = map(mu);
          if (want_lp && n == 0) ev.logp[row] = lp;
        }
      }
  } else if (n == 0) {
#pragma unroll
    for (int u = 0; u < POL_MT; u++)
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int rr = 16 * u + 4 * g + i;
        if (rr < rows) ev.value[r0 + rr] = o[0][u][i];
      }
  }
}

// grid (ceil(M / 16), nets launched)
template <class A>
__global__ void __launch_bounds__(POL_THREADS, (POL_WAVES >= 8 ? 4 : 2)) k9_policy_eval(EvalArgs ea) {   // (two workgroups per CU, as k6)
  policy_eval_body<A>(ea);
}

// ---- the value-terminated score of a shooting planner's candidates ----
// auv_plan_score's loop (k7_snapshot.hip) -- score[e] = sum over t of disc_t * reward[t][e] up to and including the first done, every
// product and sum rounded to float32 in increasing t -- and, for an environment with NO done in [0, T), one more rounded product and
// one more rounded sum, last in order: + disc_T * terminal[e].  A candidate that saw a done never reads its terminal value.
__device__ __forceinline__ float plan_score_env_v(const float* __restrict__ reward, const uint8_t* __restrict__ done, const float* __restrict__ terminal,
                                                  const int T, const int n, const int e, const float gamma) {
  float s = 0.0f, disc = 1.0f;
  for (int t = 0; t < T; t++) {
    s = __fadd_rn(s, __fmul_rn(disc, reward[(size_t)t * n + e]));
    if (done[(size_t)t * n + e]) return s;
    disc = __fmul_rn(disc, gamma);
  }
  return __fadd_rn(s, __fmul_rn(disc, terminal[e]));
}

// (score, index) a beats b: a valid score (not NaN) beats none; the larger score wins; the lower index wins a tie
#define PLANV_NONE 0x7fffffff
__device__ __forceinline__ bool planv_beats(const float sa, const int ia, const float sb, const int ib) {
  if (ia == PLANV_NONE) return false;
  if (ib == PLANV_NONE) return true;
  return sa > sb || (sa == sb && ia < ib);
}

// The geometry of k7_plan_score: lanes run across environments; a group of 1, 2, .. 64 (a power of two) environments shares its wave
// (`span` = group), any other group size has a wave to itself (`span` = 64).
__global__ void __launch_bounds__(AUV_WAVE) k9_plan_score_v(const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                            const float* __restrict__ terminal, const int T, const int n, const int group,
                                                            const int span, const float gamma, float* __restrict__ score,
                                                            int32_t* __restrict__ best) {
  const int lane = threadIdx.x;
  float bs = 0.0f;
  int bi = PLANV_NONE;
  int g;                                  // this lane's group
  if (span < AUV_WAVE || group == AUV_WAVE) {
    const int e = blockIdx.x * AUV_WAVE + lane;
    g = e / group;
    if (e < n) {
      const float s = plan_score_env_v(reward, done, terminal, T, n, e, gamma);
      score[e] = s;
      if (s == s) bs = s, bi = e - g * group;
    }
  } else {
    g = blockIdx.x;
    for (int k = lane; k < group; k += AUV_WAVE) {
      const int e = g * group + k;
      const float s = plan_score_env_v(reward, done, terminal, T, n, e, gamma);
      score[e] = s;
      if (s == s && planv_beats(s, k, bs, bi)) bs = s, bi = k;
    }
  }
  for (int off = 1; off < span; off <<= 1) {
    const float os = __shfl_xor(bs, off, AUV_WAVE);
    const int oi = __shfl_xor(bi, off, AUV_WAVE);
    if (planv_beats(os, oi, bs, bi)) bs = os, bi = oi;
  }
  const int first = span < AUV_WAVE ? (lane % span) : lane;
  if (first == 0 && (long long)g * group < n) best[g] = bi == PLANV_NONE ? 0 : bi;
}

}  // namespace

// (h1, h2, h3): a listed hidden-width triple (the caller has checked)
hipError_t auv_policy_eval_prepare(int h1, int h2, int h3, int obs_dim) {
  const size_t b = pol_lds_bytes_h(h1, h2, h3, obs_dim);
  if (b <= 64 * 1024) return hipSuccess;
  hipError_t e = hipErrorInvalidValue;
  pol_arch_visit(h1, h2, h3, [&](auto a) {
    e = hipFuncSetAttribute((const void*)k9_policy_eval<decltype(a)>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
  });
  return e;
}

// want_pi / want_v: which nets have an output asked for (at least one; the caller has checked)
void auv_launch_policy_eval(int h1, int h2, int h3, const auv_policy_eval_t& ev, bool want_pi, bool want_v, hipStream_t st) {
  EvalArgs ea;
  ea.ev = ev;
  ea.net0 = want_pi ? 0 : 1;
  ea.vec2 = ((ev.ldx & 1) == 0 && (ev.obs_dim & 1) == 0 && ((uintptr_t)ev.X & 7) == 0) ? 1 : 0;
  const dim3 grid((unsigned)(((long long)ev.M + POL_ROWS - 1) / POL_ROWS), (want_pi ? 1 : 0) + (want_v ? 1 : 0)), block(POL_THREADS);
  const size_t lds = pol_lds_bytes_h(h1, h2, h3, ev.obs_dim);
  pol_arch_visit(h1, h2, h3, [&](auto a) { hipLaunchKernelGGL((k9_policy_eval<decltype(a)>), grid, block, lds, st, ea); });
}

void auv_launch_plan_score_v(const float* reward, const uint8_t* done, const float* terminal, int T, int n, int group, float gamma, float* score,
                             int32_t* best, hipStream_t st) {
  const bool packed = group <= AUV_WAVE && (group & (group - 1)) == 0;
  const int span = packed ? group : AUV_WAVE;
  const int grid = packed ? (n + AUV_WAVE - 1) / AUV_WAVE : n / group;
  hipLaunchKernelGGL(k9_plan_score_v, dim3(grid), dim3(AUV_WAVE), 0, st, reward, done, terminal, T, n, group, span, gamma, score, best);
}
