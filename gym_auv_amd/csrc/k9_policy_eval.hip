// K9 -- the policy outside the rollout: actor and / or critic of k6_policy.hip evaluated for M arbitrary observation rows by ONE
// launch (auv_policy_eval): no environment, no rollout position, no counters, no sampling.  What the reference asks of a trained
// agent in its enjoy / play / test modes -- agent.predict(obs, deterministic=True), scripts/run.py:175, 273, 567 -- plus the two
// questions a planner and an update ask: what is this state worth, how likely was this action.
//
// The matrix part IS k6_policy_act's exact-f32 path: the same workgroup (16 rows of ONE net, eight waves), the same LDS tiles and
// row strides, pol_prefetch / pol_layer in the same order with the same template arguments -- so the mean and the value of a row are
// the same k-ordered fmaf chains, bit for bit, as the rollout launch computes for that row (tests/test_gpu_policy_eval.py).  What
// differs is where rows come from (a strided matrix, optionally gathered through an index) and the epilogue: the mean itself, the
// deterministic action (k6's action map applied to a = mu), the value, and log pi(a) of GIVEN actions written as k6 writes it.
//
// Also here: the value-terminated score of a shooting planner's candidates (auv_plan_score_v), auv_plan_score's loop with one
// more term for a candidate that saw no done.
#include "auv_policy_mfma.h"

namespace {

struct EvalArgs {
  auv_policy_eval_t ev;
  int32_t net0;                      // blockIdx.y = 0 evaluates this net (0 policy, 1 value): only the nets asked for are launched
  int32_t vec2;                      // every source row starts 8-byte aligned and holds an even number of floats (host-proven)
};

// grid (ceil(M / 16), nets launched)
__global__ void __launch_bounds__(POL_THREADS, (POL_WAVES >= 8 ? 4 : 2)) k9_policy_eval(EvalArgs ea) {   // (two workgroups per CU, as k6)
  extern __shared__ __align__(16) unsigned char smem[];
  const auv_policy_eval_t& ev = ea.ev;
  const int tid = threadIdx.x, wave = tid / AUV_WAVE, lane = tid % AUV_WAVE;
  const int net = ea.net0 + blockIdx.y;
  const int M = ev.M;
  const int r0 = blockIdx.x * POL_ROWS;                          // first row of the tile (M <= 2^31 - 1: no overflow)
  const int K0 = ev.obs_dim, K0p = pol_pad16(K0);
  const int ldx = K0p + 8, ld1 = POL_H1 + 8, ld2 = POL_H2 + 8, ld3 = POL_H3 + 8;
  float* X = (float*)smem;
  float* Y1 = X + pol_lds_x_floats(K0);
  float* Y2 = X;                                                 // (X is dead once layer 1 is through: a barrier lies in between)
  float* Y3 = Y1;                                                // (Y1 is dead once layer 2 is through)
  const float* P = ev.params + (size_t)net * pol_net_floats(K0);
  const float* W1 = P;
  const float* b1 = W1 + (size_t)POL_H1 * K0p;
  const float* W2 = b1 + POL_H1;
  const float* b2 = W2 + (size_t)POL_H2 * POL_H1;
  const float* W3 = b2 + POL_H2;
  const float* b3 = W3 + (size_t)POL_H3 * POL_H2;
  const float* W4 = b3 + POL_H3;
  const float* b4 = W4 + (size_t)POL_OUT * POL_H3;
  PolW<POL_H1 / 16, false> w1;
  PolW<POL_H2 / 16, false> w2;
  PolW<POL_H3 / 16, false> w3;
  PolW<1, false> w4;
  pol_prefetch(w1, W1, b1, K0p, wave, lane);                       // (in flight while the rows are fetched)
  // ---- the tile's rows -> LDS; padding columns and the rows past M stay zero ----
  const int rows = (M - r0 < POL_ROWS) ? M - r0 : POL_ROWS;
  for (int i = tid; i < POL_ROWS * (ldx / 2); i += POL_THREADS) *(float2*)(X + 2 * i) = make_float2(0.0f, 0.0f);
  __syncthreads();
  const size_t lds = (size_t)ev.ldx;
  if (ea.vec2) {
    // two floats per lane: ldx and obs_dim even and the base 8-byte aligned, so no pair straddles two rows or an 8-byte boundary
    for (int i = 2 * tid; i < rows * K0; i += 2 * POL_THREADS) {
      const int row = i / K0, c = i - row * K0;
      const size_t srow = ev.idx ? (size_t)ev.idx[r0 + row] : (size_t)(r0 + row);
      *(float2*)(X + row * ldx + c) = *(const float2*)(ev.X + srow * lds + c);
    }
  } else {
    for (int i = tid; i < rows * K0; i += POL_THREADS) {
      const int row = i / K0, c = i - row * K0;
      const size_t srow = ev.idx ? (size_t)ev.idx[r0 + row] : (size_t)(r0 + row);
      X[row * ldx + c] = ev.X[srow * lds + c];
    }
  }
  __syncthreads();
  pol_prefetch(w2, W2, b2, POL_H1, wave, lane);                    // (the next layer's weights: in flight during this layer)
  pol_layer<POL_H1 / 16, 1, false, false>(X, ldx, w1, b1, K0p, wave, lane, Y1, ld1, nullptr);
  __syncthreads();
  pol_prefetch(w3, W3, b3, POL_H2, wave, lane);
  pol_layer<POL_H2 / 16, 1, false, false>(Y1, ld1, w2, b2, POL_H1, wave, lane, Y2, ld2, nullptr);
  __syncthreads();
  pol_prefetch(w4, W4, b4, POL_H3, wave, lane);
  // (the log-std with them: ahead of the barrier, so that the request is not moved down to its use)
  const int nc = (lane & 15) < 2 ? (lane & 15) : 0;
  const bool want_lp = ev.logp != nullptr;                       // (uniform)
  float ls = 0.0f;
  if (wave == 0 && net == 0 && want_lp) ls = (ev.params + 2 * pol_net_floats(K0))[nc];
  pol_layer<POL_H3 / 16, 2, false, false>(Y2, ld2, w3, b3, POL_H2, wave, lane, Y3, ld3, nullptr);
  __syncthreads();
  if (wave != 0) return;
  f32x4 o[1][POL_MT];
  pol_layer<1, 2, true, false>(Y3, ld3, w4, b4, POL_H3, 0, lane, nullptr, 0, o);
  const int n = lane & 15, g = lane >> 4;
  if (net == 0) {
    const float sigma = expf(ls);
    // the action map of this lane's component: launch arguments picked by a select, as in k6_policy_act
    float cl0 = ev.clip_lo[0], cl1 = ev.clip_lo[1], ch0 = ev.clip_hi[0], ch1 = ev.clip_hi[1];
    float am0 = ev.act_mid[0], am1 = ev.act_mid[1], ah0 = ev.act_half[0], ah1 = ev.act_half[1];
    asm volatile("" : "+s"(cl0), "+s"(cl1), "+s"(ch0), "+s"(ch1), "+s"(am0), "+s"(am1), "+s"(ah0), "+s"(ah1));   // (or the selects become indexed loads)
    const float clip_lo = nc ? cl1 : cl0, clip_hi = nc ? ch1 : ch0, act_mid = nc ? am1 : am0, act_half = nc ? ah1 : ah0;
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
          // log pi(a): k6_policy.hip's expression, operation for operation (the bits of LP[t] for the a the rollout stored)
          const float a = live ? ev.A[2 * (size_t)row + n] : mu;
          const float z = (a - mu) / sigma;
          lp = -0.5f * z * z - ls - POL_LOG_SQRT_2PI;
          lp += __shfl_xor(lp, 1, AUV_WAVE);                     // the two components sit on neighbouring lanes
        }
        if (live) {
          if (ev.mu) ev.mu[2 * (size_t)row + n] = mu;
          if (ev.action) {
            const float ac = fminf(fmaxf(mu, clip_lo), clip_hi);
            ev.action[(size_t)row * (size_t)ev.action_ld + n] = act_mid + act_half * ac;
          }
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

hipError_t auv_policy_eval_prepare(int obs_dim) {
  const size_t b = pol_lds_bytes(obs_dim);
  if (b <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute((const void*)k9_policy_eval, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
}

// want_pi / want_v: which nets have an output asked for (at least one; the caller has checked)
void auv_launch_policy_eval(const auv_policy_eval_t& ev, bool want_pi, bool want_v, hipStream_t st) {
  EvalArgs ea;
  ea.ev = ev;
  ea.net0 = want_pi ? 0 : 1;
  ea.vec2 = ((ev.ldx & 1) == 0 && (ev.obs_dim & 1) == 0 && ((uintptr_t)ev.X & 7) == 0) ? 1 : 0;
  const dim3 grid((unsigned)(((long long)ev.M + POL_ROWS - 1) / POL_ROWS), (want_pi ? 1 : 0) + (want_v ? 1 : 0)), block(POL_THREADS);
  hipLaunchKernelGGL(k9_policy_eval, grid, block, pol_lds_bytes(ev.obs_dim), st, ea);
}

void auv_launch_plan_score_v(const float* reward, const uint8_t* done, const float* terminal, int T, int n, int group, float gamma, float* score,
                             int32_t* best, hipStream_t st) {
  const bool packed = group <= AUV_WAVE && (group & (group - 1)) == 0;
  const int span = packed ? group : AUV_WAVE;
  const int grid = packed ? (n + AUV_WAVE - 1) / AUV_WAVE : n / group;
  hipLaunchKernelGGL(k9_plan_score_v, dim3(grid), dim3(AUV_WAVE), 0, st, reward, done, terminal, T, n, group, span, gamma, score, best);
}
