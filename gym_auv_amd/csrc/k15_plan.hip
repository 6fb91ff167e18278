// k15_plan.hip — the shooting planner's sampler and refit (auv_plan_sample / auv_plan_refit; contracts: include/auv_hip.h): what
// gym_auv_amd/planning.py otherwise does with a chain of small torch launches around every step_multi.
//
// The sampler is element-wise: one lane per float of the ring, so every ring row is stored coalesced; its noise is the population
// kernels' counter-based draw (auv_noise.h), a function of (seed, draw, environment, 2 t + j) alone.  The refit gives one workgroup
// to a group of K <= AUV_PLAN_MAX_GROUP candidates: the scores go to LDS, the elite is found by rank (K comparisons per candidate in
// the total order of auv_plan.h, the scorer's own), and one lane per (t, j) then runs the sums in the order the contract states.
// All float32 arithmetic is spelled with the _rn intrinsics (the square root excepted, see there): no contraction, no reassociation.
#include "auv_device.h"
#include "auv_launch.h"
#include "auv_noise.h"
#include "auv_plan.h"

#define PLAN_THREADS 256

namespace {

// grid ceil(T * n * 2 / PLAN_THREADS); c = pop_eps_scale()
__global__ void __launch_bounds__(PLAN_THREADS) k15_plan_sample(const AuvPlanSample a, const float c) {
  const unsigned int row = 2u * (unsigned int)a.n;                 // floats of a ring row (T * row < 2^31: host-checked)
  const unsigned int idx = blockIdx.x * PLAN_THREADS + threadIdx.x;
  if (idx >= (unsigned int)a.T * row) return;
  const unsigned int t = idx / row, i = idx - t * row;             // i = 2 e + j
  const unsigned int e = i >> 1, j = i & 1u;
  const unsigned int b = e / (unsigned int)a.group, k = e - b * (unsigned int)a.group;
  const unsigned int B = (unsigned int)a.n / (unsigned int)a.group;
  const bool fresh = a.reset != nullptr && a.reset[b] != 0;
  unsigned int tt = fresh ? t : t + (unsigned int)a.shift;
  if (tt > (unsigned int)a.T - 1u) tt = (unsigned int)a.T - 1u;
  const size_t at = ((size_t)tt * B + b) * 2 + j;
  float v = fresh ? a.mean0[at] : a.mean[at];
  if (k != 0) {                                                    // (candidate 0: the mean sequence itself)
    const float s = fresh ? a.sigma0[at] : a.sigma[at];
    const float eps = pop_eps(pop_key(a.seed, a.draw), e, 2u * t + j, c);
    v = __fadd_rn(v, __fmul_rn(s, eps));
  }
  const float lo = j ? a.lo[1] : a.lo[0], hi = j ? a.hi[1] : a.hi[0];
  a.ring[idx] = fmaxf(fminf(v, hi), lo);
}

// grid B (one workgroup per group), PLAN_THREADS threads
__global__ void __launch_bounds__(PLAN_THREADS) k15_plan_refit(const AuvPlanRefit a) {
  __shared__ float s_val[AUV_PLAN_MAX_GROUP];                      // the group's scores; MPPI: then its weights
  __shared__ int32_t s_list[AUV_PLAN_MAX_GROUP];                   // CEM: the elite, ascending candidate index
  __shared__ uint8_t s_elite[AUV_PLAN_MAX_GROUP];                  // CEM: candidate k is of the elite
  const int tid = threadIdx.x, K = a.group, T = a.T;
  const size_t b = blockIdx.x, B = (size_t)(a.n / K);
  const size_t row = 2 * (size_t)a.n;
  const float* ring = a.ring + b * (size_t)K * 2;                  // candidate k, step t, component j: ring[t * row + 2 k + j]
  const float* score = a.score + b * (size_t)K;
  // ---- the chosen sequence and its predicted score ----
  int bi = a.best[b];
  bi = bi < 0 ? 0 : (bi > K - 1 ? K - 1 : bi);
  if (a.chosen)
    for (int tj = tid; tj < 2 * T; tj += PLAN_THREADS)
      a.chosen[((size_t)(tj >> 1) * B + b) * 2 + (tj & 1)] = ring[(size_t)(tj >> 1) * row + 2 * bi + (tj & 1)];
  if (a.predicted && tid == 0) a.predicted[b] = score[bi];
  if (!a.mean_out) return;                                         // (uniform: a launch argument)
  for (int k = tid; k < K; k += PLAN_THREADS) s_val[k] = score[k];
  __syncthreads();
  if (a.method == AUV_PLAN_CEM) {
    const int E = a.n_elite;
    for (int k = tid; k < K; k += PLAN_THREADS) {                  // rank = candidates in front of k; the elite: rank < E
      const float sk = s_val[k];
      int r = 0;
      for (int i = 0; i < K; i++) r += (i != k && plan_ranks_before(s_val[i], i, sk, k)) ? 1 : 0;
      s_elite[k] = r < E ? 1 : 0;
    }
    __syncthreads();
    for (int k = tid; k < K; k += PLAN_THREADS)                    // an elite candidate's place: the elite in front of it
      if (s_elite[k]) {
        int p = 0;
        for (int i = 0; i < k; i++) p += s_elite[i];
        s_list[p] = k;                                             // (p < E: exactly E candidates have rank < E)
      }
    __syncthreads();
    const float fe = (float)E;
    for (int tj = tid; tj < 2 * T; tj += PLAN_THREADS) {
      const float* src = ring + (size_t)(tj >> 1) * row + (tj & 1);
      float s = 0.0f;
      for (int i = 0; i < E; i++) s = __fadd_rn(s, src[2 * s_list[i]]);
      const float mean = __fdiv_rn(s, fe);
      float q = 0.0f;
      for (int i = 0; i < E; i++) {
        const float d = __fsub_rn(src[2 * s_list[i]], mean);
        q = __fadd_rn(q, __fmul_rn(d, d));
      }
      const size_t at = ((size_t)(tj >> 1) * B + b) * 2 + (tj & 1);
      a.mean_out[at] = mean;
      // (sqrtf, not __fsqrt_rn: this compiler's __fsqrt_rn is the native approximation, an ulp off now and then; sqrtf is the
      // correctly rounded root unless the file is built with -fno-hip-fp32-correctly-rounded-divide-sqrt, which the Makefile does not)
      a.sigma_out[at] = fmaxf(sqrtf(__fdiv_rn(q, fe)), a.sigma_min);
    }
    return;
  }
  // ---- MPPI ----
  float smax = 0.0f;
  bool have = false;
  for (int i = 0; i < K; i++) {                                    // (LDS broadcast reads: every lane runs the same loop)
    const float s = s_val[i];
    if (s == s && (!have || s > smax)) smax = s, have = true;
  }
  __syncthreads();
  for (int k = tid; k < K; k += PLAN_THREADS) {
    const float s = s_val[k];
    float w = 0.0f;
    if (s == s) w = s == smax ? 1.0f : expf(__fdiv_rn(__fsub_rn(s, smax), a.lambda));
    s_val[k] = w;
  }
  __syncthreads();
  for (int tj = tid; tj < 2 * T; tj += PLAN_THREADS) {
    const size_t at = ((size_t)(tj >> 1) * B + b) * 2 + (tj & 1);
    float mean = a.mean_in[at];
    if (have) {
      const float* src = ring + (size_t)(tj >> 1) * row + (tj & 1);
      float num = 0.0f, den = 0.0f;
      for (int k = 0; k < K; k++) {
        const float w = s_val[k];
        num = __fadd_rn(num, __fmul_rn(w, src[2 * k]));
        den = __fadd_rn(den, w);
      }
      mean = __fdiv_rn(num, den);
    }
    a.mean_out[at] = mean;
    a.sigma_out[at] = a.sigma_in[at];
  }
}

}  // namespace

void auv_launch_plan_sample(const AuvPlanSample& a, hipStream_t st) {
  const long long total = 2ll * a.T * a.n;
  hipLaunchKernelGGL(k15_plan_sample, dim3((unsigned)((total + PLAN_THREADS - 1) / PLAN_THREADS)), dim3(PLAN_THREADS), 0, st, a, pop_eps_scale());
}

void auv_launch_plan_refit(const AuvPlanRefit& a, hipStream_t st) {
  hipLaunchKernelGGL(k15_plan_refit, dim3((unsigned)(a.n / a.group)), dim3(PLAN_THREADS), 0, st, a);
}
