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

// (EvalArgs, the gather of the tile's rows and the launch's body, policy_eval_body: auv_policy_forward.h, shared with k17's squashed
// evaluation)
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
