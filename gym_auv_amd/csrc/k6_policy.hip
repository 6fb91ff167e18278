// K6 -- the policy in the loop: actor and critic of the reference's PPO set-up evaluated for a sub-batch of
// environments by ONE launch on the sub-batch's stream, straight from the observation rows the step kernel has just
// written, with sampling, log-probability, action clipping and the rollout stores in the epilogue.
//
// Reference: scripts/run.py:332-357 -- PPO2(MlpPolicy, net_arch [256, 128, 64] for policy and value function, tanh),
// a diagonal Gaussian over the two actions; what stable-baselines evaluates per environment step through
// SubprocVecEnv (run.py:293-296).  The torch modules of examples/ppo.py (ActorCritic) are the numerical reference
// (tests/test_gpu_policy.py: <= 1e-5).
//
// Shape of the work: [rows, obs_dim] x [obs_dim -> 256 -> 128 -> 64 -> out] twice, rows ~ 1024 per call: small GEMMs
// whose weights (0.7 MB for both nets) every workgroup streams from L2 while 1.45 GFLOP per 4096 rows go to the
// matrix pipe -- which the environment's own kernels never touch (they are VALU / latency bound), so policy and
// sweeps of different chains overlap on a CU.  One workgroup = 16 rows (one MFMA M-tile) of ONE net, eight waves (the launch
// is bound by the latencies of its weight loads and MFMA chains, not by a pipe: four waves per workgroup left the
// matrix pipe 35 % busy -- profiles/r04/pmc_policy.txt -- so the SIMDs get more waves to switch between):
//   * the observation tile goes to LDS once (and, from there, into the rollout's O[t]);
//   * a layer's 16-column n-tiles are dealt round-robin to the waves; v_mfma_f32_16x16x4_f32 (exact f32, a k-ordered fmaf
//     chain per output) with A from LDS and B = the weight rows straight from global memory as float4 (lane (n, g) reads
//     W[n][16 J + 4 g .. + 3]: A's lane (m, g) reads the same four k, so a super-step of 16 k is one 16-byte load per
//     operand and four MFMAs per n-tile; the k order inside a super-step is permuted identically on both sides);
//   * bias + tanh in the epilogue of each layer, activations stay in LDS;
//   * last layer: one n-tile (outputs padded to 16); its epilogue samples a = mu + sigma eps (counter-based generator,
//     Box-Muller), forms log pi(a), maps a into the action space into the env's action buffer, and stores the transition.
// Optional (flag): nothing else -- a bf16 variant would run the matrix pipe 16x faster but is not the reference's arithmetic.
#include "auv_launch.h"
#include "auv_policy_forward.h"

namespace {

// (LDS: pol_lds_x_floats / pol_lds_bytes in auv_policy_mfma.h; the forward pass and the frame of an act launch -- rollout position,
// transition, sampling epilogue, counters: auv_policy_forward.h, shared with k9, k11 and k12)
struct PolicyArgs {
  auv_policy_io_t io;
  int32_t e0, ne;
  long long t_host, gstep_host;      // >= 0: the host names the rollout position and the generator's step (auv_policy_rollout: a plain
                                     // loop of launches); -1: both live on the device (io.ctr) and the launch moves them on itself
};

// The launch's body, written once for every hidden-width triple A (PolArch, auv_policy_mfma.h).
template <class A, bool BF>
__device__ __forceinline__ void policy_act_body(const PolicyArgs& pa) {
  extern __shared__ __align__(16) unsigned char smem[];
  const auv_policy_io_t& io = pa.io;
  const int tid = threadIdx.x, wave = tid / AUV_WAVE, lane = tid % AUV_WAVE;
  const int net = blockIdx.y;
  const int K0 = io.obs_dim, K0p = pol_pad16(K0);
  float* X = (float*)smem;
  const PolAct p = pol_act_begin(io, pa.e0, pa.ne, pa.t_host, pa.gstep_host);
  if (p.act) {
    PolNet nw = pol_net_ptrs<A>(io.params + (size_t)net * pol_net_floats<A>(K0), K0);
    if (BF) {
      // bf16 weights: the four matrices of a net back to back, half the floats each (biases and log_std stay in `params`)
      const float* Q = (const float*)io.params_bf16 + (size_t)net * (pol_net_floats<A>(K0) - A::H1 - A::H2 - A::H3 - POL_OUT) / 2;
      nw.W1 = Q;
      nw.W2 = nw.W1 + (size_t)A::H1 * K0p / 2;
      nw.W3 = nw.W2 + (size_t)A::H2 * A::H1 / 2;
      nw.W4 = nw.W3 + (size_t)A::H3 * A::H2 / 2;
    }
    PolW<A::H1 / 16, BF> w1;
    pol_prefetch(w1, nw.W1, nw.b1, K0p, wave, lane);                 // (in flight while the observation tile is fetched)
    // ---- observation tile -> LDS (zero padded), and into the rollout (policy workgroup) ----
    const int rows = (p.cnt - p.r0 < POL_ROWS) ? p.cnt - p.r0 : POL_ROWS;
    pol_zero_tile(X, pol_ldx(K0), tid);
    __syncthreads();
    pol_act_fill_obs(X, io, p, pol_act_obs_out(io, p, K0), rows);
    f32x4 o[1][POL_MT];
    const float ls = pol_trunk<BF, A>(X, K0, nw, w1, (wave == 0 && net == 0) ? io.params + 2 * pol_net_floats<A>(K0) : nullptr, wave, lane, o);
    if (wave == 0) pol_act_sample(io, p, o, ls, lane);
  }
  pol_act_end(io, p);
}

// grid (ceil(ne / 16), 2): blockIdx.y = 0 the policy net, 1 the value net.  BF (bf16 weights) is instantiated for the reference's triple only
template <class A, bool BF>
__global__ void __launch_bounds__(POL_THREADS, (POL_WAVES >= 8 ? 4 : 2)) k6_policy_act(PolicyArgs pa) {   // (two workgroups per CU)
  policy_act_body<A, BF>(pa);
}

// Generalised advantage estimation over a rollout (what stable-baselines' PPO2 runner does on the host after n_steps,
// scripts/run.py:341-346: gamma 0.999, lam 0.98): one lane per environment walks its T transitions backwards, the loads of a
// wave are consecutive environments of one rollout row.  adv[t] = delta_t + gamma lam (1 - done_t) adv[t + 1],
// delta_t = r_t + gamma v_{t+1} (1 - done_t) - v_t; ret = adv + v.
__global__ void __launch_bounds__(256) k6_gae(const float* __restrict__ R, const float* __restrict__ V, const float* __restrict__ Dn,
                                             const float* __restrict__ last_v, const float gamma, const float lam,
                                             float* __restrict__ adv, float* __restrict__ ret, const int T, const int N) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N) return;
  float nv = last_v[e], gae = 0.0f;
  for (int t = T - 1; t >= 0; t--) {
    const size_t q = (size_t)t * N + e;
    const float v = V[q], nd = 1.0f - Dn[q];
    const float delta = R[q] + gamma * nv * nd - v;
    gae = delta + gamma * lam * nd * gae;
    adv[q] = gae;
    ret[q] = gae + v;
    nv = v;
  }
}

}  // namespace

void auv_launch_gae(const float* R, const float* V, const float* Dn, const float* last_v, float gamma, float lam, float* adv, float* ret,
                    int T, int N, hipStream_t st) {
  hipLaunchKernelGGL(k6_gae, dim3((N + 255) / 256), dim3(256), 0, st, R, V, Dn, last_v, gamma, lam, adv, ret, T, N);
}

// ---- host side: every function takes the hidden-width triple (h1, h2, h3), a listed one (the caller has checked) ----
size_t auv_policy_param_floats_impl(int h1, int h2, int h3, int obs_dim) { return 2 * pol_net_floats_h(h1, h2, h3, obs_dim) + 4; }
size_t auv_policy_lds_bytes(int h1, int h2, int h3, int obs_dim) { return pol_lds_bytes_h(h1, h2, h3, obs_dim); }

// (the reference's triple also runs on bf16 weights: the launch picks that variant by io.params_bf16, which is NULL for every other triple)
hipError_t auv_policy_prepare(int h1, int h2, int h3, int obs_dim) {
  const size_t b = pol_lds_bytes_h(h1, h2, h3, obs_dim);
  if (b <= 64 * 1024) return hipSuccess;
  hipError_t e = hipErrorInvalidValue;
  pol_arch_visit(h1, h2, h3, [&](auto a) {
    e = hipFuncSetAttribute((const void*)k6_policy_act<decltype(a), false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
  });
  if (e != hipSuccess || !pol_arch_is_ref(h1, h2, h3)) return e;
  return hipFuncSetAttribute((const void*)k6_policy_act<PolArchRef, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
}

void auv_launch_policy(int h1, int h2, int h3, const auv_policy_io_t& io, int e0, int ne, hipStream_t st, long long t_host, long long gstep_host) {
  PolicyArgs pa;
  pa.io = io, pa.e0 = e0, pa.ne = ne;
  pa.t_host = t_host, pa.gstep_host = gstep_host;
  const dim3 grid((ne + POL_ROWS - 1) / POL_ROWS, 2), block(POL_THREADS);
  const size_t lds = pol_lds_bytes_h(h1, h2, h3, io.obs_dim);
  if (io.params_bf16 && pol_arch_is_ref(h1, h2, h3)) {
    hipLaunchKernelGGL((k6_policy_act<PolArchRef, true>), grid, block, lds, st, pa);
    return;
  }
  pol_arch_visit(h1, h2, h3, [&](auto a) { hipLaunchKernelGGL((k6_policy_act<decltype(a), false>), grid, block, lds, st, pa); });
}
