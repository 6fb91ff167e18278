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

// (LDS: pol_lds_x_floats / pol_lds_bytes in auv_policy_mfma.h; the forward pass, the body of an act launch and its Tile contract:
// auv_policy_forward.h.  This launch forms the plain tile; all this file adds is where the bf16 weights lie.)
template <bool BF>
struct PolicyTile : PolPlainTile {
  using PolPlainTile::PolPlainTile;
  template <class A>
  __device__ __forceinline__ void weights(A, PolNet& nw, const int net, const int K0p) const {
    if (BF) {
      // bf16 weights: the four matrices of a net back to back, half the floats each (biases and log_std stay in `params`)
      const float* Q = (const float*)io.params_bf16 + (size_t)net * (pol_net_floats<A>(io.obs_dim) - A::H1 - A::H2 - A::H3 - POL_OUT) / 2;
      nw.W1 = Q;
      nw.W2 = nw.W1 + (size_t)A::H1 * K0p / 2;
      nw.W3 = nw.W2 + (size_t)A::H2 * A::H1 / 2;
      nw.W4 = nw.W3 + (size_t)A::H3 * A::H2 / 2;
    }
  }
};

// grid (ceil(ne / 16), 2): blockIdx.y = 0 the policy net, 1 the value net.  BF (bf16 weights) is instantiated for the reference's triple only
template <class A, bool BF>
__global__ void __launch_bounds__(POL_THREADS, (POL_WAVES >= 8 ? 4 : 2)) k6_policy_act(PolActArgs<auv_policy_io_t> pa) {   // (two workgroups per CU)
  pol_act_body<A, BF, false>(pa, PolicyTile<BF>(pa.io));
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
static auto k6_f32 = [](auto a) { return k6_policy_act<decltype(a), false>; };
static auto k6_bf16 = [](auto) { return k6_policy_act<PolArchRef, true>; };

hipError_t auv_policy_prepare(int h1, int h2, int h3, int obs_dim) {
  const size_t b = pol_lds_bytes_h(h1, h2, h3, obs_dim);
  const hipError_t e = pol_act_prepare(h1, h2, h3, b, k6_f32);
  if (e != hipSuccess || !pol_arch_is_ref(h1, h2, h3)) return e;
  return pol_act_prepare(h1, h2, h3, b, k6_bf16);
}

void auv_launch_policy(int h1, int h2, int h3, const auv_policy_io_t& io, int e0, int ne, hipStream_t st, long long t_host, long long gstep_host) {
  const PolActArgs<auv_policy_io_t> pa = {io, e0, ne, t_host, gstep_host};
  const size_t lds = pol_lds_bytes_h(h1, h2, h3, io.obs_dim);
  if (io.params_bf16 && pol_arch_is_ref(h1, h2, h3)) pol_act_launch(h1, h2, h3, pa, lds, st, k6_bf16);
  else pol_act_launch(h1, h2, h3, pa, lds, st, k6_f32);
}
