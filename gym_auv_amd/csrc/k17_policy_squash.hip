// K17 -- the tanh-squashed Gaussian policy in the loop and outside it: k6_policy_act's exact-f32 launch and k9_policy_eval's launch
// with the second action map of auv_policy_forward.h, PolSquashMap -- the environment receives act_mid + act_half * tanh(u) of the
// sample u = mu + sigma eps (of the mean, in the evaluation), a bounded action whose entropy the update's squash head
// (auv_ppo_pass.h, ppo_head on auv_ppo_squash_batch_t) can see.  What stable-baselines3 calls squash_output; docs/HISTORY.md has the
// account.
//
// The stored action stays u: A, LP (the Gaussian log-density of u), V, R, Dn, mu_out, eps_out and the counter hand-overs are the
// plain launch's, bit for bit (the same frame: pol_act_begin / pol_act_sample / pol_act_end; the same trunk); only actions_out
// differs.  clip_lo / clip_hi are not read.  No bf16 variant, no stacked, normalising or population variant.
#include "auv_launch.h"
#include "auv_policy_forward.h"

namespace {

struct SquashActArgs {
  auv_policy_io_t io;
  int32_t e0, ne;
  long long t_host, gstep_host;      // as k6's PolicyArgs: >= 0 the host names the rollout position and the generator's step, -1 io.ctr
};

// grid (ceil(ne / 16), 2): blockIdx.y = 0 the policy net, 1 the value net -- k6_policy_act<A, false> with pol_act_sample<true>
template <class A>
__global__ void __launch_bounds__(POL_THREADS, (POL_WAVES >= 8 ? 4 : 2)) k17_squash_act(SquashActArgs pa) {
  extern __shared__ __align__(16) unsigned char smem[];
  const auv_policy_io_t& io = pa.io;
  const int tid = threadIdx.x, wave = tid / AUV_WAVE, lane = tid % AUV_WAVE;
  const int net = blockIdx.y;
  const int K0 = io.obs_dim, K0p = pol_pad16(K0);
  float* X = (float*)smem;
  const PolAct p = pol_act_begin(io, pa.e0, pa.ne, pa.t_host, pa.gstep_host);
  if (p.act) {
    const PolNet nw = pol_net_ptrs<A>(io.params + (size_t)net * pol_net_floats<A>(K0), K0);
    PolW<A::H1 / 16, false> w1;
    pol_prefetch(w1, nw.W1, nw.b1, K0p, wave, lane);                 // (in flight while the observation tile is fetched)
    const int rows = (p.cnt - p.r0 < POL_ROWS) ? p.cnt - p.r0 : POL_ROWS;
    pol_zero_tile(X, pol_ldx(K0), tid);
    __syncthreads();
    pol_act_fill_obs(X, io, p, pol_act_obs_out(io, p, K0), rows);
    f32x4 o[1][POL_MT];
    const float ls = pol_trunk<false, A>(X, K0, nw, w1, (wave == 0 && net == 0) ? io.params + 2 * pol_net_floats<A>(K0) : nullptr, wave, lane, o);
    if (wave == 0) pol_act_sample<true>(io, p, o, ls, lane);
  }
  pol_act_end(io, p);
}

// grid (ceil(M / 16), nets launched): k9_policy_eval with the squashed deterministic action
template <class A>
__global__ void __launch_bounds__(POL_THREADS, (POL_WAVES >= 8 ? 4 : 2)) k17_squash_eval(EvalArgs ea) {
  policy_eval_body<A, true>(ea);
}

}  // namespace

// ---- host side: (h1, h2, h3) a listed hidden-width triple (the caller has checked); LDS as the plain launches' ----
hipError_t auv_policy_squash_prepare(int h1, int h2, int h3, int obs_dim, bool eval) {
  const size_t b = pol_lds_bytes_h(h1, h2, h3, obs_dim);
  if (b <= 64 * 1024) return hipSuccess;
  hipError_t e = hipErrorInvalidValue;
  pol_arch_visit(h1, h2, h3, [&](auto a) {
    const void* k = eval ? (const void*)k17_squash_eval<decltype(a)> : (const void*)k17_squash_act<decltype(a)>;
    e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
  });
  return e;
}

void auv_launch_policy_squash(int h1, int h2, int h3, const auv_policy_io_t& io, int e0, int ne, hipStream_t st, long long t_host,
                              long long gstep_host) {
  SquashActArgs pa;
  pa.io = io, pa.e0 = e0, pa.ne = ne;
  pa.t_host = t_host, pa.gstep_host = gstep_host;
  const dim3 grid((ne + POL_ROWS - 1) / POL_ROWS, 2), block(POL_THREADS);
  const size_t lds = pol_lds_bytes_h(h1, h2, h3, io.obs_dim);
  pol_arch_visit(h1, h2, h3, [&](auto a) { hipLaunchKernelGGL((k17_squash_act<decltype(a)>), grid, block, lds, st, pa); });
}

// want_pi / want_v: which nets have an output asked for (at least one; the caller has checked)
void auv_launch_policy_eval_squash(int h1, int h2, int h3, const auv_policy_eval_t& ev, bool want_pi, bool want_v, hipStream_t st) {
  EvalArgs ea;
  ea.ev = ev;
  ea.net0 = want_pi ? 0 : 1;
  ea.vec2 = ((ev.ldx & 1) == 0 && (ev.obs_dim & 1) == 0 && ((uintptr_t)ev.X & 7) == 0) ? 1 : 0;
  const dim3 grid((unsigned)(((long long)ev.M + POL_ROWS - 1) / POL_ROWS), (want_pi ? 1 : 0) + (want_v ? 1 : 0)), block(POL_THREADS);
  const size_t lds = pol_lds_bytes_h(h1, h2, h3, ev.obs_dim);
  pol_arch_visit(h1, h2, h3, [&](auto a) { hipLaunchKernelGGL((k17_squash_eval<decltype(a)>), grid, block, lds, st, ea); });
}
