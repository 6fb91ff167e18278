// K17 -- the tanh-squashed Gaussian policy in the loop and outside it: k6_policy_act's exact-f32 launch and k9_policy_eval's launch
// with the second action map of auv_policy_forward.h, PolSquashMap -- the environment receives act_mid + act_half * tanh(u) of the
// sample u = mu + sigma eps (of the mean, in the evaluation), a bounded action whose entropy the update's squash head
// (auv_ppo_pass.h, ppo_head on auv_ppo_squash_batch_t) can see.  What stable-baselines3 calls squash_output; docs/HISTORY.md has the
// account.
//
// The stored action stays u: A, LP (the Gaussian log-density of u), V, R, Dn, mu_out, eps_out and the counter hand-overs are the
// plain launch's, bit for bit (the same body, pol_act_body with the plain tile, and SQUASH = true: auv_policy_forward.h); only
// actions_out differs.  clip_lo / clip_hi are not read.  No bf16 variant, no stacked, normalising or population variant.
#include "auv_launch.h"
#include "auv_policy_forward.h"

namespace {

// grid (ceil(ne / 16), 2): blockIdx.y = 0 the policy net, 1 the value net -- k6_policy_act<A, false>'s plain tile, SQUASH = true
template <class A>
__global__ void __launch_bounds__(POL_THREADS, (POL_WAVES >= 8 ? 4 : 2)) k17_squash_act(PolActArgs<auv_policy_io_t> pa) {
  pol_act_body<A, false, true>(pa, PolPlainTile(pa.io));
}

// grid (ceil(M / 16), nets launched): k9_policy_eval with the squashed deterministic action
template <class A>
__global__ void __launch_bounds__(POL_THREADS, (POL_WAVES >= 8 ? 4 : 2)) k17_squash_eval(EvalArgs ea) {
  policy_eval_body<A, true>(ea);
}

}  // namespace

// ---- host side: (h1, h2, h3) a listed hidden-width triple (the caller has checked); LDS as the plain launches' ----
hipError_t auv_policy_squash_prepare(int h1, int h2, int h3, int obs_dim, bool eval) {
  return pol_act_prepare(h1, h2, h3, pol_lds_bytes_h(h1, h2, h3, obs_dim), [&](auto a) {
    return eval ? (const void*)k17_squash_eval<decltype(a)> : (const void*)k17_squash_act<decltype(a)>;
  });
}

void auv_launch_policy_squash(int h1, int h2, int h3, const auv_policy_io_t& io, int e0, int ne, hipStream_t st, long long t_host,
                              long long gstep_host) {
  const PolActArgs<auv_policy_io_t> pa = {io, e0, ne, t_host, gstep_host};
  pol_act_launch(h1, h2, h3, pa, pol_lds_bytes_h(h1, h2, h3, io.obs_dim), st, [](auto a) { return k17_squash_act<decltype(a)>; });
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
