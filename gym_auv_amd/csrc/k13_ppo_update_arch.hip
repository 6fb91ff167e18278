// K13 -- the PPO / clone update (k8_ppo_update.hip, whose head describes the launches) at the other hidden widths of POL_ARCH_LIST
// (auv_policy_mfma.h), and the dispatch of auv_ppo_* on an updater's widths.
//
// Reference: scripts/run.py:332-357 trains net_arch [256, 128, 64]; that triple runs the kernels of k8_ppo_update.hip, here are the
// instantiations of the same bodies (auv_ppo_pass.h) for every other listed triple.  They live in a file of their own so that
// k8_ppo_update.hip keeps exactly one row-pass kernel per head; their names share no substring with those.
#include <type_traits>

#include "auv_ppo_pass.h"

namespace {

// grid (ceil(B / 16), 2): blockIdx.y = 0 the policy net, 1 the value net
template <class A>
__global__ void __launch_bounds__(POL_THREADS, 4) k13_ppo_rows(RowArgs<auv_ppo_batch_t> ra) { ppo_row_pass<A>(ra.d, ra.b, blockIdx.y, blockIdx.x); }

template <class A>
__global__ void __launch_bounds__(POL_THREADS, 4) k13_ppo_clone(RowArgs<auv_ppo_clone_batch_t> ra) { ppo_row_pass<A>(ra.d, ra.b, blockIdx.y, blockIdx.x); }

template <class A>
__global__ void __launch_bounds__(POL_THREADS, 4) k13_ppo_squash(RowArgs<auv_ppo_squash_batch_t> ra) { ppo_row_pass<A>(ra.d, ra.b, blockIdx.y, blockIdx.x); }

template <class A>
struct K13 {
  static constexpr auto rows = k13_ppo_rows<A>;
  static constexpr auto clone = k13_ppo_clone<A>;
  static constexpr auto squash = k13_ppo_squash<A>;
};

// ref() for the reference's triple, other(PolArch<...>{}) for any other listed one: only those instantiate kernels here
template <class R, class F>
inline void ppo_dispatch(const auv_policy_arch_t& a, R&& ref, F&& other) {
  pol_arch_visit(a.h1, a.h2, a.h3, [&](auto t) {
    if constexpr (std::is_same<decltype(t), PolArchRef>::value) ref();
    else other(t);
  });
}

}  // namespace

size_t auv_ppo_param_floats_impl(int obs_dim, const auv_policy_arch_t& a) { return ppo_params_h(a.h1, a.h2, a.h3, obs_dim); }
size_t auv_ppo_fwd_floats(int obs_dim, const auv_policy_arch_t& a) { return 2 * pol_net_floats_h(a.h1, a.h2, a.h3, obs_dim) + 4; }
size_t auv_ppo_tr_floats(const auv_policy_arch_t& a) { return 2 * ppo_tr_floats_h(a.h1, a.h2, a.h3); }
size_t auv_ppo_lds_bytes(int obs_dim, const auv_policy_arch_t& a) { return sizeof(float) * ppo_lds_floats_h(a.h1, a.h2, a.h3, obs_dim); }

hipError_t auv_ppo_prepare(int obs_dim, const auv_policy_arch_t& a, int head) {
  hipError_t e = hipErrorInvalidValue;                               // (an unlisted triple: refused before, in auv_ppo_create_arch)
  ppo_dispatch(a, [&] { e = auv_k8_ppo_prepare(obs_dim, head); },
               [&](auto t) { e = ppo_prepare<decltype(t), K13<decltype(t)>>(obs_dim, head); });
  return e;
}

void auv_launch_ppo_load(const AuvPpoDev& d, const auv_policy_arch_t& a, const float* theta, hipStream_t st) {
  ppo_dispatch(a, [&] { auv_k8_ppo_load(d, theta, st); }, [&](auto t) { ppo_launch_load<decltype(t)>(d, theta, st); });
}

void auv_launch_ppo_grad(const AuvPpoDev& d, const auv_policy_arch_t& a, const auv_ppo_batch_t& b, float* grad, float* stats, hipStream_t st) {
  ppo_dispatch(a, [&] { auv_k8_ppo_grad(d, b, grad, stats, st); },
               [&](auto t) { ppo_launch_grad<decltype(t), K13<decltype(t)>>(d, b, grad, stats, st); });
}

void auv_launch_ppo_grad_clone(const AuvPpoDev& d, const auv_policy_arch_t& a, const auv_ppo_clone_batch_t& b, float* grad, float* stats,
                               hipStream_t st) {
  ppo_dispatch(a, [&] { auv_k8_ppo_grad_clone(d, b, grad, stats, st); },
               [&](auto t) { ppo_launch_grad_clone<decltype(t), K13<decltype(t)>>(d, b, grad, stats, st); });
}

void auv_launch_ppo_grad_squash(const AuvPpoDev& d, const auv_policy_arch_t& a, const auv_ppo_squash_batch_t& b, float* grad, float* stats,
                                hipStream_t st) {
  ppo_dispatch(a, [&] { auv_k8_ppo_grad_squash(d, b, grad, stats, st); },
               [&](auto t) { ppo_launch_grad_squash<decltype(t), K13<decltype(t)>>(d, b, grad, stats, st); });
}

void auv_launch_ppo_adam(const AuvPpoDev& d, const auv_policy_arch_t& a, float* theta, float* m, float* v, const float* grad,
                         const AuvPpoAdamDev& h, float* norms_out, hipStream_t st) {
  ppo_dispatch(a, [&] { auv_k8_ppo_adam(d, theta, m, v, grad, h, norms_out, st); },
               [&](auto t) { ppo_launch_adam<decltype(t)>(d, theta, m, v, grad, h, norms_out, st); });
}
