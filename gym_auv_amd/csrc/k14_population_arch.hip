// K14 -- the population launches (k11_population.hip, auv_population_pass.h) at the other hidden widths of POL_ARCH_LIST
// (auv_policy_mfma.h), and the dispatch of auv_population_* on a launch's widths.
//
// Reference: scripts/run.py:332-357 uses net_arch [256, 128, 64]; that triple runs the three kernels of k11_population.hip, here are
// the instantiations of the same bodies for every other listed triple -- three kernels each: the perturbation and the ES estimate
// are templated too, so that pop_live's segment offsets stay compile-time constants as they are for the reference's widths.  They
// live in a file of their own so that k11_population.hip keeps exactly its three kernels; their names share no substring with those.
#include <type_traits>

#include "auv_launch.h"
#include "auv_population_pass.h"

namespace {

// grid ceil(M / 16)
template <class A>
__global__ void __launch_bounds__(POL_THREADS, (POL_WAVES >= 8 ? 4 : 2)) k14_pop_act(PopArgs pa) { pop_act_pass<A>(pa); }

template <class A>
__global__ void __launch_bounds__(256) k14_pop_perturb(const float* __restrict__ theta, float* __restrict__ members, const long long stride,
                                                       const int P, const int obs_dim, const unsigned int nf, const float sigma,
                                                       const unsigned long long seed, const unsigned long long generation, const float c) {
  pop_perturb_pass<A>(theta, members, stride, P, obs_dim, nf, sigma, seed, generation, c);
}

template <class A>
__global__ void __launch_bounds__(256) k14_pop_update(float* __restrict__ theta, const float* __restrict__ w, float* __restrict__ grad,
                                                      const int P, const int obs_dim, const unsigned int nf, const float scale, const float lr,
                                                      const unsigned long long seed, const unsigned long long generation, const float c) {
  pop_update_pass<A>(theta, w, grad, P, obs_dim, nf, scale, lr, seed, generation, c);
}

template <class A>
struct K14 {
  static constexpr auto act = k14_pop_act<A>;
  static constexpr auto perturb = k14_pop_perturb<A>;
  static constexpr auto update = k14_pop_update<A>;
};

// ref() for the reference's triple, other(PolArch<...>{}) for any other listed one: only those instantiate kernels here
template <class R, class F>
inline void pop_dispatch(const auv_policy_arch_t& a, R&& ref, F&& other) {
  pol_arch_visit(a.h1, a.h2, a.h3, [&](auto t) {
    if constexpr (std::is_same<decltype(t), PolArchRef>::value) ref();
    else other(t);
  });
}

}  // namespace

// 0 for an unlisted triple
size_t auv_population_member_floats_impl(const auv_policy_arch_t& a, int obs_dim) {
  size_t n = 0;
  pol_arch_visit(a.h1, a.h2, a.h3, [&](auto t) { n = pop_member_floats<decltype(t)>(obs_dim); });
  return n;
}

hipError_t auv_population_prepare(const auv_policy_arch_t& a, int obs_dim) {
  hipError_t e = hipErrorInvalidValue;                               // (an unlisted triple: refused before, by the entries of auv_capi_learn.hip)
  pop_dispatch(a, [&] { e = auv_k11_population_prepare(obs_dim); }, [&](auto t) { e = pop_prepare<decltype(t), K14<decltype(t)>>(obs_dim); });
  return e;
}

void auv_launch_population_act(const auv_policy_arch_t& a, const auv_population_io_t& io, hipStream_t st) {
  pop_dispatch(a, [&] { auv_k11_population_act(io, st); }, [&](auto t) { pop_launch_act<decltype(t), K14<decltype(t)>>(io, st); });
}

void auv_launch_population_perturb(const auv_policy_arch_t& a, const float* theta, float* members, long long stride, int P, int obs_dim,
                                   float sigma, unsigned long long seed, unsigned long long generation, hipStream_t st) {
  pop_dispatch(a, [&] { auv_k11_population_perturb(theta, members, stride, P, obs_dim, sigma, seed, generation, st); },
               [&](auto t) { pop_launch_perturb<decltype(t), K14<decltype(t)>>(theta, members, stride, P, obs_dim, sigma, seed, generation, st); });
}

void auv_launch_population_update(const auv_policy_arch_t& a, float* theta, const float* w, float* grad, int P, int obs_dim, float sigma,
                                  float lr, unsigned long long seed, unsigned long long generation, hipStream_t st) {
  pop_dispatch(a, [&] { auv_k11_population_update(theta, w, grad, P, obs_dim, sigma, lr, seed, generation, st); },
               [&](auto t) { pop_launch_update<decltype(t), K14<decltype(t)>>(theta, w, grad, P, obs_dim, sigma, lr, seed, generation, st); });
}
