// K11 -- a population of policies in one launch (auv_population_act) and the two kernels that make a population on the device and
// fold it back (auv_population_perturb, auv_population_update): evolution strategies, ARS on the reference's own [256, 128, 64]
// actor (scripts/run.py:332-357), "evaluate these 256 checkpoints side by side".
//
// The bodies live in auv_population_pass.h (whose head describes them), templates over the hidden widths; here are exactly the three
// kernels of the reference's triple, under the names they have always had.  The other triples of POL_ARCH_LIST have theirs in
// k14_population_arch.hip, which also holds the dispatch of auv_population_* on a launch's widths and calls the auv_k11_* below for
// the reference's.
#include "auv_population_pass.h"

namespace {

// grid ceil(M / 16)
__global__ void __launch_bounds__(POL_THREADS, (POL_WAVES >= 8 ? 4 : 2)) k11_population_act(PopArgs pa) {   // (two workgroups per CU, as k6)
  pop_act_pass<PolArchRef>(pa);
}

// one thread per (member, four consecutive elements): a 16-byte store
__global__ void __launch_bounds__(256) k11_perturb(const float* __restrict__ theta, float* __restrict__ members, const long long stride,
                                                   const int P, const int obs_dim, const unsigned int nf, const float sigma,
                                                   const unsigned long long seed, const unsigned long long generation, const float c) {
  pop_perturb_pass<PolArchRef>(theta, members, stride, P, obs_dim, nf, sigma, seed, generation, c);
}

// one thread per element
__global__ void __launch_bounds__(256) k11_es_update(float* __restrict__ theta, const float* __restrict__ w, float* __restrict__ grad,
                                                     const int P, const int obs_dim, const unsigned int nf, const float scale, const float lr,
                                                     const unsigned long long seed, const unsigned long long generation, const float c) {
  pop_update_pass<PolArchRef>(theta, w, grad, P, obs_dim, nf, scale, lr, seed, generation, c);
}

struct K11 {
  static constexpr auto act = k11_population_act;
  static constexpr auto perturb = k11_perturb;
  static constexpr auto update = k11_es_update;
};

}  // namespace

hipError_t auv_k11_population_prepare(int obs_dim) { return pop_prepare<PolArchRef, K11>(obs_dim); }

void auv_k11_population_act(const auv_population_io_t& io, hipStream_t st) { pop_launch_act<PolArchRef, K11>(io, st); }

void auv_k11_population_perturb(const float* theta, float* members, long long stride, int P, int obs_dim, float sigma, unsigned long long seed,
                                unsigned long long generation, hipStream_t st) {
  pop_launch_perturb<PolArchRef, K11>(theta, members, stride, P, obs_dim, sigma, seed, generation, st);
}

void auv_k11_population_update(float* theta, const float* w, float* grad, int P, int obs_dim, float sigma, float lr, unsigned long long seed,
                               unsigned long long generation, hipStream_t st) {
  pop_launch_update<PolArchRef, K11>(theta, w, grad, P, obs_dim, sigma, lr, seed, generation, st);
}
