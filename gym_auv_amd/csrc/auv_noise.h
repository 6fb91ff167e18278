// auv_noise.h — the counter-based noise every kernel file shares: the splitmix64 finaliser (pol_mix) and the draw of the population
// kernels and the planner's sampler, eps(seed, generation, pair, element).  Defined here alone; auv_policy_forward.h (pol_gauss),
// auv_population_pass.h (perturbation, ES estimate) and k15_plan.hip (auv_plan_sample) include it.
//
// The draw has no logf / cosf in it: the sum of the four 16-bit fields of a splitmix64 hash, centred and scaled to unit variance (an
// Irwin-Hall sum of four uniforms: symmetric, |eps| <= 3.464).  gym_auv_amd/population.py (es_noise) mirrors it in NumPy bit for bit.
#ifndef AUV_NOISE_H
#define AUV_NOISE_H
#include <hip/hip_runtime.h>
#include <math.h>

namespace {

// splitmix64 finaliser: 64 well-mixed bits
__device__ __forceinline__ unsigned long long pol_mix(unsigned long long z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// ---- (seed, generation, pair, element) -> eps, unit variance, bit-reproducible on the host ----
// the part of the key all elements of a launch share
__device__ __forceinline__ unsigned long long pop_key(unsigned long long seed, unsigned long long generation) {
  return pol_mix(seed ^ (generation * 0xd1342543de82ef95ull));
}
// c = float32(1 / sqrt(4 (65536^2 - 1) / 12)), formed on the host (pop_eps_scale)
__device__ __forceinline__ float pop_eps(unsigned long long key, unsigned int pair, unsigned int i, float c) {
  const unsigned long long h = pol_mix(pol_mix(key ^ (unsigned long long)pair) ^ (unsigned long long)i);
  const int S = (int)(h & 0xffffu) + (int)((h >> 16) & 0xffffu) + (int)((h >> 32) & 0xffffu) + (int)(h >> 48);
  return __fmul_rn((float)(S - 131070), c);                     // |S - 131070| < 2^24: the conversion is exact
}

inline float pop_eps_scale() { return (float)(1.0 / sqrt(4.0 * (65536.0 * 65536.0 - 1.0) / 12.0)); }

}  // namespace
#endif /* AUV_NOISE_H */
