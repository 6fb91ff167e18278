// The bodies of the three population kernels -- the launch that evaluates a policy per group of rows, the perturbation that makes a
// population on the device and the ES estimate that folds it back -- as templates over the hidden widths A = PolArch<H1, H2, H3>, and
// the host launches that go with them.  k11_population.hip instantiates them for the reference's [256, 128, 64] (scripts/run.py:332-357),
// k14_population_arch.hip for every other triple of POL_ARCH_LIST (auv_policy_mfma.h).
//
// pop_act_pass runs the forward pass k9_policy_eval runs for the policy net (auv_policy_forward.h: pol_trunk<false, A> and the shared
// action map; the same workgroup of 16 rows of ONE net and eight waves) with one difference: the weight block is picked per TILE,
// members + (row / G) * stride, instead of once per launch.  G is a multiple of 16, so a tile never straddles two members, and every
// workgroup streams its net's weights on its own anyway.  For the same row and the same block the mean has the bits auv_policy_eval
// gives at the same widths (tests/test_gpu_population.py, tests/test_gpu_population_arch.py).
//
// The noise of pop_perturb_pass / pop_update_pass is a function of (seed, generation, pair, element) alone and has no logf / cosf in
// it: the sum of the four 16-bit fields of a splitmix64 hash, centred and scaled to unit variance (an Irwin-Hall sum of four uniforms:
// symmetric, |eps| <= 3.464).  gym_auv_amd/population.py mirrors it in NumPy bit for bit; the update regenerates it, nothing is stored.
// The widths enter those two only through pop_live<A>: which elements of a packed block are parameters of the net.
#ifndef AUV_POPULATION_PASS_H
#define AUV_POPULATION_PASS_H
#include "auv_noise.h"
#include "auv_policy_forward.h"

namespace {

struct PopArgs {
  auv_population_io_t io;
  int32_t vec2;                      // every source row starts 8-byte aligned and holds an even number of floats (host-proven)
};

// rows of a strided matrix -> the tile.  V = float2: ldx and obs_dim even and the base 8-byte aligned, so no pair straddles two rows
// or an 8-byte boundary
template <class V>
__device__ __forceinline__ void pop_fill_rows(float* X, const int ldx, const auv_population_io_t& io, const int r0, const int rows, const int tid) {
  constexpr int W = sizeof(V) / sizeof(float);
  const int K0 = io.obs_dim;
  const float* src = io.X + (size_t)r0 * (size_t)io.ldx;
  const size_t lds = (size_t)io.ldx;
  for (int i = W * tid; i < rows * K0; i += W * POL_THREADS) {
    const int row = i / K0, c = i - row * K0;
    *(V*)(X + row * ldx + c) = *(const V*)(src + row * lds + c);
  }
}

// grid ceil(M / 16), POL_THREADS threads, pol_lds_bytes<A>(obs_dim) of dynamic LDS where io.act
template <class A>
__device__ __forceinline__ void pop_act_pass(const PopArgs& pa) {
  extern __shared__ __align__(16) unsigned char smem[];
  const auv_population_io_t& io = pa.io;
  const int tid = threadIdx.x, wave = tid / AUV_WAVE, lane = tid % AUV_WAVE;
  const int M = io.M;
  const int r0 = blockIdx.x * POL_ROWS;                          // first row of the tile (M <= 2^31 - 1: no overflow)
  // ---- the step the tile's environments have just completed: reward and done into the running sums ----
  // (requested here, stored at the end, as k6_policy_act does with its transition: load - store - load - store at the head of the
  // kernel are two trips to memory in front of everything wave 0 does)
  const bool accum = io.accumulate != 0 && tid < POL_ROWS && r0 + tid < M;
  float acc_r = 0.0f, acc_f = 0.0f;
  uint8_t acc_d = 0;
  int32_t acc_e = 0;
  if (accum) acc_r = io.reward_in[r0 + tid], acc_d = io.done_in[r0 + tid], acc_f = io.fit[r0 + tid], acc_e = io.ends[r0 + tid];
  if (io.act) {                                                  // (uniform; 0: the flush launch behind a window's last step)
    const int K0 = io.obs_dim, K0p = pol_pad16(K0);
    float* X = (float*)smem;
    const int ldx = pol_ldx(K0);
    const PolNet nw = pol_net_ptrs<A>(io.members + (size_t)(r0 / io.G) * (size_t)io.stride, K0);   // this tile's member
    PolW<A::H1 / 16, false> w1;
    pol_prefetch(w1, nw.W1, nw.b1, K0p, wave, lane);               // (in flight while the rows are fetched)
    // ---- the tile's rows -> LDS; padding columns and the rows past M stay zero ----
    const int rows = (M - r0 < POL_ROWS) ? M - r0 : POL_ROWS;
    pol_zero_tile(X, ldx, tid);
    __syncthreads();
    if (pa.vec2) pop_fill_rows<float2>(X, ldx, io, r0, rows, tid);
    else pop_fill_rows<float>(X, ldx, io, r0, rows, tid);
    f32x4 o[1][POL_MT];
    pol_trunk<false, A>(X, K0, nw, w1, nullptr, wave, lane, o);   // (no log-std: nothing is sampled)
    if (wave != 0) return;
    const int n = lane & 15, g = lane >> 4;
    const PolActMap map = pol_act_map(io, pol_comp(lane));
#pragma unroll
    for (int u = 0; u < POL_MT; u++)
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int rr = 16 * u + 4 * g + i;                       // row inside the tile
        const int row = r0 + rr;
        if (n < 2 && rr < rows) {
          const float mu = o[0][u][i];
          if (io.mu) io.mu[2 * (size_t)row + n] = mu;
          if (io.action) io.action[(size_t)row * (size_t)io.action_ld + n] = map(mu);
        }
      }
  }
  if (accum) {
    io.fit[r0 + tid] = __fadd_rn(acc_f, acc_r);
    io.ends[r0 + tid] = acc_e + (acc_d ? 1 : 0);
  }
}

// (the counter-based noise, pop_key / pop_eps / pop_eps_scale: auv_noise.h, shared with the planner's sampler)

// Is element i of a packed net (W1 b1 W2 b2 W3 b3 W4 b4, include/auv_hip.h: auv_policy_io) a parameter of the net -- or padding:
// a column of W1 beyond obs_dim, a row 2..15 of W4, an entry 2..15 of b4?  The fragment-order formula inverted: in a matrix,
// element [n][k] sits at ((((n / 16) * (K / 32) + k / 32) * 2 + (k % 8) / 4) * 64 + ((k % 32) / 8) * 16 + n % 16) * 4 + k % 4.
// The widths set the segment lengths only (compile-time: the offsets fold to constants); the W1 rule works on 512-float (n-tile,
// k-step) blocks and the W4 rule on the row n % 16, whatever the widths.
template <class A>
__device__ __forceinline__ bool pop_live(unsigned int i, int obs_dim) {
  const unsigned int K0p = (unsigned int)pol_pad16(obs_dim), nJ = K0p / 32;
  const unsigned int w1 = A::H1 * K0p;
  if (i < w1) {
    const unsigned int k = 32 * ((i >> 9) % nJ) + 8 * ((i >> 6) & 3) + 4 * ((i >> 8) & 1) + (i & 3);
    return k < (unsigned int)obs_dim;
  }
  i -= w1;
  const unsigned int full = A::H1 + A::H2 * A::H1 + A::H2 + A::H3 * A::H2 + A::H3;   // b1 W2 b2 W3 b3: no padding
  if (i < full) return true;
  i -= full;
  if (i < POL_OUT * A::H3) return ((i >> 2) & 15) < 2;           // W4: one n-tile, the row is n % 16
  i -= POL_OUT * A::H3;
  return i < 2;                                                  // b4 (and nothing behind it)
}

// one thread per (member, four consecutive elements): a 16-byte store.  grid (ceil(stride / 4 / 256), P), 256 threads
template <class A>
__device__ __forceinline__ void pop_perturb_pass(const float* __restrict__ theta, float* __restrict__ members, const long long stride,
                                                 const int P, const int obs_dim, const unsigned int nf, const float sigma,
                                                 const unsigned long long seed, const unsigned long long generation, const float c) {
  const unsigned int i0 = 4 * (blockIdx.x * 256 + threadIdx.x);
  const int p = blockIdx.y;
  if ((long long)i0 >= stride) return;
  const unsigned long long key = pop_key(seed, generation);
  float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (i0 < nf) {                                                 // (nf is a multiple of 4: the four are inside or outside together)
    const float4 b = *(const float4*)(theta + i0);
    v[0] = b.x, v[1] = b.y, v[2] = b.z, v[3] = b.w;
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (pop_live<A>(i0 + j, obs_dim)) {
        const float d = __fmul_rn(sigma, pop_eps(key, (unsigned int)(p >> 1), i0 + j, c));
        v[j] = __fadd_rn(v[j], (p & 1) ? -d : d);
      }
  }
  *(float4*)(members + (size_t)p * (size_t)stride + i0) = make_float4(v[0], v[1], v[2], v[3]);
}

// one thread per element.  grid ceil(nf / 256), 256 threads
template <class A>
__device__ __forceinline__ void pop_update_pass(float* __restrict__ theta, const float* __restrict__ w, float* __restrict__ grad,
                                                const int P, const int obs_dim, const unsigned int nf, const float scale, const float lr,
                                                const unsigned long long seed, const unsigned long long generation, const float c) {
  const unsigned int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nf) return;
  if (!pop_live<A>(i, obs_dim)) {
    grad[i] = 0.0f;
    return;
  }
  const unsigned long long key = pop_key(seed, generation);
  float acc = 0.0f;
  for (int pair = 0; pair < P / 2; pair++) {
    const float d = __fsub_rn(w[2 * pair], w[2 * pair + 1]);
    acc = __fadd_rn(acc, __fmul_rn(d, pop_eps(key, (unsigned int)pair, i, c)));
  }
  const float g = __fmul_rn(acc, scale);
  grad[i] = g;
  if (lr != 0.0f) theta[i] = __fadd_rn(theta[i], __fmul_rn(lr, g));
}

// ---- the host side of a triple: K names its three kernels (K::act, K::perturb, K::update) ----
template <class A>
inline size_t pop_member_floats(int obs_dim) { return (pol_net_floats<A>(obs_dim) + 3) & ~(size_t)3; }

template <class A, class K>
inline hipError_t pop_prepare(int obs_dim) {
  const size_t b = pol_lds_bytes<A>(obs_dim);
  if (b <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute((const void*)K::act, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
}

template <class A, class K>
inline void pop_launch_act(const auv_population_io_t& io, hipStream_t st) {
  PopArgs pa;
  pa.io = io;
  pa.vec2 = ((io.ldx & 1) == 0 && (io.obs_dim & 1) == 0 && ((uintptr_t)io.X & 7) == 0) ? 1 : 0;
  const dim3 grid((unsigned)(((long long)io.M + POL_ROWS - 1) / POL_ROWS)), block(POL_THREADS);
  hipLaunchKernelGGL(K::act, grid, block, io.act ? pol_lds_bytes<A>(io.obs_dim) : 0, st, pa);
}

template <class A, class K>
inline void pop_launch_perturb(const float* theta, float* members, long long stride, int P, int obs_dim, float sigma, unsigned long long seed,
                               unsigned long long generation, hipStream_t st) {
  const unsigned int nf = (unsigned int)pop_member_floats<A>(obs_dim);
  const dim3 grid((unsigned)((stride / 4 + 255) / 256), (unsigned)P), block(256);
  hipLaunchKernelGGL(K::perturb, grid, block, 0, st, theta, members, stride, P, obs_dim, nf, sigma, seed, generation, pop_eps_scale());
}

template <class A, class K>
inline void pop_launch_update(float* theta, const float* w, float* grad, int P, int obs_dim, float sigma, float lr, unsigned long long seed,
                              unsigned long long generation, hipStream_t st) {
  const unsigned int nf = (unsigned int)pop_member_floats<A>(obs_dim);
  const float scale = (float)(1.0 / ((double)P * (double)sigma));
  hipLaunchKernelGGL(K::update, dim3((nf + 255) / 256), dim3(256), 0, st, theta, w, grad, P, obs_dim, nf, scale, lr, seed, generation,
                     pop_eps_scale());
}

}  // namespace

// the reference triple's launches (k11_population.hip), which k14_population_arch.hip dispatches to
hipError_t auv_k11_population_prepare(int obs_dim);
void auv_k11_population_act(const auv_population_io_t& io, hipStream_t st);
void auv_k11_population_perturb(const float* theta, float* members, long long stride, int P, int obs_dim, float sigma, unsigned long long seed,
                                unsigned long long generation, hipStream_t st);
void auv_k11_population_update(float* theta, const float* w, float* grad, int P, int obs_dim, float sigma, float lr, unsigned long long seed,
                               unsigned long long generation, hipStream_t st);
#endif /* AUV_POPULATION_PASS_H */
