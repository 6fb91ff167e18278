// The policy MLP on the matrix cores: tile geometry, the packed-weight layout and the layer routine shared by the forward launches
// (k6, k9, k11, k12 through auv_policy_forward.h, which holds their common forward pass) and the PPO update (k8_ppo_update.hip).
// Reference: scripts/run.py:332-357 (MlpPolicy, net_arch [256, 128, 64], tanh).
#ifndef AUV_POLICY_MFMA_H
#define AUV_POLICY_MFMA_H
#include "auv_device.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#ifndef POL_MT
#define POL_MT 1                   // MFMA M-tiles (of 16 rows) per workgroup.  (2 -- every weight fragment a wave loads then serves two
#endif                             // tiles, half the L2 traffic -- was measured: 51 against 61 M env-steps/s in PPO rollouts: fewer, longer
                                   // workgroups; the launch is not bound by what it pulls out of L2)
#define POL_ROWS (16 * POL_MT)
#ifndef POL_WAVES
#define POL_WAVES 8                 // waves per workgroup: a layer's n-tiles are dealt round-robin to them
#endif
#define POL_THREADS (64 * POL_WAVES)
#define POL_H1 256
#define POL_H2 128
#define POL_H3 64
#define POL_OUT 16                 // the last layer's outputs (2 actions / 1 value) padded to one n-tile
#define POL_LOG_SQRT_2PI 0.9189385332046727f

// The hidden widths of the forward launches (k6, k9, k12) are a compile-time parameter: obs -> H1 -> H2 -> H3 -> out, tanh.  What the
// layer routine and the LDS carve-up below rely on is asserted here: every width a multiple of 64 (the row strides H + 8 stay = 8 mod 64
// floats -- the bank argument below -- and K / 32 stays even where a layer runs with KS = 2), H1 >= H3 (Y3 lives in Y1's place).
template <int H1_, int H2_, int H3_>
struct PolArch {
  static constexpr int H1 = H1_, H2 = H2_, H3 = H3_;
  static_assert(H1_ > 0 && H2_ > 0 && H3_ > 0 && H1_ % 64 == 0 && H2_ % 64 == 0 && H3_ % 64 == 0, "hidden widths: multiples of 64");
  static_assert(H1_ >= H3_, "Y3 re-uses Y1's LDS");
};
typedef PolArch<POL_H1, POL_H2, POL_H3> PolArchRef;   // the reference's net: the default (k8's and k11's own kernels; k13 / k14 hold the other triples')
// THE LIST of the triples the forward launches and the fused update (k8, k13) are instantiated for, the default first: a triple more is one line here.  It is expanded
// once, in pol_arch_any; every host-side dispatch finds its kernel through pol_arch_visit, which also instantiates it.
#define POL_ARCH_LIST(X) \
  X(256, 128, 64)        \
  X(128, 128, 64)        \
  X(128, 64, 64)         \
  X(64, 64, 64)
// f(PolArch<a, b, c>{}) -> bool for the triples of the list in order, up to the first that answers true
template <class F>
__host__ inline bool pol_arch_any(F&& f) {
#define POL_ARCH_TRY(a, b, c) if (f(PolArch<a, b, c>{})) return true;
  POL_ARCH_LIST(POL_ARCH_TRY)
#undef POL_ARCH_TRY
  return false;
}
// f(PolArch<h1, h2, h3>{}) if the triple is listed; false, and f not called, if it is not
template <class F>
__host__ inline bool pol_arch_visit(int h1, int h2, int h3, F&& f) {
  return pol_arch_any([&](auto a) {
    if (h1 != a.H1 || h2 != a.H2 || h3 != a.H3) return false;
    f(a);
    return true;
  });
}
__host__ inline bool pol_arch_is_ref(int h1, int h2, int h3) { return h1 == POL_H1 && h2 == POL_H2 && h3 == POL_H3; }
__host__ inline bool pol_arch_listed(int h1, int h2, int h3) { return pol_arch_visit(h1, h2, h3, [](auto) {}); }

__host__ __device__ inline int pol_pad16(int x) { return (x + 31) & ~31; }   // (the k-step of pol_layer: 32)
// floats of ONE packed net: W1 [H1][K0p] b1 [H1] W2 [H2][H1] b2 [H2] W3 [H3][H2] b3 [H3] W4 [16][H3] b4 [16]
__host__ __device__ inline size_t pol_net_floats_h(int h1, int h2, int h3, int obs_dim) {
  const size_t k0 = (size_t)pol_pad16(obs_dim);
  return h1 * k0 + h1 + (size_t)h2 * h1 + h2 + (size_t)h3 * h2 + h3 + (size_t)POL_OUT * h3 + POL_OUT;
}
template <class A = PolArchRef>
__host__ __device__ inline size_t pol_net_floats(int obs_dim) { return pol_net_floats_h(A::H1, A::H2, A::H3, obs_dim); }

// LDS of a forward workgroup (carved up in auv_policy_forward.h: pol_ldx, pol_tile_y1, pol_trunk): X [ROWS][max(K0p, H2) + 8] |
// Y1 [ROWS][max(H1, H3) + 8]; Y2 [ROWS][H2 + 8] re-uses X's place (dead after layer 1), Y3 [ROWS][H3 + 8] Y1's (dead after layer 2).
// Row strides = 8 mod 64 floats: the 16-byte reads of an A operand -- 16 rows x 4 k-groups -- then touch every bank once.
__host__ __device__ inline size_t pol_lds_x_floats_h(int h2, int obs_dim) {
  const size_t x = (size_t)pol_pad16(obs_dim) + 8, y2 = (size_t)h2 + 8;
  return POL_ROWS * (x > y2 ? x : y2);
}
__host__ __device__ inline size_t pol_lds_y1_floats_h(int h1, int h3) { return (size_t)POL_ROWS * ((h1 > h3 ? h1 : h3) + 8); }
__host__ __device__ inline size_t pol_lds_bytes_h(int h1, int h2, int h3, int obs_dim) {
  return sizeof(float) * (pol_lds_x_floats_h(h2, obs_dim) + pol_lds_y1_floats_h(h1, h3));
}
template <class A = PolArchRef>
__host__ __device__ inline size_t pol_lds_x_floats(int obs_dim) { return pol_lds_x_floats_h(A::H2, obs_dim); }
template <class A = PolArchRef>
__host__ __device__ inline size_t pol_lds_bytes(int obs_dim) { return pol_lds_bytes_h(A::H1, A::H2, A::H3, obs_dim); }

// tanh: 1 - 2 / (exp(2 x) + 1) with the hardware's exp2 and reciprocal (absolute error ~2e-7, far inside the 1e-5 of the
// parity test; saturates correctly: exp -> inf gives 1, exp -> 0 gives -1) instead of the library's ~40-instruction tanhf
__device__ __forceinline__ float pol_tanh(const float x) {
#ifdef POL_LIBM_TANH
  return tanhf(x);
#else
  const float t = __expf(2.0f * x);
  return 1.0f - 2.0f * __frcp_rn(t + 1.0f);
#endif
}

// tanh of a squashed policy's action (PolSquashMap, the squash head of the update): (1 - t) / (1 + t), t = exp(-2 |u|), with the
// library's expf and a rounded division.  Odd bit for bit (|u| goes in, the sign comes back on), exactly +-1 from t < 2^-25 on
// (|u| > 8.7) and for u = +-inf, never NaN for a u that is not; absolute error ~1e-7 (the rounding of t near 1).
__device__ __forceinline__ float pol_squash_tanh(const float u) {
  const float t = expf(-2.0f * fabsf(u));
  return copysignf((1.0f - t) / (1.0f + t), u);
}

// One layer for this wave's n-tiles: Y = tanh(X W^T + b) (or the raw pre-activation rows of the last layer).
//   X  LDS [16][ldx], columns [0, Kp) valid (zero padded); W global, the [N][Kp] matrix of torch's Linear.weight (K padded
//   to a multiple of 32) re-ordered into MFMA fragment order; wave w takes the n-tiles w, w + 4, ... (NT of them).
//   A k-step covers 32 k: lane (row or column l & 15, group g = l >> 4) holds k = 32 J + 8 g + j, j = 0..7, of its row of
//   X (LDS) and of its row of W; MFMA j of the step multiplies element j of every lane, i.e. the k set
//   {32 J + 8 g + j : g} -- A and B permuted alike.  Read from the row-major matrix, neighbouring lanes would sit in
//   different rows (768 bytes apart): 64 separate requests per load instruction, and the kernel is bound by that (36 us for
//   4096 rows, profiles/r04/policy_bench_rowmajor.log); in fragment order an instruction reads one contiguous kilobyte.
//   The weights of the next DEPTH k-steps are in flight while a step's MFMAs issue: a workgroup streams its net's 0.37 MB
//   from L2 with only a wave or two per SIMD to hide the latency (one 16-k step ahead: 60 us for 4096 rows; profiles/r04).
//   KS = 2: the k range alternates between two accumulators per n-tile (a single v_mfma_f32_16x16x4_f32 chain is
//   latency-bound: 40 cycles dependent against 32 of issue).
#ifndef POL_DEPTH
#define POL_DEPTH 2                // (4 was measured: 141 VGPRs, or 24 spilled under the 128 that two workgroups per CU allow: 27 against 23 us)
#endif
// the weight fragments of a wave's n-tiles for the next DEPTH k-steps, in flight or landed.  BF: the weights are stored as
// bf16 (auv_policy_io::params_bf16, optional): a k-step's fragment is then 16 bytes per lane and ONE
// v_mfma_f32_16x16x32_bf16 instead of eight f32 MFMAs (activations are rounded to bf16 on the way into the MFMA,
// accumulation, bias and tanh stay f32) -- NOT the reference's arithmetic: ~1e-2 on the means, behind a flag.
template <int NTILES, bool BF>
struct PolW {
  static constexpr int NT = (NTILES + POL_WAVES - 1) / POL_WAVES;   // n-tiles of this wave: wave, wave + WAVES, ...
  static constexpr int BLK = BF ? 256 : 512;                         // floats (4-byte units) per (n-tile, k-step) block
  float4 q[POL_DEPTH][NT][BF ? 1 : 2];
  const float* row[NT];
  float bias[NT];                    // the epilogue's bias of this lane's column of each n-tile, requested with the weights
};

// Request the first DEPTH k-steps of a layer's weights.  They depend on nothing the kernel computes, so the request for
// layer l + 1 goes out BEFORE layer l's epilogue and the barrier behind it (and layer 1's before the observation tile is
// fetched): a layer then starts on fragments that have landed instead of on a cold trip to L2.
template <int NTILES, bool BF>
__device__ __forceinline__ void pol_prefetch(PolW<NTILES, BF>& w, const float* __restrict__ W, const float* __restrict__ b,
                                             const int Kp, const int wave, const int lane) {
  if (wave >= NTILES) return;
  // (the biases too: asked for in a layer's epilogue they cost it a trip to L2 with nothing else to do; asked for here,
  // ahead of the barrier in front of the layer, they cannot be moved back down to their use)
#pragma unroll
  for (int t = 0; t < PolW<NTILES, BF>::NT; t++) w.bias[t] = b[((wave + POL_WAVES * t) % NTILES) * 16 + (lane & 15)];
  const int nJ = Kp / 32;
  constexpr int BLK = PolW<NTILES, BF>::BLK;
#pragma unroll
  for (int t = 0; t < PolW<NTILES, BF>::NT; t++) w.row[t] = W + (size_t)((wave + POL_WAVES * t) % NTILES) * nJ * BLK + 4 * lane;   // (% : a tile index
                                                                         // past the end re-reads a valid tile, its result is dropped)
#pragma unroll
  for (int d = 0; d < POL_DEPTH; d++) {
    const int Jd = d < nJ ? d : nJ - 1;
#pragma unroll
    for (int t = 0; t < PolW<NTILES, BF>::NT; t++) {
      w.q[d][t][0] = *(const float4*)(w.row[t] + BLK * Jd);
      if (!BF) w.q[d][t][BF ? 0 : 1] = *(const float4*)(w.row[t] + BLK * Jd + 256);
    }
  }
}

__device__ __forceinline__ bf16x8 pol_to_bf16(const float4 lo, const float4 hi) {
  bf16x8 v;
  v[0] = (__bf16)lo.x, v[1] = (__bf16)lo.y, v[2] = (__bf16)lo.z, v[3] = (__bf16)lo.w;
  v[4] = (__bf16)hi.x, v[5] = (__bf16)hi.y, v[6] = (__bf16)hi.z, v[7] = (__bf16)hi.w;
  return v;
}

template <int NTILES, int KS, bool LAST, bool BF>
__device__ __forceinline__ void pol_layer(const float* __restrict__ X, const int ldx, PolW<NTILES, BF>& w,
                                          const float* __restrict__ b, const int Kp, const int wave, const int lane,
                                          float* __restrict__ Y, const int ldy, f32x4 (*out)[POL_MT]) {
  constexpr int NT = PolW<NTILES, BF>::NT;
  constexpr int BLK = PolW<NTILES, BF>::BLK;
  if (wave >= NTILES) return;                                // (more waves than tiles in the narrow layers: nothing to do)
  const int m = lane & 15, g = lane >> 4;
  f32x4 acc[POL_MT][NT][KS];
#pragma unroll
  for (int u = 0; u < POL_MT; u++)
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
      for (int s = 0; s < KS; s++) acc[u][t][s] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
  const float* xrow = X + m * ldx + 8 * g;                   // m-tile u: + 16 u rows
  const int nJ = Kp / 32;                                    // (a multiple of KS for every layer of this architecture)
  for (int J = 0; J < nJ; J += POL_DEPTH) {
#pragma unroll
    for (int d = 0; d < POL_DEPTH; d++) {
      const int Jc = J + d;
      if (Jc < nJ) {                                         // (uniform)
        float4 a[POL_MT][2];
#pragma unroll
        for (int u = 0; u < POL_MT; u++)
          a[u][0] = *(const float4*)(xrow + 16 * u * ldx + 32 * Jc), a[u][1] = *(const float4*)(xrow + 16 * u * ldx + 32 * Jc + 4);
        float4 cur[NT][2];
#pragma unroll
        for (int t = 0; t < NT; t++) cur[t][0] = w.q[d][t][0], cur[t][1] = w.q[d][t][BF ? 0 : 1];
        if (Jc + POL_DEPTH < nJ) {                           // refill this slot for step Jc + DEPTH
#pragma unroll
          for (int t = 0; t < NT; t++) {
            w.q[d][t][0] = *(const float4*)(w.row[t] + BLK * (Jc + POL_DEPTH));
            if (!BF) w.q[d][t][BF ? 0 : 1] = *(const float4*)(w.row[t] + BLK * (Jc + POL_DEPTH) + 256);
          }
        }
        const int s = (KS == 2) ? (d & 1) : 0;               // (DEPTH is even: step parity == slot parity)
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
          for (int u = 0; u < POL_MT; u++) {
            f32x4 c = acc[u][t][s];
            if (BF) {
              const bf16x8 av = pol_to_bf16(a[u][0], a[u][1]);
              const bf16x8 bv = *(const bf16x8*)&cur[t][0];
              c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, c, 0, 0, 0);
            } else {
              c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][0].x, cur[t][0].x, c, 0, 0, 0);
              c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][0].y, cur[t][0].y, c, 0, 0, 0);
              c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][0].z, cur[t][0].z, c, 0, 0, 0);
              c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][0].w, cur[t][0].w, c, 0, 0, 0);
              c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][1].x, cur[t][1].x, c, 0, 0, 0);
              c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][1].y, cur[t][1].y, c, 0, 0, 0);
              c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][1].z, cur[t][1].z, c, 0, 0, 0);
              c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][1].w, cur[t][1].w, c, 0, 0, 0);
            }
            acc[u][t][s] = c;
          }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < NT; t++) {
    if (wave + POL_WAVES * t >= NTILES) break;
    const int n = (wave + POL_WAVES * t) * 16 + m;           // D: column on the lane (lane & 15), rows 4 g + i in the registers
    const float bias = w.bias[t];
#pragma unroll
    for (int u = 0; u < POL_MT; u++) {
      f32x4 c = acc[u][t][0];
      if (KS == 2) c += acc[u][t][KS - 1];
      c += bias;
      if (LAST) {
        out[t][u] = c;
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++) Y[(16 * u + 4 * g + i) * ldy + n] = pol_tanh(c[i]);
      }
    }
  }
}

}  // namespace
#endif /* AUV_POLICY_MFMA_H */
