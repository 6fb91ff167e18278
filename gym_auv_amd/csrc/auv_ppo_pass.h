// The bodies of the PPO / clone update's launches, templates on the hidden widths A = PolArch<H1, H2, H3> (auv_policy_mfma.h): the row
// pass, the weight-gradient pass, the reduction, clip + Adam and their host-side launch sequences.  Two translation units instantiate
// them: k8_ppo_update.hip for the reference's widths (kernels k8_*), k13_ppo_update_arch.hip for the other listed triples (k13_ppo_*).
// What the launches compute is described at the head of k8_ppo_update.hip.
#ifndef AUV_PPO_PASS_H
#define AUV_PPO_PASS_H
#include "auv_ppo.h"
#include "auv_policy_mfma.h"

namespace {

// floats of the transposed copy of one net: W2^T [H1][H2] | W3^T [H2][H3] | W4^T [H3][32] (columns padded to 32)
__host__ __device__ inline size_t ppo_tr_floats_h(int h1, int h2, int h3) { return (size_t)h1 * h2 + (size_t)h2 * h3 + (size_t)h3 * 32; }
template <class A>
__host__ __device__ constexpr int ppo_tr_floats() { return A::H1 * A::H2 + A::H2 * A::H3 + A::H3 * 32; }

__host__ __device__ inline size_t ppo_net_params_h(int h1, int h2, int h3, int D, int out) {      // torch layout: W1 b1 W2 b2 W3 b3 W4 b4
  return (size_t)h1 * D + h1 + (size_t)h2 * h1 + h2 + (size_t)h3 * h2 + h3 + (size_t)out * h3 + out;
}
__host__ __device__ inline size_t ppo_params_h(int h1, int h2, int h3, int D) {
  return ppo_net_params_h(h1, h2, h3, D, 2) + ppo_net_params_h(h1, h2, h3, D, 1) + 2;
}
template <class A>
__host__ __device__ inline size_t ppo_net_params(int D, int out) { return ppo_net_params_h(A::H1, A::H2, A::H3, D, out); }
template <class A>
__host__ __device__ inline size_t ppo_params(int D) { return ppo_params_h(A::H1, A::H2, A::H3, D); }

// LDS of the row pass (floats): X | Y1 | Y2 | Y3 | D4 | D3 | D2 | 16 source rows (int64) | a counter.  Row strides = 8 mod 64 floats, the
// rule of k6_policy.hip: the 16-byte reads of an A operand then touch every bank once (D4 holds 32 columns in rows of 72 for that; X's
// stride K0p + 8 is k6's own, 40 at K0p = 32)
__host__ __device__ inline size_t ppo_lds_floats_h(int h1, int h2, int h3, int obs_dim) {
  return (size_t)16 * ((pol_pad16(obs_dim) + 8) + (h1 + 8) + 2 * (h2 + 8) + 2 * (h3 + 8) + 72) + 32 + 4;
}

// position of element [n][k] of a [N][Kp] matrix in MFMA fragment order (include/auv_hip.h, auv_policy_io)
__host__ __device__ inline size_t ppo_frag(int n, int k, int Kp) {
  return ((((size_t)(n / 16) * (Kp / 32) + k / 32) * 2 + (k % 8) / 4) * 64 + ((k % 32) / 8) * 16 + n % 16) * 4 + k % 4;
}

// Where flat parameter p (torch layout) lives: `pad` its position in a padded row-major net (the split partials), `fwd` in the forward
// copy, `tr` in the transposed copy (-1: none).  group 0: policy net and log_std, 1: value net.
struct PpoWhere {
  long long pad, fwd, tr;
  int group;
};
template <class A>
__device__ inline PpoWhere ppo_where(long long p, const int D, const int K0p) {
  PpoWhere w;
  const long long n0 = (long long)ppo_net_params<A>(D, 2), n1 = (long long)ppo_net_params<A>(D, 1);
  const long long netf = (long long)pol_net_floats<A>(D);
  w.tr = -1;
  if (p >= n0 + n1) {                                            // log_std
    w.group = 0, w.pad = -1, w.fwd = 2 * netf + (p - n0 - n1);
    return w;
  }
  const int net = p >= n0;
  long long q = net ? p - n0 : p;
  w.group = net;
  const int in[4] = {D, A::H1, A::H2, A::H3}, inp[4] = {K0p, A::H1, A::H2, A::H3};
  const int out[4] = {A::H1, A::H2, A::H3, net ? 1 : 2}, outp[4] = {A::H1, A::H2, A::H3, POL_OUT};
  const long long troff[4] = {0, 0, (long long)A::H1 * A::H2, (long long)A::H1 * A::H2 + A::H2 * A::H3};
  long long off = net * netf;
  for (int l = 0; l < 4; l++) {
    const long long nw = (long long)out[l] * in[l];
    if (q < nw) {
      const int n = (int)(q / in[l]), k = (int)(q - (long long)n * in[l]);
      w.pad = off + (long long)n * inp[l] + k;
      w.fwd = off + (long long)ppo_frag(n, k, inp[l]);
      if (l > 0) w.tr = net * (long long)ppo_tr_floats<A>() + troff[l] + (long long)ppo_frag(k, n, l == 3 ? 32 : outp[l]);
      return w;
    }
    q -= nw, off += (long long)outp[l] * inp[l];
    if (q < out[l]) {
      w.pad = w.fwd = off + q;
      return w;
    }
    q -= out[l], off += outp[l];
  }
  w.pad = w.fwd = 0;                                             // (not reached: p < n0 + n1)
  return w;
}

// ---------------------------------------------------------------------------------------------------------------- row pass
template <class Batch>                                             // auv_ppo_batch_t: the PPO head; auv_ppo_squash_batch_t: PPO with the squashed
                                                                   // distribution's entropy; auv_ppo_clone_batch_t: the supervised head
struct RowArgs {
  AuvPpoDev d;
  Batch b;
};

__device__ __forceinline__ int ppo_bad(const float x) { return !(fabsf(x) <= 3.402823466e38f); }   // NaN or +-inf

// a [16][cols] LDS matrix -> its 16 x 16 blocks of row tile rt in the scratch
__device__ __forceinline__ void ppo_store_blocks(const float* __restrict__ M, const int ld, const int nct, float* __restrict__ dst,
                                                 const int rt, const int tid) {
  float* base = dst + (size_t)rt * nct * 256;
  for (int q = tid; q < nct * 64; q += POL_THREADS) {
    const int ct = q >> 6, l = q & 63, g = l >> 4, c = l & 15;
    const float* s = M + (4 * g) * ld + ct * 16 + c;
    *(float4*)(base + 4 * (size_t)q) = make_float4(s[0], s[ld], s[2 * ld], s[3 * ld]);
  }
}

// the epilogue of a backward layer: dZ = (dZ_next W_next) * (1 - Y^2) of this wave's n-tiles, into LDS (the next layer's A operand,
// nullable) and into the scratch, where a lane's four registers are one float4 of the tile's block
template <int NTILES>
__device__ __forceinline__ void ppo_back_store(f32x4 (*o)[POL_MT], const float* __restrict__ Y, const int ldy, float* __restrict__ Dl, const int ldd,
                                               float* __restrict__ dst, const int rt, const int wave, const int lane) {
  if (wave >= NTILES) return;
  const int c = lane & 15, g = lane >> 4;
#pragma unroll
  for (int t = 0; t < (NTILES + POL_WAVES - 1) / POL_WAVES; t++) {
    const int tile = wave + POL_WAVES * t;
    if (tile >= NTILES) break;
    const int n = tile * 16 + c;
    f32x4 dz;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float y = Y[(4 * g + i) * ldy + n];
      dz[i] = o[t][0][i] * (1.0f - y * y);
    }
    if (Dl) {
#pragma unroll
      for (int i = 0; i < 4; i++) Dl[(4 * g + i) * ldd + n] = dz[i];
    }
    *(float4*)(dst + ((size_t)rt * NTILES + tile) * 256 + 4 * lane) = make_float4(dz[0], dz[1], dz[2], dz[3]);
  }
}

// The head of k8_rows (wave 0, between the forward and the backward pass): o = this lane's four rows 4 g + i of output column n of
// the net (the policy's mean, the value), srow the tile's source rows (-1: padding).  Returns d loss / d o and writes the tile's
// statistics; the overloads on the batch's type pick the head: PPO's (SQUASH false), PPO's with the squashed distribution's entropy
// (true, auv_ppo_squash_batch_t: the same fields), the supervised head of k8_clone below.
//   SQUASH (include/auv_hip.h, auv_ppo_grad_squash): ent_i = sum_k [0.5 + log sqrt(2 pi) + log_std_k + log(1 - tanh^2 a_ik)] of the
//   STORED action a = mu + sigma sg(z), log(1 - tanh^2 a) = 2 (log 2 - |a| - log1p(exp(-2 |a|))).  On top of PPO's gradients:
//   d loss / d mu_ik += ent_coef 2 tanh(a_ik) / B;  d loss / d log_std_k += ent_coef (1 / B) sum_i 2 tanh(a_ik) (a_ik - mu_ik) (folded
//   into the tile's d log_std slots: the reduction still subtracts the constant ent_coef).  The tile's sum of log(1 - tanh^2) goes to
//   a ninth slot behind the [rt_max][8] table.  With ent_coef == 0 nothing is added anywhere: PPO's bits.
template <class A, bool SQUASH, class Batch>
__device__ __forceinline__ f32x4 ppo_head_pg(const AuvPpoDev& d, const Batch& b, const int net, const int rt, const int lane, const f32x4 o,
                                             const long long* __restrict__ srow, const int* __restrict__ nbad) {
  const size_t netf = pol_net_floats<A>(d.obs_dim);
  const int B = b.B;
  const int n = lane & 15, g = lane >> 4;
  const float invB = 1.0f / (float)B;
  f32x4 d4 = {0.0f, 0.0f, 0.0f, 0.0f};
  float* ts = d.tstat + 8 * (size_t)rt;
  if (net == 0) {
    const int nc = n < 2 ? n : 0;
    const float ls = (d.fwd + 2 * netf)[nc];
    const float sigma = expf(ls);
    const float lo = 1.0f - b.clip, hi = 1.0f + b.clip;
    float s_pg = 0.0f, s_clip = 0.0f, s_dls = 0.0f, mx_adv = 0.0f, mx_ratio = 0.0f;
    float s_lj = 0.0f, s_tu = 0.0f;                                // SQUASH: sums of log(1 - tanh^2 a) and of 2 tanh(a) (a - mu)
    const bool ent_on = SQUASH && b.ent_coef != 0.0f;
    int bad = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const long long s = srow[4 * g + i];
      const bool valid = s >= 0;
      const size_t sr = valid ? (size_t)s : 0;
      const float a = valid ? b.A[2 * sr + nc] : 0.0f, lpo = valid ? b.LP[sr] : 0.0f, adv = valid ? b.ADV[sr] : 0.0f;
      const float ret = valid ? b.RET[sr] : 0.0f;
      const float mu = o[i];
      const float z = (a - mu) / sigma;
      float lp = -0.5f * (z * z) - ls - POL_LOG_SQRT_2PI;
      lp += __shfl_xor(lp, 1, AUV_WAVE);                         // the two components sit on neighbouring lanes
      const float ratio = expf(lp - lpo);
      const float pgi = -fminf(ratio * adv, fminf(fmaxf(ratio, lo), hi) * adv);
      const bool clipped = (adv > 0.0f && ratio > hi) || (adv < 0.0f && ratio < lo);
      const float glp = clipped ? 0.0f : -adv * ratio * invB;
      if (valid && n < 2) {
        d4[i] = glp * ((a - mu) / (sigma * sigma));
        s_dls += glp * (z * z - 1.0f);
        bad += ppo_bad(a);
        if (SQUASH) {
          const float au = fabsf(a), th2 = 2.0f * pol_squash_tanh(a);
          s_lj += 2.0f * (0.6931471805599453f - au - log1pf(expf(-2.0f * au)));
          s_tu += th2 * (a - mu);
          if (ent_on) d4[i] += b.ent_coef * th2 * invB;
        }
      }
      if (valid && n == 0) {
        s_pg += pgi, s_clip += clipped ? 1.0f : 0.0f;
        mx_adv = fmaxf(mx_adv, fabsf(adv)), mx_ratio = fmaxf(mx_ratio, ratio);
        bad += ppo_bad(lpo) + ppo_bad(adv) + ppo_bad(ret);
      }
    }
    // the four row groups of a column: a butterfly over lanes n, n + 16, n + 32, n + 48 (the same order on every call)
#pragma unroll
    for (int sh = 16; sh <= 32; sh <<= 1) {
      s_pg += __shfl_xor(s_pg, sh, AUV_WAVE), s_clip += __shfl_xor(s_clip, sh, AUV_WAVE), s_dls += __shfl_xor(s_dls, sh, AUV_WAVE);
      mx_adv = fmaxf(mx_adv, __shfl_xor(mx_adv, sh, AUV_WAVE)), mx_ratio = fmaxf(mx_ratio, __shfl_xor(mx_ratio, sh, AUV_WAVE));
      bad += __shfl_xor(bad, sh, AUV_WAVE);
      if (SQUASH) s_lj += __shfl_xor(s_lj, sh, AUV_WAVE), s_tu += __shfl_xor(s_tu, sh, AUV_WAVE);
    }
    bad += __shfl_xor(bad, 1, AUV_WAVE);                         // (lane 1 counted the second action component)
    if (SQUASH) {
      if (ent_on) s_dls += b.ent_coef * invB * s_tu;
      s_lj += __shfl_xor(s_lj, 1, AUV_WAVE);
      if (lane == 0) d.tstat[8 * (size_t)d.rt_max + rt] = s_lj;
    }
    if (lane == 0) ts[0] = s_pg, ts[2] = mx_adv, ts[3] = mx_ratio, ts[4] = (float)(bad + *nbad), ts[5] = s_clip, ts[6] = s_dls;
    if (lane == 1) ts[7] = s_dls;
  } else {
    float s_vf = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const long long s = srow[4 * g + i];
      const bool valid = s >= 0 && n == 0;
      const float ret = valid ? b.RET[(size_t)s] : 0.0f;
      const float e = o[i] - ret;
      if (valid) d4[i] = b.vf_coef * e * invB, s_vf += 0.5f * (e * e);
    }
    s_vf += __shfl_xor(s_vf, 16, AUV_WAVE);
    s_vf += __shfl_xor(s_vf, 32, AUV_WAVE);
    if (lane == 0) ts[1] = s_vf;
  }
  return d4;
}

template <class A>
__device__ __forceinline__ f32x4 ppo_head(const AuvPpoDev& d, const auv_ppo_batch_t& b, const int net, const int rt, const int lane, const f32x4 o,
                                          const long long* __restrict__ srow, const int* __restrict__ nbad) {
  return ppo_head_pg<A, false>(d, b, net, rt, lane, o, srow, nbad);
}
template <class A>
__device__ __forceinline__ f32x4 ppo_head(const AuvPpoDev& d, const auv_ppo_squash_batch_t& b, const int net, const int rt, const int lane,
                                          const f32x4 o, const long long* __restrict__ srow, const int* __restrict__ nbad) {
  return ppo_head_pg<A, true>(d, b, net, rt, lane, o, srow, nbad);
}

// The supervised head of k8_clone (include/auv_hip.h, auv_ppo_grad_clone): the policy towards the target actions A (kind 0: the
// Gaussian negative log-likelihood, 1: the squared error of the mean), the value net towards RET, every row times its weight.
//   kind 0: d bc / d mu_ik = -w_i (a_ik - mu_ik) / sigma_k^2 / B, d bc / d log_std_k = sum_i w_i (1 - z_ik^2) / B
//   kind 1: d bc / d mu_ik = -w_i (a_ik - mu_ik) / B, nothing for log_std;   d loss / d v_i = vf_coef w_i (v_i - ret_i) / B
// Laid out as the head above: components on neighbouring lanes, the same butterfly, the same non-finite count.  tstat: sum bc, sum vf,
// max |a - mu| over rows of weight > 0, sum w, non-finite inputs, 0, d log_std[2] -- what k8_reduce (clone) turns into stats[8].
template <class A>
__device__ __forceinline__ f32x4 ppo_head(const AuvPpoDev& d, const auv_ppo_clone_batch_t& b, const int net, const int rt, const int lane,
                                          const f32x4 o, const long long* __restrict__ srow, const int* __restrict__ nbad) {
  const int n = lane & 15, g = lane >> 4;
  const float invB = 1.0f / (float)b.B;
  f32x4 d4 = {0.0f, 0.0f, 0.0f, 0.0f};
  float* ts = d.tstat + 8 * (size_t)rt;
  if (net == 0) {
    const int nc = n < 2 ? n : 0;
    const float ls = (d.fwd + 2 * pol_net_floats<A>(d.obs_dim))[nc];
    const float sigma = expf(ls);
    const bool nll = b.kind == 0;
    float s_bc = 0.0f, s_w = 0.0f, s_dls = 0.0f, mx_err = 0.0f;
    int bad = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const long long s = srow[4 * g + i];
      const bool valid = s >= 0;
      const size_t sr = valid ? (size_t)s : 0;
      const float a = valid ? b.A[2 * sr + nc] : 0.0f, ret = valid ? b.RET[sr] : 0.0f;
      const float w = valid ? (b.W ? b.W[sr] : 1.0f) : 0.0f;
      const float e = a - o[i];
      const float z = e / sigma;
      float bc = w * (nll ? 0.5f * (z * z) + ls + POL_LOG_SQRT_2PI : 0.5f * (e * e));
      bc += __shfl_xor(bc, 1, AUV_WAVE);                         // the two components sit on neighbouring lanes
      if (valid && n < 2) {
        d4[i] = nll ? -w * (e / (sigma * sigma)) * invB : -w * e * invB;
        if (nll) s_dls += w * (1.0f - z * z) * invB;
        if (w > 0.0f) mx_err = fmaxf(mx_err, fabsf(e));
        bad += ppo_bad(a);
      }
      if (valid && n == 0) {
        s_bc += bc, s_w += w;
        bad += ppo_bad(ret) + (b.W ? ppo_bad(w) : 0);
      }
    }
#pragma unroll
    for (int sh = 16; sh <= 32; sh <<= 1) {
      s_bc += __shfl_xor(s_bc, sh, AUV_WAVE), s_w += __shfl_xor(s_w, sh, AUV_WAVE), s_dls += __shfl_xor(s_dls, sh, AUV_WAVE);
      mx_err = fmaxf(mx_err, __shfl_xor(mx_err, sh, AUV_WAVE));
      bad += __shfl_xor(bad, sh, AUV_WAVE);
    }
    bad += __shfl_xor(bad, 1, AUV_WAVE);
    mx_err = fmaxf(mx_err, __shfl_xor(mx_err, 1, AUV_WAVE));
    if (lane == 0) ts[0] = s_bc, ts[2] = mx_err, ts[3] = s_w, ts[4] = (float)(bad + *nbad), ts[5] = 0.0f, ts[6] = s_dls;
    if (lane == 1) ts[7] = s_dls;
  } else {
    float s_vf = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const long long s = srow[4 * g + i];
      const bool valid = s >= 0 && n == 0;
      const float ret = valid ? b.RET[(size_t)s] : 0.0f;
      const float w = valid ? (b.W ? b.W[(size_t)s] : 1.0f) : 0.0f;
      const float e = o[i] - ret;
      if (valid) d4[i] = b.vf_coef * (w * e) * invB, s_vf += w * (0.5f * (e * e));
    }
    s_vf += __shfl_xor(s_vf, 16, AUV_WAVE);
    s_vf += __shfl_xor(s_vf, 32, AUV_WAVE);
    if (lane == 0) ts[1] = s_vf;
  }
  return d4;
}

// The row pass of one workgroup, 16 rows of net `net` (row tile rt): gather, forward, ppo_head of the batch's type, backward
template <class A, class Batch>
__device__ __forceinline__ void ppo_row_pass(const AuvPpoDev& d, const Batch& b, const int net, const int rt) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, wave = tid / AUV_WAVE, lane = tid % AUV_WAVE;
  const int r0 = rt * 16;
  const int K0 = d.obs_dim, K0p = d.k0p, B = b.B;
  const int ldx = K0p + 8, ld1 = A::H1 + 8, ld2 = A::H2 + 8, ld3 = A::H3 + 8, ld4 = 72;
  float* X = (float*)smem;
  float* Y1 = X + 16 * ldx;
  float* Y2 = Y1 + 16 * ld1;
  float* Y3 = Y2 + 16 * ld2;
  float* D4 = Y3 + 16 * ld3;
  float* D3 = D4 + 16 * ld4;
  float* D2 = D3 + 16 * ld3;
  long long* srow = (long long*)(D2 + 16 * ld2);                 // (every part is a multiple of 16 floats long: 8-byte aligned)
  int* nbad = (int*)(srow + 16);
  const size_t netf = pol_net_floats<A>(K0);
  const float* P = d.fwd + (size_t)net * netf;
  const float* W1 = P;
  const float* b1 = W1 + (size_t)A::H1 * K0p;
  const float* W2 = b1 + A::H1;
  const float* b2 = W2 + (size_t)A::H2 * A::H1;
  const float* W3 = b2 + A::H2;
  const float* b3 = W3 + (size_t)A::H3 * A::H2;
  const float* W4 = b3 + A::H3;
  const float* b4 = W4 + (size_t)POL_OUT * A::H3;
  const float* T2 = d.tr + (size_t)net * ppo_tr_floats<A>();
  const float* T3 = T2 + A::H1 * A::H2;
  const float* T4 = T3 + A::H2 * A::H3;
  PolW<A::H1 / 16, false> w1;
  PolW<A::H2 / 16, false> w2;
  PolW<A::H3 / 16, false> w3;
  PolW<1, false> w4;
  pol_prefetch(w1, W1, b1, K0p, wave, lane);
  // ---- the tile's rows, gathered through idx, zero padded ----
  for (int q = tid; q < 16 * (ldx / 2); q += POL_THREADS) *(float2*)(X + 2 * q) = make_float2(0.0f, 0.0f);
  if (tid < 16) srow[tid] = r0 + tid < B ? (b.idx ? (long long)b.idx[r0 + tid] : (long long)(r0 + tid)) : -1;
  if (tid == 0) *nbad = 0;
  __syncthreads();
  {
    const int row = tid >> 5;                                    // 32 threads per row
    const long long s = srow[row];
    int bad = 0;
    if (s >= 0) {
      const float* src = b.O + (size_t)s * K0;
      for (int c = tid & 31; c < K0; c += 32) {
        const float v = src[c];
        X[row * ldx + c] = v;
        bad += ppo_bad(v);
      }
    }
    if (net == 0 && bad) atomicAdd(nbad, bad);                   // (an integer count in LDS: order does not matter)
  }
  __syncthreads();
  pol_prefetch(w2, W2, b2, A::H1, wave, lane);
  pol_layer<A::H1 / 16, 1, false, false>(X, ldx, w1, b1, K0p, wave, lane, Y1, ld1, nullptr);
  __syncthreads();
  pol_prefetch(w3, W3, b3, A::H2, wave, lane);
  pol_layer<A::H2 / 16, 1, false, false>(Y1, ld1, w2, b2, A::H1, wave, lane, Y2, ld2, nullptr);
  __syncthreads();
  pol_prefetch(w4, W4, b4, A::H3, wave, lane);
  pol_layer<A::H3 / 16, 2, false, false>(Y2, ld2, w3, b3, A::H2, wave, lane, Y3, ld3, nullptr);
  __syncthreads();
  PolW<A::H3 / 16, false> t4;
  pol_prefetch(t4, T4, d.zero, 32, wave, lane);                  // (W4^T: in flight during the head)
  if (wave == 0) {
    f32x4 o[1][POL_MT];
    pol_layer<1, 2, true, false>(Y3, ld3, w4, b4, A::H3, 0, lane, nullptr, 0, o);
    const f32x4 d4 = ppo_head<A>(d, b, net, rt, lane, o[0][0], srow, nbad);
    const int n = lane & 15, g = lane >> 4;
#pragma unroll
    for (int i = 0; i < 4; i++) D4[(4 * g + i) * ld4 + n] = d4[i], D4[(4 * g + i) * ld4 + 16 + n] = 0.0f;
    *(float4*)(d.dZ[net][3] + (size_t)rt * 256 + 4 * lane) = make_float4(d4[0], d4[1], d4[2], d4[3]);
  }
  __syncthreads();
  // ---- backward through the hidden layers: the "weights" are W_{l+1}^T, the "bias" zero, the epilogue * (1 - Y_l^2) ----
  PolW<A::H2 / 16, false> t3;
  PolW<A::H1 / 16, false> t2;
  f32x4 o3[PolW<A::H3 / 16, false>::NT][POL_MT], o2[PolW<A::H2 / 16, false>::NT][POL_MT], o1[PolW<A::H1 / 16, false>::NT][POL_MT];
  pol_prefetch(t3, T3, d.zero, A::H3, wave, lane);
  pol_layer<A::H3 / 16, 1, true, false>(D4, ld4, t4, d.zero, 32, wave, lane, nullptr, 0, o3);
  ppo_back_store<A::H3 / 16>(o3, Y3, ld3, D3, ld3, d.dZ[net][2], rt, wave, lane);
  __syncthreads();
  pol_prefetch(t2, T2, d.zero, A::H2, wave, lane);
  pol_layer<A::H2 / 16, 1, true, false>(D3, ld3, t3, d.zero, A::H3, wave, lane, nullptr, 0, o2);
  ppo_back_store<A::H2 / 16>(o2, Y2, ld2, D2, ld2, d.dZ[net][1], rt, wave, lane);
  __syncthreads();
  pol_layer<A::H1 / 16, 1, true, false>(D2, ld2, t2, d.zero, A::H2, wave, lane, nullptr, 0, o1);
  ppo_back_store<A::H1 / 16>(o1, Y1, ld1, nullptr, 0, d.dZ[net][0], rt, wave, lane);
  // ---- the inputs of the weight-gradient pass: X (once: the policy net's workgroup), Y1, Y2, Y3 ----
  if (net == 0) ppo_store_blocks(X, ldx, K0p / 16, d.X, rt, tid);
  ppo_store_blocks(Y1, ld1, A::H1 / 16, d.Y[net][0], rt, tid);
  ppo_store_blocks(Y2, ld2, A::H2 / 16, d.Y[net][1], rt, tid);
  ppo_store_blocks(Y3, ld3, A::H3 / 16, d.Y[net][2], rt, tid);
}

// ------------------------------------------------------------------------------------------------------ weight-gradient pass
#define WG_WAVES 4
#define WG_KT 4                    // 16 x 16 output tiles per workgroup: one n-tile, up to four k-tiles

struct WgArgs {
  AuvPpoDev d;
  int32_t rt, nsplit;
};

// The units of a net: per layer (n-tiles = out / 16) x (k-groups = ceil((in / 16) / WG_KT)); at the reference's widths 16 g1 + 32 + 8 + 1,
// at [64, 64, 64] 4 g1 + 4 + 4 + 1 (a layer of 64 inputs is one whole k-group).  G: the k-groups of layers 1 .. 3.
template <class A>
struct PpoWg {
  static constexpr int G1 = (A::H1 / 16 + WG_KT - 1) / WG_KT, G2 = (A::H2 / 16 + WG_KT - 1) / WG_KT, G3 = (A::H3 / 16 + WG_KT - 1) / WG_KT;
  static constexpr int U1 = (A::H2 / 16) * G1, U2 = (A::H3 / 16) * G2, U3 = G3;
};
__host__ __device__ inline int ppo_wg_groups0(int K0p) { return (K0p / 16 + WG_KT - 1) / WG_KT; }
template <class A>
__host__ __device__ inline int ppo_wg_units(int K0p) { return (A::H1 / 16) * ppo_wg_groups0(K0p) + PpoWg<A>::U1 + PpoWg<A>::U2 + PpoWg<A>::U3; }

// grid (2 * units, nsplit).  A: blocks of dZ_l (columns = this unit's 16 outputs n), B: blocks of Y_{l-1} (columns = 16 inputs k); lane
// (c, g) holds rows 4 g + j of column c as one float4, MFMA j multiplies element j of every lane: the sum over the 16 rows of a block.
template <class A>
__global__ void __launch_bounds__(64 * WG_WAVES) k8_wgrad(WgArgs wa) {
  __shared__ __align__(16) float red[WG_WAVES][WG_KT][256];
  __shared__ float redb[WG_WAVES][64];
  typedef PpoWg<A> G;
  const AuvPpoDev& d = wa.d;
  const int tid = threadIdx.x, wave = tid / AUV_WAVE, lane = tid % AUV_WAVE;
  const int K0p = d.k0p, units = ppo_wg_units<A>(K0p);
  const int net = blockIdx.x / units;
  int u = blockIdx.x % units;
  const int g1 = ppo_wg_groups0(K0p);
  int layer, nt, kt0, nkt;                                       // nkt: k-tiles of the layer
  if (u < (A::H1 / 16) * g1) layer = 0, nt = u / g1, kt0 = WG_KT * (u % g1), nkt = K0p / 16;
  else if ((u -= (A::H1 / 16) * g1) < G::U1) layer = 1, nt = u / G::G1, kt0 = WG_KT * (u % G::G1), nkt = A::H1 / 16;
  else if ((u -= G::U1) < G::U2) layer = 2, nt = u / G::G2, kt0 = WG_KT * (u % G::G2), nkt = A::H2 / 16;
  else layer = 3, nt = 0, kt0 = G::G3 == 1 ? 0 : WG_KT * (u - G::U2), nkt = A::H3 / 16;
  const int nk = nkt - kt0 < WG_KT ? nkt - kt0 : WG_KT;
  const int ncta = layer == 0 ? A::H1 / 16 : layer == 1 ? A::H2 / 16 : layer == 2 ? A::H3 / 16 : 1;
  const float* Am = d.dZ[net][layer];
  const float* Bm = layer == 0 ? d.X : d.Y[net][layer - 1];
  const int Q = wa.nsplit * WG_WAVES, q = blockIdx.y * WG_WAVES + wave;
  const int tps = (wa.rt + Q - 1) / Q;
  const int t0 = q * tps, t1 = t0 + tps < wa.rt ? t0 + tps : wa.rt;
  f32x4 acc[WG_KT];
#pragma unroll
  for (int j = 0; j < WG_KT; j++) acc[j] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
  float bsum = 0.0f;
  for (int t = t0; t < t1; t++) {
    const float4 av = *(const float4*)(Am + ((size_t)t * ncta + nt) * 256 + 4 * lane);
    float4 bv[WG_KT];
#pragma unroll
    for (int j = 0; j < WG_KT; j++)
      if (j < nk) bv[j] = *(const float4*)(Bm + ((size_t)t * nkt + kt0 + j) * 256 + 4 * lane);
#pragma unroll
    for (int j = 0; j < WG_KT; j++)
      if (j < nk) {
        f32x4 c = acc[j];
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv[j].x, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv[j].y, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv[j].z, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv[j].w, c, 0, 0, 0);
        acc[j] = c;
      }
    bsum += (av.x + av.y) + (av.z + av.w);
  }
#pragma unroll
  for (int j = 0; j < WG_KT; j++) *(float4*)&red[wave][j][4 * lane] = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
  redb[wave][lane] = bsum;
  __syncthreads();
  // padded row-major position of the layer's matrix and bias inside a net (the forward copy's offsets)
  const int inp = layer == 0 ? K0p : layer == 1 ? A::H1 : layer == 2 ? A::H2 : A::H3;
  size_t off = 0;
  if (layer >= 1) off += (size_t)A::H1 * K0p + A::H1;
  if (layer >= 2) off += (size_t)A::H2 * A::H1 + A::H2;
  if (layer >= 3) off += (size_t)A::H3 * A::H2 + A::H3;
  const size_t netf = pol_net_floats<A>(d.obs_dim);
  float* part = d.part + ((size_t)blockIdx.y * 2 + net) * netf + off;
  {
    // element tid of a tile: lane l = tid / 4 held it in register i = tid % 4 -> output row n = 4 (l / 16) + i, column k = l % 16
    const int l = tid >> 2, i = tid & 3;
    const int n = nt * 16 + 4 * (l >> 4) + i;
#pragma unroll
    for (int j = 0; j < WG_KT; j++)
      if (j < nk) {
        const float s = ((red[0][j][tid] + red[1][j][tid]) + red[2][j][tid]) + red[3][j][tid];
        part[(size_t)n * inp + (kt0 + j) * 16 + (l & 15)] = s;
      }
  }
  if (kt0 == 0 && tid < 16) {
    const int outp = layer == 0 ? A::H1 : layer == 1 ? A::H2 : layer == 2 ? A::H3 : POL_OUT;
    float s = 0.0f;
    for (int w = 0; w < WG_WAVES; w++)
      for (int g = 0; g < 4; g++) s += redb[w][16 * g + tid];
    part[(size_t)outp * inp + nt * 16 + tid] = s;
  }
}

// ------------------------------------------------------------------------------------------------- reduction of the partials
struct RedArgs {
  AuvPpoDev d;
  float* grad;
  float* stats;
  long long P;
  int32_t nsplit, rt, B;
  int32_t clone;                   // the tiles are k8_clone's: slot 3 is a sum (of the weights), not a maximum
  float vf_coef, ent_coef;
};

// blocks 0 .. ceil(P / 256) - 1: the flat gradient; the last block: statistics and the log_std gradient.  SQ: the tiles are the squash
// head's -- a ninth sum, of log(1 - tanh^2 a), lies behind the table; the entropy of the loss and of slot 7 is the squashed one
template <class A, bool SQ = false>
__global__ void __launch_bounds__(256) k8_reduce(RedArgs a) {
  const AuvPpoDev& d = a.d;
  const int tid = threadIdx.x;
  if (blockIdx.x + 1 < gridDim.x) {
    const long long p = (long long)blockIdx.x * 256 + tid;
    if (p >= a.P - 2) return;
    const PpoWhere w = ppo_where<A>(p, d.obs_dim, d.k0p);
    const size_t stride = 2 * pol_net_floats<A>(d.obs_dim);             // one split's partials: both nets
    const float* src = d.part + w.pad;
    float s = 0.0f;
    for (int k = 0; k < a.nsplit; k++) s += src[(size_t)k * stride];
    a.grad[p] = s;
    return;
  }
  constexpr int JQ = SQ ? 8 : 0;                                  // the ninth row (SQ only)
  __shared__ float red[SQ ? 9 : 8][256];
  float v[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (int t = tid; t < a.rt; t += 256) {
    const float* ts = d.tstat + 8 * (size_t)t;
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = (j == 2 || (j == 3 && !a.clone)) ? fmaxf(v[j], ts[j]) : v[j] + ts[j];
  }
#pragma unroll
  for (int j = 0; j < 8; j++) red[j][tid] = v[j];
  if (SQ) {
    float vq = 0.0f;
    for (int t = tid; t < a.rt; t += 256) vq += d.tstat[8 * (size_t)d.rt_max + t];
    red[JQ][tid] = vq;
  }
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (tid < h) {
#pragma unroll
      for (int j = 0; j < 8; j++)
        red[j][tid] = (j == 2 || (j == 3 && !a.clone)) ? fmaxf(red[j][tid], red[j][tid + h]) : red[j][tid] + red[j][tid + h];
      if (SQ) red[JQ][tid] += red[JQ][tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float invB = 1.0f / (float)a.B;
    const float* ls = d.fwd + 2 * pol_net_floats<A>(d.obs_dim);
    const float pg = red[0][0] * invB, vf = red[1][0] * invB;
    float ent = (0.5f + POL_LOG_SQRT_2PI + ls[0]) + (0.5f + POL_LOG_SQRT_2PI + ls[1]);
    if (SQ) ent += red[JQ][0] * invB;                              // + mean_i sum_k log(1 - tanh^2 a_ik)
    a.stats[0] = pg + a.vf_coef * vf - a.ent_coef * ent;
    a.stats[1] = pg, a.stats[2] = vf, a.stats[3] = red[2][0], a.stats[4] = red[3][0], a.stats[5] = red[4][0];
    a.stats[6] = red[5][0] * invB, a.stats[7] = SQ ? ent : 0.0f;
    a.grad[a.P - 2] = red[6][0] - a.ent_coef;
    a.grad[a.P - 1] = red[7][0] - a.ent_coef;
  }
}

// ------------------------------------------------------------------------------------------------------------ clip and Adam
struct AdamArgs {
  AuvPpoDev d;
  float* theta;
  float* m;
  float* v;
  const float* grad;
  float* norms_out;
  long long P;
  AuvPpoAdamDev h;
};

// AUV_PPO_NORM_BLOCKS blocks: block k sums the squares of its contiguous share of the flat gradient, per group, in double
__global__ void __launch_bounds__(256) k8_norm(const float* __restrict__ grad, const long long P, const long long n_pi, const long long n_v,
                                              double* __restrict__ sqpart) {
  __shared__ double red[2][256];
  const int tid = threadIdx.x;
  const long long per = (P + gridDim.x - 1) / gridDim.x;
  const long long p0 = (long long)blockIdx.x * per, p1 = p0 + per < P ? p0 + per : P;
  double s[2] = {0.0, 0.0};
  for (long long p = p0 + tid; p < p1; p += 256) {
    const double g = (double)grad[p];
    s[(p >= n_pi && p < n_pi + n_v) ? 1 : 0] += g * g;
  }
  red[0][tid] = s[0], red[1][tid] = s[1];
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (tid < h) red[0][tid] += red[0][tid + h], red[1][tid] += red[1][tid + h];
    __syncthreads();
  }
  if (tid == 0) sqpart[2 * blockIdx.x] = red[0][0], sqpart[2 * blockIdx.x + 1] = red[1][0];
}

// one thread per parameter.  LOAD: no update, only the scatter of theta into the packed copies (auv_ppo_load)
template <class A, bool LOAD>
__global__ void __launch_bounds__(256) k8_adam(AdamArgs a) {
  __shared__ float coef[2];
  const AuvPpoDev& d = a.d;
  const int tid = threadIdx.x;
  if (!LOAD) {
    if (tid == 0) {
      double sq[2] = {0.0, 0.0};
      for (int k = 0; k < AUV_PPO_NORM_BLOCKS; k++) sq[0] += d.sqpart[2 * k], sq[1] += d.sqpart[2 * k + 1];
#pragma unroll
      for (int g = 0; g < 2; g++) {
        // examples/ppo.py, clip_grad_norm: total = sqrt(sum), coef = (max_norm / (total + 1e-6)).clamp(max = 1)
        const float total = sqrtf((float)sq[g]), mx = g ? a.h.max_norm_v : a.h.max_norm_pi;
        coef[g] = mx > 0.0f ? fminf(mx / (total + 1e-6f), 1.0f) : 1.0f;
        if (blockIdx.x == 0) a.norms_out[g] = total;
      }
    }
    __syncthreads();
  }
  const long long p = (long long)blockIdx.x * 256 + tid;
  if (p >= a.P) return;
  const PpoWhere w = ppo_where<A>(p, d.obs_dim, d.k0p);
  float th = a.theta[p];
  if (!LOAD) {
    // torch.optim.Adam (amsgrad off, no weight decay): exp_avg.lerp_(g, 1 - beta1); exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2);
    // param.addcdiv_(exp_avg, exp_avg_sq.sqrt() / sqrt(bc2) + eps, value = -lr / bc1)
    const float g = a.grad[p] * coef[w.group];
    float m = a.m[p], v = a.v[p];
    m = fmaf(a.h.w1, g - m, m);
    v = fmaf(a.h.w2, g * g, v * a.h.b2);                            // (torch's addcmul: input + value * (g * g), addcdiv alike: one fma each)
    const float denom = sqrtf(v) / a.h.bc2_sqrt + a.h.eps;
    th = fmaf(-a.h.step_size, m / denom, th);
    a.m[p] = m, a.v[p] = v, a.theta[p] = th;
  }
  d.fwd[w.fwd] = th;
  if (w.tr >= 0) d.tr[w.tr] = th;
  if (d.pol) d.pol[w.fwd] = th;
}

// ------------------------------------------------------------------------------------------------------- host: the launches
// K names a translation unit's three row-pass kernels of width A -- rows, clone and squash (pointers to __global__ functions), picked by
// a head number (auv_ppo.h, AUV_PPO_HEAD_*); every other kernel is a template of this header.
template <class A>
inline size_t ppo_lds_bytes(int obs_dim) { return sizeof(float) * ppo_lds_floats_h(A::H1, A::H2, A::H3, obs_dim); }

// The dynamic LDS a row pass may ask for is an attribute of the KERNEL -- of the one instantiation that is launched -- not of an updater: it is
// set in front of every launch that needs more than the 64 KiB a kernel gets unasked, so updaters of different widths can live side by side.
template <class A, class K>
inline hipError_t ppo_prepare(int obs_dim, int head) {
  const size_t b = ppo_lds_bytes<A>(obs_dim);
  if (b <= 64 * 1024) return hipSuccess;
  const void* k = head == AUV_PPO_HEAD_CLONE ? (const void*)K::clone : head == AUV_PPO_HEAD_SQUASH ? (const void*)K::squash : (const void*)K::rows;
  return hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
}

// The split-K factor, a function of B, obs_dim and the widths alone (so the summation order is): about 16 row tiles per wave for large
// batches; for small ones at least two workgroups per CU (512) as long as every wave still has a row tile (nsplit * WG_WAVES <= rt).
template <class A>
inline int ppo_nsplit(int rt, int K0p) {
  const int blocks = 2 * ppo_wg_units<A>(K0p);
  const int fill = (512 + blocks - 1) / blocks, have = (rt + WG_WAVES - 1) / WG_WAVES;
  const int big = (rt + 16 * WG_WAVES - 1) / (16 * WG_WAVES), small = fill < have ? fill : have;
  const int s = big > small ? big : small;
  return s < 1 ? 1 : s > AUV_PPO_MAX_SPLIT ? AUV_PPO_MAX_SPLIT : s;
}

template <class A>
inline void ppo_launch_load(const AuvPpoDev& d, const float* theta, hipStream_t st) {
  AdamArgs a = {};
  a.d = d, a.theta = (float*)theta, a.P = (long long)ppo_params<A>(d.obs_dim);
  hipLaunchKernelGGL((k8_adam<A, true>), dim3((unsigned)((a.P + 255) / 256)), dim3(256), 0, st, a);
}

// the launches behind a row pass: weight gradients, then the flat gradient and the statistics (squash: the reduction that reads the
// squash head's ninth slot; the two other modes launch what they always did)
template <class A>
inline void ppo_launch_after_rows(const AuvPpoDev& d, int B, bool clone, float vf_coef, float ent_coef, float* grad, float* stats, hipStream_t st,
                                  bool squash = false) {
  const int rt = (B + 15) / 16, nsplit = ppo_nsplit<A>(rt, d.k0p);
  WgArgs wa;
  wa.d = d, wa.rt = rt, wa.nsplit = nsplit;
  hipLaunchKernelGGL(k8_wgrad<A>, dim3(2 * ppo_wg_units<A>(d.k0p), nsplit), dim3(64 * WG_WAVES), 0, st, wa);
  RedArgs re;
  re.d = d, re.grad = grad, re.stats = stats, re.P = (long long)ppo_params<A>(d.obs_dim);
  re.nsplit = nsplit, re.rt = rt, re.B = B, re.clone = clone, re.vf_coef = vf_coef, re.ent_coef = ent_coef;
  if (squash) hipLaunchKernelGGL((k8_reduce<A, true>), dim3((unsigned)((re.P + 255) / 256) + 1), dim3(256), 0, st, re);
  else hipLaunchKernelGGL(k8_reduce<A>, dim3((unsigned)((re.P + 255) / 256) + 1), dim3(256), 0, st, re);
}

template <class A, class K>
inline void ppo_launch_grad(const AuvPpoDev& d, const auv_ppo_batch_t& b, float* grad, float* stats, hipStream_t st) {
  RowArgs<auv_ppo_batch_t> ra;
  ra.d = d, ra.b = b;
  hipLaunchKernelGGL(K::rows, dim3((b.B + 15) / 16, 2), dim3(POL_THREADS), ppo_lds_bytes<A>(d.obs_dim), st, ra);
  ppo_launch_after_rows<A>(d, b.B, false, b.vf_coef, b.ent_coef, grad, stats, st);
}

template <class A, class K>
inline void ppo_launch_grad_clone(const AuvPpoDev& d, const auv_ppo_clone_batch_t& b, float* grad, float* stats, hipStream_t st) {
  RowArgs<auv_ppo_clone_batch_t> ra;
  ra.d = d, ra.b = b;
  hipLaunchKernelGGL(K::clone, dim3((b.B + 15) / 16, 2), dim3(POL_THREADS), ppo_lds_bytes<A>(d.obs_dim), st, ra);
  ppo_launch_after_rows<A>(d, b.B, true, b.vf_coef, b.ent_coef, grad, stats, st);
}

template <class A, class K>
inline void ppo_launch_grad_squash(const AuvPpoDev& d, const auv_ppo_squash_batch_t& b, float* grad, float* stats, hipStream_t st) {
  RowArgs<auv_ppo_squash_batch_t> ra;
  ra.d = d, ra.b = b;
  hipLaunchKernelGGL(K::squash, dim3((b.B + 15) / 16, 2), dim3(POL_THREADS), ppo_lds_bytes<A>(d.obs_dim), st, ra);
  ppo_launch_after_rows<A>(d, b.B, false, b.vf_coef, b.ent_coef, grad, stats, st, true);
}

template <class A>
inline void ppo_launch_adam(const AuvPpoDev& d, float* theta, float* m, float* v, const float* grad, const AuvPpoAdamDev& h, float* norms_out,
                            hipStream_t st) {
  AdamArgs a;
  a.d = d, a.theta = theta, a.m = m, a.v = v, a.grad = grad, a.norms_out = norms_out, a.P = (long long)ppo_params<A>(d.obs_dim), a.h = h;
  hipLaunchKernelGGL(k8_norm, dim3(AUV_PPO_NORM_BLOCKS), dim3(256), 0, st, grad, a.P, (long long)ppo_net_params<A>(d.obs_dim, 2),
                     (long long)ppo_net_params<A>(d.obs_dim, 1), d.sqpart);
  hipLaunchKernelGGL((k8_adam<A, false>), dim3((unsigned)((a.P + 255) / 256)), dim3(256), 0, st, a);
}

}  // namespace
#endif /* AUV_PPO_PASS_H */

