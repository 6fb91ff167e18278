// The forward pass of the policy MLP as the fused launches run it -- k6_policy_act, k9_policy_eval, k11_population_act,
// k12_stacked_act, k16_norm_act, k17_squash_act / _eval -- written once: the packed net's pointers, the LDS carve-up, the prefetch /
// layer / barrier sequence (pol_trunk), the counter-based generator, the action maps, log pi(a), and the whole ACT launch
// (pol_act_body: rollout position, transition, tile, trunk, sampling epilogue, counters; its host helpers) that k6, k12, k16 and k17
// instantiate with a Tile -- how the input tile is formed -- and a map.  What stays in a kernel file is its Tile.  (The PPO update,
// k8_ppo_update.hip, has its own sequence and includes auv_policy_mfma.h only.)
//
// The order of requests and barriers in here was measured line by line (profiles/r04, profiles/policy_trunk); the library is built
// with -ffp-contract=off and the tests compare bits across the launches.
#ifndef AUV_POLICY_FORWARD_H
#define AUV_POLICY_FORWARD_H
#include "auv_noise.h"
#include "auv_policy_mfma.h"

namespace {

// ---- one packed net (layout: pol_net_floats) ----
struct PolNet {
  const float *W1, *b1, *W2, *b2, *W3, *b3, *W4, *b4;
};
template <class A = PolArchRef>
__device__ __forceinline__ PolNet pol_net_ptrs(const float* P, const int K0) {
  PolNet n;
  n.W1 = P;
  n.b1 = n.W1 + (size_t)A::H1 * pol_pad16(K0);
  n.W2 = n.b1 + A::H1;
  n.b2 = n.W2 + (size_t)A::H2 * A::H1;
  n.W3 = n.b2 + A::H2;
  n.b3 = n.W3 + (size_t)A::H3 * A::H2;
  n.W4 = n.b3 + A::H3;
  n.b4 = n.W4 + (size_t)POL_OUT * A::H3;
  return n;
}

// ---- the LDS of a forward workgroup (pol_lds_x_floats / pol_lds_bytes): X at the base, rows of pol_ldx floats; Y1 behind it ----
// (plain values, not a struct of pointers and strides: with one between here and pol_layer the layers' epilogues lost their paired
// LDS stores and every launch 1 - 2 % of its time)
__device__ __forceinline__ int pol_ldx(const int K0) { return pol_pad16(K0) + 8; }
template <class A = PolArchRef>
__device__ __forceinline__ float* pol_tile_y1(float* X, const int K0) { return X + pol_lds_x_floats<A>(K0); }
template <class A = PolArchRef>
__device__ __forceinline__ float* pol_tiles_end(float* X, const int K0) { return pol_tile_y1<A>(X, K0) + pol_lds_y1_floats_h(A::H1, A::H3); }

// the input tile starts as zeros: padding columns and the rows past the end stay so.  A barrier goes between this and the fill.
__device__ __forceinline__ void pol_zero_tile(float* X, const int ldx, const int tid) {
  for (int i = tid; i < POL_ROWS * (ldx / 2); i += POL_THREADS) *(float2*)(X + 2 * i) = make_float2(0.0f, 0.0f);
}

// `n` floats of one contiguous range -> the tile's rows of K0 columns, and into `dstO` (nullable: the rollout's O[t], whose rows of
// the tile are one contiguous range too).  V = float2: K0 even, so rows start 8-byte aligned and no pair straddles two rows.
template <class V>
__device__ __forceinline__ void pol_fill_range(float* X, const int ldx, const float* src, float* dstO, const int n, const int K0,
                                               const int tid) {
  constexpr int W = sizeof(V) / sizeof(float);
  for (int idx = W * tid; idx < n; idx += W * POL_THREADS) {
    const V v = *(const V*)(src + idx);
    const int row = idx / K0, c = idx - row * K0;
    *(V*)(X + row * ldx + c) = v;
    if (dstO) *(V*)(dstO + idx) = v;
  }
}

// the policy net's output component a lane stands for: columns 0 and 1 of the last layer's n-tile are the two actions (the other
// lanes compute along as component 0 and store nothing)
__device__ __forceinline__ int pol_comp(const int lane) { return (lane & 15) < 2 ? (lane & 15) : 0; }

// ---- the forward pass: from the barrier behind the tile fill to the last layer's raw outputs (on wave 0, in `o`) ----
// X: the filled tile of K0 columns.  w1: requested by the caller BEFORE it fetched the tile (pol_prefetch).  log_std: nullable, this
// lane asks for its component's log-std (returned; 0 without).
// A: the hidden widths (PolArch; the reference's unless named); the sequence is the same for every one of them.
template <bool BF, class A = PolArchRef>
__device__ __forceinline__ float pol_trunk(float* X, const int K0, const PolNet& n, PolW<A::H1 / 16, BF>& w1, const float* log_std,
                                           const int wave, const int lane, f32x4 (*o)[POL_MT]) {
  const int K0p = pol_pad16(K0);
  const int ldx = pol_ldx(K0), ld1 = A::H1 + 8, ld2 = A::H2 + 8, ld3 = A::H3 + 8;
  float* Y1 = pol_tile_y1<A>(X, K0);
  float* Y2 = X;                                                   // (X is dead once layer 1 is through: a barrier lies in between)
  float* Y3 = Y1;                                                  // (Y1 is dead once layer 2 is through)
  PolW<A::H2 / 16, BF> w2;
  PolW<A::H3 / 16, BF> w3;
  PolW<1, BF> w4;
  __syncthreads();
  pol_prefetch(w2, n.W2, n.b2, A::H1, wave, lane);                 // (the next layer's weights: in flight during this layer)
  pol_layer<A::H1 / 16, 1, false, BF>(X, ldx, w1, n.b1, K0p, wave, lane, Y1, ld1, nullptr);
  __syncthreads();
  pol_prefetch(w3, n.W3, n.b3, A::H2, wave, lane);
  pol_layer<A::H2 / 16, 1, false, BF>(Y1, ld1, w2, n.b2, A::H1, wave, lane, Y2, ld2, nullptr);
  __syncthreads();
  pol_prefetch(w4, n.W4, n.b4, A::H3, wave, lane);
  // (the sampling's log-std with them: ahead of the barrier, so that the request is not moved down to its use)
  float ls = 0.0f;
  if (log_std) ls = log_std[pol_comp(lane)];
  pol_layer<A::H3 / 16, 2, false, BF>(Y2, ld2, w3, n.b3, A::H2, wave, lane, Y3, ld3, nullptr);
  __syncthreads();
  if (wave == 0) pol_layer<1, 2, true, BF>(Y3, ld3, w4, n.b4, A::H3, 0, lane, nullptr, 0, o);
  return ls;
}
// ---- the counter-based generator of the policy launches ----
// (seed, step, row, component) -> 64 well-mixed bits (pol_mix, the splitmix64 finaliser: auv_noise.h) -> a Gaussian
__device__ __forceinline__ float pol_gauss(unsigned long long seed, unsigned long long step, unsigned int row, unsigned int comp) {
  const unsigned long long h = pol_mix(pol_mix(seed ^ (step * 0xd1342543de82ef95ull)) ^ (((unsigned long long)row << 1) | comp));
  // (0, 1): 24 bits.  From 2^23 on field + 0.5 is a tie that rounds to even, and the top field's to 2^24 -- u1 = 1 and a draw that is
  // exactly 0 -- so the product is held below 1: that one field in 2^24 moves, every other draw keeps its bits
  const float u1 = fminf(((float)(unsigned int)(h >> 40) + 0.5f) * (1.0f / 16777216.0f), 0x1.fffffep-1f);
  const float u2 = ((float)(unsigned int)((h >> 8) & 0xffffffu)) * (1.0f / 16777216.0f);   // [0, 1)
  return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}

// ---- the action map of this lane's component: env action = act_mid + act_half * clamp(a, clip_lo, clip_hi) ----
// IO: any launch argument struct with clip_lo[2], clip_hi[2], act_mid[2], act_half[2].  nc = pol_comp(lane).
struct PolActMap {
  float clip_lo, clip_hi, act_mid, act_half;
  __device__ __forceinline__ float operator()(const float a) const {
    const float ac = fminf(fmaxf(a, clip_lo), clip_hi);
    return act_mid + act_half * ac;
  }
};
template <class IO>
__device__ __forceinline__ PolActMap pol_act_map(const IO& io, const int nc) {
  // launch arguments picked by a select (indexed by the lane they are vector loads from the argument segment, behind the stores of
  // every row: four trips to memory in the epilogue)
  float cl0 = io.clip_lo[0], cl1 = io.clip_lo[1], ch0 = io.clip_hi[0], ch1 = io.clip_hi[1];
  float am0 = io.act_mid[0], am1 = io.act_mid[1], ah0 = io.act_half[0], ah1 = io.act_half[1];
  asm volatile("" : "+s"(cl0), "+s"(cl1), "+s"(ch0), "+s"(ch1), "+s"(am0), "+s"(am1), "+s"(ah0), "+s"(ah1));   // (or the selects become indexed loads again)
  PolActMap m;
  m.clip_lo = nc ? cl1 : cl0, m.clip_hi = nc ? ch1 : ch0, m.act_mid = nc ? am1 : am0, m.act_half = nc ? ah1 : ah0;
  return m;
}

// ---- the action map of a squashed policy: env action = act_mid + act_half * tanh(a); clip_lo / clip_hi are not read ----
// (pol_squash_tanh: odd, exactly +-1 for large |a|, never NaN for a finite a; the launch arguments pinned as pol_act_map's)
struct PolSquashMap {
  float act_mid, act_half;
  __device__ __forceinline__ float operator()(const float a) const { return act_mid + act_half * pol_squash_tanh(a); }
};
template <class IO>
__device__ __forceinline__ PolSquashMap pol_squash_map(const IO& io, const int nc) {
  float am0 = io.act_mid[0], am1 = io.act_mid[1], ah0 = io.act_half[0], ah1 = io.act_half[1];
  asm volatile("" : "+s"(am0), "+s"(am1), "+s"(ah0), "+s"(ah1));
  PolSquashMap m;
  m.act_mid = nc ? am1 : am0, m.act_half = nc ? ah1 : ah0;
  return m;
}
// the map of a launch: SQUASH picks the functor at compile time (false: the clipped affine map, what every launch but k17's applies)
template <bool SQUASH, class IO>
__device__ __forceinline__ auto pol_map_of(const IO& io, const int nc) {
  if constexpr (SQUASH) return pol_squash_map(io, nc);
  else return pol_act_map(io, nc);
}

// log pi(a) of the diagonal Gaussian, both components summed (they sit on neighbouring lanes: every lane of the wave calls this)
__device__ __forceinline__ float pol_logp(const float a, const float mu, const float sigma, const float ls) {
  const float z = (a - mu) / sigma;
  float lp = -0.5f * z * z - ls - POL_LOG_SQRT_2PI;
  lp += __shfl_xor(lp, 1, AUV_WAVE);
  return lp;
}

// ---- the frame of an ACT launch (k6_policy_act, k12_stacked_act, k16_norm_act, k17_squash_act): grid (ceil(ne / 16), 2),
// blockIdx.y = 0 the policy net, 1 the value net; pol_act_body calls pol_act_begin first, pol_act_sample behind the trunk on wave 0,
// pol_act_end last ----
struct PolAct {
  bool host_counts, act, trans;
  long long t;                       // position in the rollout; t == T: the flush call after a rollout's last step
  unsigned long long gstep;          // the generator's step
  int e0, cnt, r0, col0;             // the slice, the tile's first row inside it and its first column in a rollout row
  float trans_r;
  uint8_t trans_d;
};

// t_host, gstep_host >= 0: the host names the rollout position and the generator's step (a plain loop of launches); -1: both live
// on the device (io.ctr) and the launch moves them on itself
__device__ __forceinline__ PolAct pol_act_begin(const auv_policy_io_t& io, const int e0, const int ne, const long long t_host,
                                                const long long gstep_host) {
  PolAct p;
  const int tid = threadIdx.x;
  p.e0 = e0, p.cnt = ne;
  p.r0 = blockIdx.x * POL_ROWS;
  // position in the rollout and the generator's step counter: read by every workgroup before anybody moves them on
  p.host_counts = t_host >= 0;
  p.t = p.host_counts ? t_host : io.ctr[0];
  p.gstep = (unsigned long long)(p.host_counts ? gstep_host : io.ctr[1]);
  p.col0 = e0 - io.env_base + p.r0;
  // ---- the transition the environment's last step completed: reward and done of step t - 1 ----
  // (requested here, stored at the end: load - store - load - store at the head of the kernel were two trips to memory in
  // front of everything wave 0 does, and wave 0 is the one that samples)
  p.trans = blockIdx.y == 0 && p.t >= 1 && p.t <= io.T && tid < POL_ROWS && p.r0 + tid < ne;
  p.trans_r = 0.0f, p.trans_d = 0;
  if (p.trans) p.trans_r = io.reward_in[e0 + p.r0 + tid], p.trans_d = io.done_in[e0 + p.r0 + tid];
  p.act = p.t < io.T;
  return p;
}

// where the policy workgroup copies its input tile in the rollout: O[t]'s rows of the tile, `width` columns each (nullptr: no copy)
__device__ __forceinline__ float* pol_act_obs_out(const auv_policy_io_t& io, const PolAct& p, const int width) {
  return (blockIdx.y == 0 && io.O) ? io.O + ((size_t)p.t * (size_t)io.ld + p.col0) * width : nullptr;
}
// the input tile of unstacked rows: the tile's rows are consecutive rows of the observation buffer, one contiguous range, read two
// floats per lane where obs_dim is even
__device__ __forceinline__ void pol_act_fill_obs(float* X, const auv_policy_io_t& io, const PolAct& p, float* dstO, const int rows) {
  const int K0 = io.obs_dim, ldx = pol_ldx(K0), tid = threadIdx.x;
  const float* src = io.obs + (size_t)(p.e0 + p.r0) * K0;
  if ((K0 & 1) == 0) pol_fill_range<float2>(X, ldx, src, dstO, rows * K0, K0, tid);
  else pol_fill_range<float>(X, ldx, src, dstO, rows * K0, K0, tid);
}

// wave 0, behind the trunk: `o` the last layer's outputs, `ls` the log-std the trunk returned.  SQUASH: what actions_out gets of the
// sample (pol_map_of); A, LP and everything else stored are the same either way
template <bool SQUASH = false>
__device__ __forceinline__ void pol_act_sample(const auv_policy_io_t& io, const PolAct& p, const f32x4 (*o)[POL_MT], const float ls,
                                               const int lane) {
  const int n = lane & 15, g = lane >> 4;
  const size_t ld = (size_t)io.ld;                                 // environments per rollout row
  if (blockIdx.y == 0) {
    // ---- diagonal Gaussian: sample, log-probability, action ----
    const int nc = pol_comp(lane);
    const float sigma = expf(ls);
    const auto map = pol_map_of<SQUASH>(io, nc);
#pragma unroll
    for (int u = 0; u < POL_MT; u++)
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int rr = 16 * u + 4 * g + i;                         // row inside the tile
        const int row = p.r0 + rr;
        const int e = p.e0 + row;
        const float mu = o[0][u][i];
        const float eps = pol_gauss(io.seed, p.gstep, (unsigned int)e, (unsigned int)nc);
        const float a = mu + sigma * eps;
        const float lp = pol_logp(a, mu, sigma, ls);
        if (n < 2 && row < p.cnt) {
          const size_t q = (size_t)p.t * ld + p.col0 + rr;
          io.A[2 * q + n] = a;
          if (n == 0) io.LP[q] = lp;
          io.actions_out[2 * (size_t)e + n] = map(a);
          if (io.mu_out) io.mu_out[2 * (size_t)row + n] = mu;
          if (io.eps_out) io.eps_out[2 * (size_t)row + n] = eps;
        }
      }
  } else if (n == 0) {
#pragma unroll
    for (int u = 0; u < POL_MT; u++)
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int rr = 16 * u + 4 * g + i;
        if (p.r0 + rr < p.cnt) io.V[(size_t)p.t * ld + p.col0 + rr] = o[0][u][i];
      }
  }
}

// every thread of the workgroup, last: the transition's store and the counters
__device__ __forceinline__ void pol_act_end(const auv_policy_io_t& io, const PolAct& p) {
  const int tid = threadIdx.x;
  const long long t = p.t;
  if (p.trans) {
    float r = p.trans_r;
    if (io.reward_clip > 0.0f) r = fminf(fmaxf(r, -io.reward_clip), io.reward_clip);
    io.R[(size_t)(t - 1) * (size_t)io.ld + p.col0 + tid] = r * io.reward_scale;
    io.Dn[(size_t)(t - 1) * (size_t)io.ld + p.col0 + tid] = p.trans_d ? 1.0f : 0.0f;
  }
  // ---- the rollout position and the generator's counter move on ----
  if (p.host_counts) {
    // the host named them (nobody in this launch reads io.ctr): one workgroup keeps the device copies in step, for a later
    // auv_policy_act on the same buffers
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
      if (t <= io.T) io.ctr[0] = t + 1;
      io.ctr[1] = (long long)(p.gstep + 1);
    }
    return;
  }
  // on the device (a launch that may sit in a captured graph): every workgroup has read them by the time it counts itself off,
  // the last one moves them.  (512 returning atomics on one word: ~4 of the 8 us an EMPTY launch of this grid takes -- why
  // auv_policy_rollout, a plain host loop, names the counters itself.)
  __syncthreads();
  if (tid == 0) {
    const unsigned long long total = (unsigned long long)gridDim.x * gridDim.y;
    const unsigned long long old = atomicAdd((unsigned long long*)&io.ctr[2], 1ull);
    if (old == total - 1) {
      io.ctr[2] = 0;
      if (t <= io.T) io.ctr[0] = t + 1;                            // (a flush call leaves T + 1: further calls do nothing)
      io.ctr[1] = (long long)(p.gstep + 1);
    }
  }
}

// ---- the act launch, written once: what an act kernel is launched with, the Tile contract, the body, the host's two helpers ----
// IO: auv_policy_io_t, or a struct that holds one as `io` (auv_policy_stack_t, auv_policy_norm_t)
template <class IO>
struct PolActArgs {
  IO io;
  int32_t e0, ne;
  long long t_host, gstep_host;      // >= 0: the host names the rollout position and the generator's step (auv_policy_rollout: a plain
                                     // loop of launches); -1: both live on the device (io.ctr) and the launch moves them on itself
};

// A Tile is what differs between the act launches: how the input tile is formed.  pol_act_body calls, in this order,
//   width()                      the net's input width K0
//   weights(A(), nw, net, K0p)   behind pol_net_ptrs: other weight pointers than the packed f32 ones (k6's bf16 variant)
//   Req rq(p)                    the thread's state of the step, made before `if (p.act)`; fill and finish get it back (the Tile is const)
//   request(A(), rq, X, p, rows) AHEAD of the barrier behind the tile's zeroing: loads whose values the fill needs, into rq, and LDS
//                                words behind the tiles (pol_tiles_end<A>: the launch's LDS size must cover what a Tile puts there)
//   fill(A(), X, p, rq, rows)    BEHIND that barrier: the rows of the tile into X, and into the rollout's O[t] (policy workgroup).  A
//                                fill that needs the whole raw tile before it goes on sets its own barrier (k16: one more than k6)
//   finish(p, rq)                outside `if (p.act)`, ahead of pol_act_end: the Tile's own state, stored last
// requests first, stores last -- the rule every kernel file's header states for its step.  The plain tile, consecutive rows of the
// observation buffer, is the base the others derive from: a Tile names only the hooks it changes.  (The hooks take the widths as a
// tag and X, not a pointer worked out here: a dead pol_tiles_end in the body cost the plain kernels two scalar registers --
// profiles/policy_frame.)
struct PolPlainTile {
  const auv_policy_io_t& io;
  struct Req {
    __device__ __forceinline__ explicit Req(const PolAct&) {}
  };
  __device__ __forceinline__ explicit PolPlainTile(const auv_policy_io_t& io_) : io(io_) {}
  __device__ __forceinline__ int width() const { return io.obs_dim; }
  template <class A>
  __device__ __forceinline__ void weights(A, PolNet&, const int, const int) const {}
  template <class A>
  __device__ __forceinline__ void request(A, Req&, float*, const PolAct&, const int) const {}
  template <class A>
  __device__ __forceinline__ void fill(A, float* X, const PolAct& p, const Req&, const int rows) const {
    pol_act_fill_obs(X, io, p, pol_act_obs_out(io, p, io.obs_dim), rows);
  }
  template <class R>
  __device__ __forceinline__ void finish(const PolAct&, const R&) const {}
};

// The launch's body, written once for every hidden-width triple A (PolArch, auv_policy_mfma.h), BF (bf16 weights), SQUASH (the map
// actions_out gets: pol_map_of) and Tile.
template <class A, bool BF, bool SQUASH, class IO, class Tile>
__device__ __forceinline__ void pol_act_body(const PolActArgs<IO>& pa, const Tile& tile) {
  extern __shared__ __align__(16) unsigned char smem[];
  const auv_policy_io_t& io = tile.io;
  const int tid = threadIdx.x, wave = tid / AUV_WAVE, lane = tid % AUV_WAVE;
  const int net = blockIdx.y;
  const int K0 = tile.width(), K0p = pol_pad16(K0);
  float* X = (float*)smem;
  const PolAct p = pol_act_begin(io, pa.e0, pa.ne, pa.t_host, pa.gstep_host);
  typename Tile::Req rq(p);
  if (p.act) {
    PolNet nw = pol_net_ptrs<A>(io.params + (size_t)net * pol_net_floats<A>(K0), K0);
    tile.weights(A(), nw, net, K0p);
    PolW<A::H1 / 16, BF> w1;
    pol_prefetch(w1, nw.W1, nw.b1, K0p, wave, lane);                 // (in flight while the tile is formed)
    const int rows = (p.cnt - p.r0 < POL_ROWS) ? p.cnt - p.r0 : POL_ROWS;
    tile.request(A(), rq, X, p, rows);
    // ---- input tile -> LDS (zero padded), and into the rollout (policy workgroup) ----
    pol_zero_tile(X, pol_ldx(K0), tid);
    __syncthreads();
    tile.fill(A(), X, p, rq, rows);
    f32x4 o[1][POL_MT];
    const float ls = pol_trunk<BF, A>(X, K0, nw, w1, (wave == 0 && net == 0) ? io.params + 2 * pol_net_floats<A>(K0) : nullptr, wave, lane, o);
    if (wave == 0) pol_act_sample<SQUASH>(io, p, o, ls, lane);
  }
  tile.finish(p, rq);
  pol_act_end(io, p);
}

// host side.  kernel_of(PolArch<..>{}): the act kernel's instantiation for that triple, `void (*)(PolActArgs<IO>)`; (h1, h2, h3) a
// listed triple (the caller has checked).  Above 64 KB of LDS a kernel must be told before its first launch:
template <class KernelOf>
hipError_t pol_act_prepare(int h1, int h2, int h3, size_t lds, KernelOf kernel_of) {
  if (lds <= 64 * 1024) return hipSuccess;
  hipError_t e = hipErrorInvalidValue;
  pol_arch_visit(h1, h2, h3, [&](auto a) {
    e = hipFuncSetAttribute((const void*)kernel_of(a), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  });
  return e;
}
// grid (ceil(ne / 16), 2), POL_THREADS
template <class IO, class KernelOf>
void pol_act_launch(int h1, int h2, int h3, const PolActArgs<IO>& pa, size_t lds, hipStream_t st, KernelOf kernel_of) {
  const dim3 grid((pa.ne + POL_ROWS - 1) / POL_ROWS, 2), block(POL_THREADS);
  pol_arch_visit(h1, h2, h3, [&](auto a) { hipLaunchKernelGGL(kernel_of(a), grid, block, lds, st, pa); });
}

// ---- the frame of an EVAL launch (k9_policy_eval, k17_squash_eval): grid (ceil(M / 16), nets launched), no environment, no
// rollout position, no counters, no sampling ----
struct EvalArgs {
  auv_policy_eval_t ev;
  int32_t net0;                      // blockIdx.y = 0 evaluates this net (0 policy, 1 value): only the nets asked for are launched
  int32_t vec2;                      // every source row starts 8-byte aligned and holds an even number of floats (host-proven)
};

// rows of a strided matrix, optionally gathered through ev.idx, -> the tile.  V = float2: ldx and obs_dim even and the base 8-byte
// aligned, so no pair straddles two rows or an 8-byte boundary
template <class V>
__device__ __forceinline__ void eval_fill_rows(float* X, const int ldx, const auv_policy_eval_t& ev, const int r0, const int rows, const int tid) {
  constexpr int W = sizeof(V) / sizeof(float);
  const int K0 = ev.obs_dim;
  const size_t lds = (size_t)ev.ldx;
  for (int i = W * tid; i < rows * K0; i += W * POL_THREADS) {
    const int row = i / K0, c = i - row * K0;
    const size_t srow = ev.idx ? (size_t)ev.idx[r0 + row] : (size_t)(r0 + row);
    *(V*)(X + row * ldx + c) = *(const V*)(ev.X + srow * lds + c);
  }
}

// The launch's body, written once for every hidden-width triple A (PolArch, auv_policy_mfma.h).  SQUASH: the deterministic action is
// act_mid + act_half * tanh(mu) (k17_squash_eval); mean, value and log pi(a) are the same either way.
template <class A, bool SQUASH = false>
__device__ __forceinline__ void policy_eval_body(const EvalArgs& ea) {
  extern __shared__ __align__(16) unsigned char smem[];
  const auv_policy_eval_t& ev = ea.ev;
  const int tid = threadIdx.x, wave = tid / AUV_WAVE, lane = tid % AUV_WAVE;
  const int net = ea.net0 + blockIdx.y;
  const int M = ev.M;
  const int r0 = blockIdx.x * POL_ROWS;                          // first row of the tile (M <= 2^31 - 1: no overflow)
  const int K0 = ev.obs_dim, K0p = pol_pad16(K0);
  float* X = (float*)smem;
  const int ldx = pol_ldx(K0);
  const PolNet nw = pol_net_ptrs<A>(ev.params + (size_t)net * pol_net_floats<A>(K0), K0);
  PolW<A::H1 / 16, false> w1;
  pol_prefetch(w1, nw.W1, nw.b1, K0p, wave, lane);                 // (in flight while the rows are fetched)
  // ---- the tile's rows -> LDS; padding columns and the rows past M stay zero ----
  const int rows = (M - r0 < POL_ROWS) ? M - r0 : POL_ROWS;
  pol_zero_tile(X, ldx, tid);
  __syncthreads();
  if (ea.vec2) eval_fill_rows<float2>(X, ldx, ev, r0, rows, tid);
  else eval_fill_rows<float>(X, ldx, ev, r0, rows, tid);
  const bool want_lp = ev.logp != nullptr;                       // (uniform)
  f32x4 o[1][POL_MT];
  const float ls = pol_trunk<false, A>(X, K0, nw, w1, (wave == 0 && net == 0 && want_lp) ? ev.params + 2 * pol_net_floats<A>(K0) : nullptr, wave, lane, o);
  if (wave != 0) return;
  const int n = lane & 15, g = lane >> 4;
  if (net == 0) {
    const float sigma = expf(ls);
    const auto map = pol_map_of<SQUASH>(ev, pol_comp(lane));
#pragma unroll
    for (int u = 0; u < POL_MT; u++)
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int rr = 16 * u + 4 * g + i;                       // row inside the tile
        const int row = r0 + rr;
        const bool live = n < 2 && rr < rows;
        const float mu = o[0][u][i];
        float lp = 0.0f;
        if (want_lp) {
          // log pi(a): the rollout launch's own function (the bits of LP[t] for the a the rollout stored)
          const float a = live ? ev.A[2 * (size_t)row + n] : mu;
          lp = pol_logp(a, mu, sigma, ls);
        }
        if (live) {
          if (ev.mu) ev.mu[2 * (size_t)row + n] = mu;
          if (ev.action) ev.action[(size_t)row * (size_t)ev.action_ld + n] = map(mu);
          if (want_lp && n == 0) ev.logp[row] = lp;
        }
      }
  } else if (n == 0) {
#pragma unroll
    for (int u = 0; u < POL_MT; u++)
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int rr = 16 * u + 4 * g + i;
        if (rr < rows) ev.value[r0 + rr] = o[0][u][i];
      }
  }
}

}  // namespace
#endif /* AUV_POLICY_FORWARD_H */
