// K12 -- frame-stacked observations in the policy launch (auv_policy_act_stacked, auv_policy_rollout_stacked) and the same history
// update without a network (auv_stack_frames).  What stable-baselines ships as VecFrameStack (the reference trains with it,
// scripts/run.py:332-357): the last `frames` observations of an environment are ONE input row, so that a feed-forward policy sees how
// the obstacles move.
//
// k12_stacked_act IS k6_policy_act's exact-f32 path -- the same workgroup (16 rows of ONE net, eight waves), the same LDS tiles and
// row strides, pol_prefetch / pol_layer in the same order with the same template arguments, the same epilogue expressions (sampling
// from (seed, generator step, environment), log pi, clip, action map, R[t - 1] / Dn[t - 1] of the step just completed) -- with one
// difference: the input tile.  A row has frames * obs_dim columns; columns [j * obs_dim, (j + 1) * obs_dim) hold the observation of
// j steps ago, j = 0 the environment's observation buffer as it stands now, and zeros where the episode is younger than j steps
// (stable-baselines zeroes the stack at a reset).  NEWEST FIRST: a column permutation of stable-baselines' newest-last order, chosen so
// that the columns of frame 0 are the columns of the unstacked row.  For the same row and the same `params` the mean and the value have
// the bits auv_policy_eval gives on that row (tests/test_gpu_framestack.py).  frames == 1 touches no history at all: the input tile is
// filled by k6's own loop and the launch is auv_policy_act bit for bit.
//
// State per environment, on the device (so the launch can sit in a captured graph): a ring hist[N][frames][obs_dim] and
// stk[N][2] = (pos | tag << 8, age) -- pos the ring slot of the newest frame, age the number of valid frames (0 after a reset of the
// stack, at most `frames`).  An act launch forms  age' = min((done_in ? 0 : age) + 1, frames),  pos' = (pos + 1) mod frames,  reads
// frame j >= 1 from slot (pos' - j) mod frames if j < age', and then stores hist[pos'] = obs, stk = (pos', age').
//
// Ordering.  A tile's rows are read by TWO workgroups of a launch -- blockIdx.y = 0 the policy net, 1 the value net -- and both need
// the state as it stood BEFORE the launch; only the policy workgroup stores (hist, stk, O).  Nothing orders the two, so the value
// workgroup may read stk after its sibling has moved it on.  The tag tells it: every act launch of a chain has its own generator step,
// the policy workgroup stores tag = (generator step mod (2^23 - 1)) + 1 next to pos -- 1 .. 2^23 - 1, so that tag << 8 never reaches
// the sign bit and the word stays positive -- and a workgroup that finds its OWN launch's tag there takes (pos, age) as the
// (pos', age') they already are.  Launches that follow each other on a chain must therefore have different generator steps, mod
// 2^23 - 1: the counters of auv_policy_act and the t0 / gstep0 contract of the rollout call see to that, and a launch REPLAYED with
// the generator step of the one before it finds its own tag and does not move the history (include/auv_hip.h says so).
// auv_stack_frames and a reset of the stack store tag 0, which no launch has.
// The ring needs no more than program order: the slot written is pos', the slots read are (pos' - j) mod frames with 1 <= j <= frames - 1 -- never pos' -- in this workgroup and in its sibling alike, and obs,
// done_in are written by nobody in this launch.  Within the policy workgroup the state is requested ahead of the barrier behind the
// tile's zeroing, stk and the transition are stored at the very end (k6's rule: requests first, stores last).
// The flush launch (t == T) stores R[T - 1] / Dn[T - 1] only: hist and stk stay as they are, so the next rollout's first launch, which
// sees the same obs and done_in, adds that frame exactly once.
#include "auv_policy_mfma.h"

namespace {

struct StackArgs {
  auv_policy_stack_t s;
  int32_t e0, ne;
  long long t_host, gstep_host;      // as k6's PolicyArgs: >= 0 the host names position and generator step, -1 they live in io.ctr
};

// splitmix64 finaliser and the Gaussian of (seed, step, row, component): k6_policy.hip's pol_mix / pol_gauss, expression by expression
__device__ __forceinline__ unsigned long long stk_mix(unsigned long long z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ float stk_gauss(unsigned long long seed, unsigned long long step, unsigned int row, unsigned int comp) {
  const unsigned long long h = stk_mix(stk_mix(seed ^ (step * 0xd1342543de82ef95ull)) ^ (((unsigned long long)row << 1) | comp));
  const float u1 = ((float)(unsigned int)(h >> 40) + 0.5f) * (1.0f / 16777216.0f);      // (0, 1): 24 bits
  const float u2 = ((float)(unsigned int)((h >> 8) & 0xffffffu)) * (1.0f / 16777216.0f);   // [0, 1)
  return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}

// the history's step for one environment: (pos, age) -> (pos', age')
__device__ __forceinline__ void stk_advance(const int2 s, const bool done, const int F, const int tag, int& pos, int& age) {
  if (tag != 0 && (int)((unsigned int)s.x >> 8) == tag) {        // this launch's sibling workgroup has stored them already
    pos = s.x & 255, age = s.y;
    return;
  }
  const int a = (done ? 0 : s.y) + 1;
  age = a < F ? a : F;
  pos = (s.x & 255) + 1;
  if (pos >= F) pos = 0;
}

// LDS: k6's tiles for frames * obs_dim columns, and behind them (pos', age') of the tile's 16 rows
__host__ __device__ inline size_t stk_lds_bytes(int width) { return pol_lds_bytes(width) + sizeof(int32_t) * 2 * POL_ROWS; }

// grid (ceil(ne / 16), 2): blockIdx.y = 0 the policy net, 1 the value net.
__global__ void __launch_bounds__(POL_THREADS, (POL_WAVES >= 8 ? 4 : 2)) k12_stacked_act(StackArgs pa) {   // (two workgroups per CU, as k6)
  extern __shared__ __align__(16) unsigned char smem[];
  const auv_policy_io_t& io = pa.s.io;
  const int tid = threadIdx.x, wave = tid / AUV_WAVE, lane = tid % AUV_WAVE;
  const int net = blockIdx.y;
  const int r0 = blockIdx.x * POL_ROWS;                          // first row of the tile inside the slice
  const int F = pa.s.frames, D = io.obs_dim;
  const int K0 = F * D, K0p = pol_pad16(K0);                     // the net's input width
  const int ldx = K0p + 8, ld1 = POL_H1 + 8, ld2 = POL_H2 + 8, ld3 = POL_H3 + 8;
  float* X = (float*)smem;
  float* Y1 = X + pol_lds_x_floats(K0);
  float* Y2 = X;                                                 // (X is dead once layer 1 is through: a barrier lies in between)
  float* Y3 = Y1;                                                // (Y1 is dead once layer 2 is through)
  int32_t* S = (int32_t*)(Y1 + (size_t)POL_ROWS * ld1);          // [ROWS][2]: pos', age'
  // position in the rollout and the generator's step counter: read by every workgroup before anybody moves them on
  const bool host_counts = pa.t_host >= 0;
  const long long t = host_counts ? pa.t_host : io.ctr[0];
  const unsigned long long gstep = (unsigned long long)(host_counts ? pa.gstep_host : io.ctr[1]);
  const int T = io.T;
  const int cnt = pa.ne;
  const size_t ld = (size_t)io.ld;                               // environments per rollout row
  const int col0 = pa.e0 - io.env_base + r0;                     // the tile's first column in a rollout row
  // ---- the transition the environment's last step completed: reward and done of step t - 1 (requested here, stored at the end) ----
  const bool trans = net == 0 && t >= 1 && t <= T && tid < POL_ROWS && r0 + tid < cnt;
  float trans_r = 0.0f;
  uint8_t trans_d = 0;
  if (trans) trans_r = io.reward_in[pa.e0 + r0 + tid], trans_d = io.done_in[pa.e0 + r0 + tid];
  const bool act = t < T;                                        // t == T: the flush call after a rollout's last step
  const int tag = (int)(gstep % 0x7fffffull) + 1;                // 1 .. 2^23 - 1: tag << 8 stays below 2^31, the word stays positive
  bool keep = false;                                             // this thread stores its row's (pos', age') at the end
  int my_pos = 0, my_age = 0;
  if (act) {
    const float* P = io.params + (size_t)net * pol_net_floats(K0);
    const float* W1 = P;
    const float* b1 = W1 + (size_t)POL_H1 * K0p;
    const float* W2 = b1 + POL_H1;
    const float* b2 = W2 + (size_t)POL_H2 * POL_H1;
    const float* W3 = b2 + POL_H2;
    const float* b3 = W3 + (size_t)POL_H3 * POL_H2;
    const float* W4 = b3 + POL_H3;
    const float* b4 = W4 + (size_t)POL_OUT * POL_H3;
    PolW<POL_H1 / 16, false> w1;
    PolW<POL_H2 / 16, false> w2;
    PolW<POL_H3 / 16, false> w3;
    PolW<1, false> w4;
    pol_prefetch(w1, W1, b1, K0p, wave, lane);                     // (in flight while the tile is formed)
    const int rows = (cnt - r0 < POL_ROWS) ? cnt - r0 : POL_ROWS;
    // ---- the history's step of the tile's rows: requested ahead of the barrier behind the zeroing ----
    if (F > 1 && tid < rows) {
      const int e = pa.e0 + r0 + tid;
      const int2 s = *(const int2*)(pa.s.stk + 2 * (size_t)e);
      const bool d = io.done_in[e] != 0;
      stk_advance(s, d, F, tag, my_pos, my_age);
      S[2 * tid] = my_pos, S[2 * tid + 1] = my_age;
      keep = net == 0;
    }
    // ---- input tile -> LDS (zero padded), and into the rollout (policy workgroup) ----
    for (int idx = tid; idx < POL_ROWS * (ldx / 2); idx += POL_THREADS) *(float2*)(X + 2 * idx) = make_float2(0.0f, 0.0f);
    __syncthreads();
    float* dstO = (net == 0 && io.O) ? io.O + ((size_t)t * ld + col0) * K0 : nullptr;
    if (F == 1) {
      // k6's own loop: the tile's rows are one contiguous range of the observation buffer
      const float* src = io.obs + (size_t)(pa.e0 + r0) * K0;
      if ((K0 & 1) == 0) {
        for (int idx = 2 * tid; idx < rows * K0; idx += 2 * POL_THREADS) {
          const float2 v = *(const float2*)(src + idx);
          const int row = idx / K0, c = idx - row * K0;
          *(float2*)(X + row * ldx + c) = v;
          if (dstO) *(float2*)(dstO + idx) = v;
        }
      } else {
        for (int idx = tid; idx < rows * K0; idx += POL_THREADS) {
          const float v = src[idx];
          const int row = idx / K0, c = idx - row * K0;
          X[row * ldx + c] = v;
          if (dstO) dstO[idx] = v;
        }
      }
    } else if ((D & 1) == 0) {
      // two floats per lane: obs_dim even, so rows and frames start 8-byte aligned and no pair straddles two frames
      for (int idx = 2 * tid; idx < rows * K0; idx += 2 * POL_THREADS) {
        const int row = idx / K0, c = idx - row * K0;
        const int j = c / D, cc = c - j * D;
        const size_t e = (size_t)(pa.e0 + r0 + row);
        const int pos = S[2 * row], age = S[2 * row + 1];
        float2 v = make_float2(0.0f, 0.0f);
        if (j == 0) {
          v = *(const float2*)(io.obs + e * D + cc);
        } else if (j < age) {
          const int slot = pos - j + (pos < j ? F : 0);
          v = *(const float2*)(pa.s.hist + (e * F + slot) * D + cc);
        }
        *(float2*)(X + row * ldx + c) = v;
        if (dstO) *(float2*)(dstO + idx) = v;                    // (O[t]'s rows of the tile are one contiguous range)
        if (j == 0 && net == 0) *(float2*)(pa.s.hist + (e * F + pos) * D + cc) = v;
      }
    } else {
      for (int idx = tid; idx < rows * K0; idx += POL_THREADS) {
        const int row = idx / K0, c = idx - row * K0;
        const int j = c / D, cc = c - j * D;
        const size_t e = (size_t)(pa.e0 + r0 + row);
        const int pos = S[2 * row], age = S[2 * row + 1];
        float v = 0.0f;
        if (j == 0) {
          v = io.obs[e * D + cc];
        } else if (j < age) {
          const int slot = pos - j + (pos < j ? F : 0);
          v = pa.s.hist[(e * F + slot) * D + cc];
        }
        X[row * ldx + c] = v;
        if (dstO) dstO[idx] = v;
        if (j == 0 && net == 0) pa.s.hist[(e * F + pos) * D + cc] = v;
      }
    }
    __syncthreads();
    pol_prefetch(w2, W2, b2, POL_H1, wave, lane);                    // (the next layer's weights: in flight during this layer)
    pol_layer<POL_H1 / 16, 1, false, false>(X, ldx, w1, b1, K0p, wave, lane, Y1, ld1, nullptr);
    __syncthreads();
    pol_prefetch(w3, W3, b3, POL_H2, wave, lane);
    pol_layer<POL_H2 / 16, 1, false, false>(Y1, ld1, w2, b2, POL_H1, wave, lane, Y2, ld2, nullptr);
    __syncthreads();
    pol_prefetch(w4, W4, b4, POL_H3, wave, lane);
    // (the sampling's log-std with them: ahead of the barrier, so that the request is not moved down to its use)
    const int nc = (lane & 15) < 2 ? (lane & 15) : 0;
    float ls = 0.0f;
    if (wave == 0 && net == 0) ls = (io.params + 2 * pol_net_floats(K0))[nc];
    pol_layer<POL_H3 / 16, 2, false, false>(Y2, ld2, w3, b3, POL_H2, wave, lane, Y3, ld3, nullptr);
    __syncthreads();
    if (wave == 0) {
      f32x4 o[1][POL_MT];
      pol_layer<1, 2, true, false>(Y3, ld3, w4, b4, POL_H3, 0, lane, nullptr, 0, o);
      const int n = lane & 15, g = lane >> 4;
      if (net == 0) {
        // ---- diagonal Gaussian: sample, log-probability, action (k6's epilogue) ----
        const float sigma = expf(ls);
        float cl0 = io.clip_lo[0], cl1 = io.clip_lo[1], ch0 = io.clip_hi[0], ch1 = io.clip_hi[1];
        float am0 = io.act_mid[0], am1 = io.act_mid[1], ah0 = io.act_half[0], ah1 = io.act_half[1];
        asm volatile("" : "+s"(cl0), "+s"(cl1), "+s"(ch0), "+s"(ch1), "+s"(am0), "+s"(am1), "+s"(ah0), "+s"(ah1));   // (or the selects become indexed loads)
        const float clip_lo = nc ? cl1 : cl0, clip_hi = nc ? ch1 : ch0, act_mid = nc ? am1 : am0, act_half = nc ? ah1 : ah0;
#pragma unroll
        for (int u = 0; u < POL_MT; u++)
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int rr = 16 * u + 4 * g + i;                   // row inside the tile
            const int row = r0 + rr;
            const int e = pa.e0 + row;
            const float mu = o[0][u][i];
            const float eps = stk_gauss(io.seed, gstep, (unsigned int)e, (unsigned int)nc);
            const float a = mu + sigma * eps;
            const float z = (a - mu) / sigma;
            float lp = -0.5f * z * z - ls - POL_LOG_SQRT_2PI;
            lp += __shfl_xor(lp, 1, AUV_WAVE);                   // the two components sit on neighbouring lanes
            if (n < 2 && row < cnt) {
              const size_t q = (size_t)t * ld + col0 + rr;
              io.A[2 * q + n] = a;
              if (n == 0) io.LP[q] = lp;
              const float ac = fminf(fmaxf(a, clip_lo), clip_hi);
              io.actions_out[2 * (size_t)e + n] = act_mid + act_half * ac;
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
            if (r0 + rr < cnt) io.V[(size_t)t * ld + col0 + rr] = o[0][u][i];
          }
      }
    }
  }
  if (keep) *(int2*)(pa.s.stk + 2 * (size_t)(pa.e0 + r0 + tid)) = make_int2(my_pos | (tag << 8), my_age);
  if (trans) {
    float r = trans_r;
    if (io.reward_clip > 0.0f) r = fminf(fmaxf(r, -io.reward_clip), io.reward_clip);
    io.R[(size_t)(t - 1) * ld + col0 + tid] = r * io.reward_scale;
    io.Dn[(size_t)(t - 1) * ld + col0 + tid] = trans_d ? 1.0f : 0.0f;
  }
  // ---- the rollout position and the generator's counter move on (k6's two ways) ----
  if (host_counts) {
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
      if (t <= T) io.ctr[0] = t + 1;
      io.ctr[1] = (long long)(gstep + 1);
    }
    return;
  }
  __syncthreads();
  if (tid == 0) {
    const unsigned long long total = (unsigned long long)gridDim.x * gridDim.y;
    const unsigned long long old = atomicAdd((unsigned long long*)&io.ctr[2], 1ull);
    if (old == total - 1) {
      io.ctr[2] = 0;
      if (t <= T) io.ctr[0] = t + 1;                             // (a flush call leaves T + 1: further calls do nothing)
      io.ctr[1] = (long long)(gstep + 1);
    }
  }
}

// ---- the history update alone: stacked rows out[ne][ldx] of environments [e0, e0 + ne), no network ----
// One workgroup owns STK_ROWS environments: their state goes to LDS ahead of a barrier, every frame is copied V floats per lane (V = 4:
// 16-byte accesses, where obs_dim, ldx and the bases allow), and the state is stored behind the copies.  advance == 0 is a peek: the row
// the next act launch would form, and nothing is stored to hist or stk.
#define STK_ROWS 8
#define STK_THREADS 256

struct FramesArgs {
  const float* obs;
  const uint8_t* done;               // nullable: no environment is done
  float* hist;
  int32_t* stk;
  float* out;
  long long ldx;
  int32_t e0, ne, D, F, advance;
};

template <int V>
struct StkVec;
template <>
struct StkVec<1> { typedef float type; };
template <>
struct StkVec<2> { typedef float2 type; };
template <>
struct StkVec<4> { typedef float4 type; };

template <int V>
__global__ void __launch_bounds__(STK_THREADS) k12_stack_frames(FramesArgs fa) {
  typedef typename StkVec<V>::type vec;
  __shared__ int32_t S[2 * STK_ROWS];
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * STK_ROWS;
  const int rows = (fa.ne - r0 < STK_ROWS) ? fa.ne - r0 : STK_ROWS;
  const int F = fa.F, D = fa.D, K0 = F * D;
  int my_pos = 0, my_age = 0;
  const bool mine = F > 1 && tid < rows;
  if (mine) {
    const int e = fa.e0 + r0 + tid;
    const int2 s = *(const int2*)(fa.stk + 2 * (size_t)e);
    const bool d = fa.done ? fa.done[e] != 0 : false;
    stk_advance(s, d, F, 0, my_pos, my_age);
    S[2 * tid] = my_pos, S[2 * tid + 1] = my_age;
  }
  __syncthreads();
  const vec zero = {};
  for (int idx = V * tid; idx < rows * K0; idx += V * STK_THREADS) {
    const int row = idx / K0, c = idx - row * K0;
    const int j = c / D, cc = c - j * D;
    const size_t e = (size_t)(fa.e0 + r0 + row);
    vec v = zero;
    int pos = 0;
    if (j == 0) {
      v = *(const vec*)(fa.obs + e * D + cc);
      if (F > 1) pos = S[2 * row];
    } else {
      pos = S[2 * row];
      if (j < S[2 * row + 1]) {
        const int slot = pos - j + (pos < j ? F : 0);
        v = *(const vec*)(fa.hist + (e * F + slot) * D + cc);
      }
    }
    *(vec*)(fa.out + (size_t)(r0 + row) * (size_t)fa.ldx + c) = v;
    if (j == 0 && F > 1 && fa.advance) *(vec*)(fa.hist + (e * F + pos) * D + cc) = v;
  }
  if (mine && fa.advance) *(int2*)(fa.stk + 2 * (size_t)(fa.e0 + r0 + tid)) = make_int2(my_pos, my_age);
}

}  // namespace

size_t auv_policy_stacked_lds_bytes(int width) { return stk_lds_bytes(width); }

hipError_t auv_policy_stacked_prepare(int width) {
  const size_t b = stk_lds_bytes(width);
  if (b <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute((const void*)k12_stacked_act, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
}

void auv_launch_policy_stacked(const auv_policy_stack_t& s, int e0, int ne, hipStream_t st, long long t_host, long long gstep_host) {
  StackArgs pa;
  pa.s = s, pa.e0 = e0, pa.ne = ne;
  pa.t_host = t_host, pa.gstep_host = gstep_host;
  const dim3 grid((ne + POL_ROWS - 1) / POL_ROWS, 2), block(POL_THREADS);
  hipLaunchKernelGGL(k12_stacked_act, grid, block, stk_lds_bytes(s.frames * s.io.obs_dim), st, pa);
}

void auv_launch_stack_frames(const float* obs, const uint8_t* done, float* hist, int32_t* stk, float* out, long long ldx, int e0, int ne,
                             int obs_dim, int frames, int advance, hipStream_t st) {
  FramesArgs fa;
  fa.obs = obs, fa.done = done, fa.hist = hist, fa.stk = stk, fa.out = out, fa.ldx = ldx;
  fa.e0 = e0, fa.ne = ne, fa.D = obs_dim, fa.F = frames, fa.advance = advance;
  const uintptr_t bases = (uintptr_t)obs | (uintptr_t)hist | (uintptr_t)out;
  const dim3 grid((ne + STK_ROWS - 1) / STK_ROWS), block(STK_THREADS);
  if ((obs_dim & 3) == 0 && (ldx & 3) == 0 && (bases & 15) == 0) hipLaunchKernelGGL(k12_stack_frames<4>, grid, block, 0, st, fa);
  else if ((obs_dim & 1) == 0 && (ldx & 1) == 0 && (bases & 7) == 0) hipLaunchKernelGGL(k12_stack_frames<2>, grid, block, 0, st, fa);
  else hipLaunchKernelGGL(k12_stack_frames<1>, grid, block, 0, st, fa);
}
