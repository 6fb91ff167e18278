// K12 -- frame-stacked observations in the policy launch (auv_policy_act_stacked, auv_policy_rollout_stacked) and the same history
// update without a network (auv_stack_frames).  What stable-baselines ships as VecFrameStack (the reference trains with it,
// scripts/run.py:332-357): the last `frames` observations of an environment are ONE input row, so that a feed-forward policy sees how
// the obstacles move.
//
// k12_stacked_act<A> is k6_policy_act<A, false> with another input tile: both are pol_act_body (auv_policy_forward.h, which states the
// Tile contract), and this file holds only StackTile -- the history's step, the loader that reads the ring, the tagged store.  A row
// has frames * obs_dim columns; columns
// [j * obs_dim, (j + 1) * obs_dim) hold the observation of
// j steps ago, j = 0 the environment's observation buffer as it stands now, and zeros where the episode is younger than j steps
// (stable-baselines zeroes the stack at a reset).  NEWEST FIRST: a column permutation of stable-baselines' newest-last order, chosen so
// that the columns of frame 0 are the columns of the unstacked row.  For the same row and the same `params` the mean and the value have
// the bits auv_policy_eval gives on that row (tests/test_gpu_framestack.py).  frames == 1 touches no history at all: the input tile is
// filled by the function k6 calls (pol_act_fill_obs) and the launch is auv_policy_act bit for bit.
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
#include "auv_launch.h"
#include "auv_policy_forward.h"

namespace {

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
__host__ __device__ inline size_t stk_lds_bytes_h(int h1, int h2, int h3, int width) {
  return pol_lds_bytes_h(h1, h2, h3, width) + sizeof(int32_t) * 2 * POL_ROWS;
}

// the stacked tile: frame 0 from the observation buffer (and, `store`, into the ring's slot pos'), frame j >= 1 from the ring where
// the episode is old enough; every row also into dstO (nullable; O[t]'s rows of the tile are one contiguous range).  S: (pos', age')
// of the tile's rows; e_first: the environment of the tile's first row.  V = float2: obs_dim even, so rows and frames start 8-byte
// aligned and no pair straddles two frames.
template <class V>
__device__ __forceinline__ void stk_fill_ring(float* X, const int ldx, const auv_policy_stack_t& s, const int32_t* S, float* dstO,
                                              const int e_first, const int rows, const bool store, const int tid) {
  constexpr int W = sizeof(V) / sizeof(float);
  const int F = s.frames, D = s.io.obs_dim, K0 = F * D;
  for (int idx = W * tid; idx < rows * K0; idx += W * POL_THREADS) {
    const int row = idx / K0, c = idx - row * K0;
    const int j = c / D, cc = c - j * D;
    const size_t e = (size_t)(e_first + row);
    const int pos = S[2 * row], age = S[2 * row + 1];
    V v = {};
    if (j == 0) {
      v = *(const V*)(s.io.obs + e * D + cc);
    } else if (j < age) {
      const int slot = pos - j + (pos < j ? F : 0);
      v = *(const V*)(s.hist + (e * F + slot) * D + cc);
    }
    *(V*)(X + row * ldx + c) = v;
    if (dstO) *(V*)(dstO + idx) = v;
    if (j == 0 && store) *(V*)(s.hist + (e * F + pos) * D + cc) = v;
  }
}

// the stacked tile (Tile contract: auv_policy_forward.h): frames * obs_dim columns, (pos', age') of the tile's rows in LDS behind
// the tiles, the thread's own row's kept for the store at the end
struct StackTile : PolPlainTile {
  const auv_policy_stack_t& s;
  struct Req {
    bool keep = false;               // this thread stores its row's (pos', age') at the end
    int pos = 0, age = 0, tag;       // tag 1 .. 2^23 - 1: tag << 8 stays below 2^31, the word stays positive
    __device__ __forceinline__ explicit Req(const PolAct& p) : tag((int)(p.gstep % 0x7fffffull) + 1) {}
  };
  __device__ __forceinline__ explicit StackTile(const auv_policy_stack_t& s_) : PolPlainTile(s_.io), s(s_) {}
  __device__ __forceinline__ int width() const { return s.frames * io.obs_dim; }
  // the history's step of the tile's rows
  template <class A>
  __device__ __forceinline__ void request(A, Req& r, float* X, const PolAct& p, const int rows) const {
    const int F = s.frames, tid = threadIdx.x;
    int32_t* S = (int32_t*)pol_tiles_end<A>(X, width());           // [ROWS][2]: pos', age'
    if (F > 1 && tid < rows) {
      const int e = p.e0 + p.r0 + tid;
      const int2 w = *(const int2*)(s.stk + 2 * (size_t)e);
      const bool d = io.done_in[e] != 0;
      stk_advance(w, d, F, r.tag, r.pos, r.age);
      S[2 * tid] = r.pos, S[2 * tid + 1] = r.age;
      r.keep = blockIdx.y == 0;
    }
  }
  template <class A>
  __device__ __forceinline__ void fill(A, float* X, const PolAct& p, const Req&, const int rows) const {
    const int K0 = width(), ldx = pol_ldx(K0), tid = threadIdx.x;
    float* dstO = pol_act_obs_out(io, p, K0);
    const int32_t* S = (const int32_t*)pol_tiles_end<A>(X, K0);
    const bool store = blockIdx.y == 0;
    if (s.frames == 1) pol_act_fill_obs(X, io, p, dstO, rows);
    else if ((io.obs_dim & 1) == 0) stk_fill_ring<float2>(X, ldx, s, S, dstO, p.e0 + p.r0, rows, store, tid);
    else stk_fill_ring<float>(X, ldx, s, S, dstO, p.e0 + p.r0, rows, store, tid);
  }
  __device__ __forceinline__ void finish(const PolAct& p, const Req& r) const {
    if (r.keep) *(int2*)(s.stk + 2 * (size_t)(p.e0 + p.r0 + threadIdx.x)) = make_int2(r.pos | (r.tag << 8), r.age);
  }
};

// grid (ceil(ne / 16), 2): blockIdx.y = 0 the policy net, 1 the value net
template <class A>
__global__ void __launch_bounds__(POL_THREADS, (POL_WAVES >= 8 ? 4 : 2)) k12_stacked_act(PolActArgs<auv_policy_stack_t> pa) {   // (two workgroups per CU, as k6)
  pol_act_body<A, false, false>(pa, StackTile(pa.io));
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

// (h1, h2, h3): a listed hidden-width triple (the caller has checked)
size_t auv_policy_stacked_lds_bytes(int h1, int h2, int h3, int width) { return stk_lds_bytes_h(h1, h2, h3, width); }

static auto k12_act = [](auto a) { return k12_stacked_act<decltype(a)>; };

hipError_t auv_policy_stacked_prepare(int h1, int h2, int h3, int width) {
  return pol_act_prepare(h1, h2, h3, stk_lds_bytes_h(h1, h2, h3, width), k12_act);
}

void auv_launch_policy_stacked(int h1, int h2, int h3, const auv_policy_stack_t& s, int e0, int ne, hipStream_t st, long long t_host,
                               long long gstep_host) {
  const PolActArgs<auv_policy_stack_t> pa = {s, e0, ne, t_host, gstep_host};
  pol_act_launch(h1, h2, h3, pa, stk_lds_bytes_h(h1, h2, h3, s.frames * s.io.obs_dim), st, k12_act);
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
