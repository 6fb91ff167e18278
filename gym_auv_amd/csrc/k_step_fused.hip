// k_step_fused.hip -- the launch shapes of step() that put more than one phase into a launch, built from the very
// same device functions as the individually launchable kernels (k1_dynamics / k2_lidar / k3_nav / k3_reward), so the
// per-kernel parity tests cover their arithmetic and tests/test_gpu_parity.py pins the compositions bit for bit:
//   k_step_roles            ONE launch per step: dynamics, LiDAR sweep, navigation search, tail + reward as four roles
//   k23_lidar_nav           K2 and K3-nav side by side in one launch (the fence-free three-launch shape)
//   k31_reward_dyn          inside a captured graph of several steps: reward phase of step t + dynamics of step t + 1
// Every launch covers the slice [e0, e0 + ne) of the handle's environments (AuvDev::e0 / ne; the whole batch by
// default): sub-batches of one handle stepped on different streams overlap each other's head and tail.
// (Measured and removed in round 3, numbers in DESIGN.md: the whole step as one wave per environment, 66.9 M
// env-steps/s; [K1 + navigation] -> [LiDAR + reward], 73.6 M; navigation forked onto a second stream, 64.5 M; K1 ->
// [LiDAR | navigation + reward] ("paired"), 98 M; the navigation's tail + reward with lanes <-> environments as a
// second launch, 106-112 M against 133 M with four sub-batch chains; the one-launch step with the navigation WAVE of an
// environment also running its tail and its reward phase -- three roles -- was the shape until late in round 3: 19 %
// more VALU issue cycles than the four roles below, 130 M against 136 M in the same sweep -- git history and
// profiles/r03/shapes_sweep*.log.)
#include <cstdlib>
#include <hip/hip_ext.h>

#define AUV_DEVICE_FUNCS_ONLY
#include "auv_launch.h"
#include "auv_multi_geom.h"
#include "k1_dynamics.hip"
#include "k2_lidar.hip"
#include "k3_nav_reward.hip"

#ifndef AUV_K23_MIN_WAVES
#define AUV_K23_MIN_WAVES 4   // waves per SIMD the LiDAR launches are compiled for (128 VGPRs)
#endif

// Test hooks (tests/test_gpu_parity.py) exist only in the library built with -DAUV_TEST_HOOKS (make hooks ->
// libauv_hip_hooks.so): idle workgroups between the roles (puts an environment's waves on different XCDs) and a
// hand-over that never happens for the first environment of the launch (fault 1: its sweep withholds the word; 2: the
// dynamics role withholds its state packet; 3: its search withholds the record) -- the polls must run out and fail
// loudly.  The shipped library has neither.
#ifdef AUV_TEST_HOOKS
#define AUV_HOOK_SKEW(d) ((d).pair_skew)
#define AUV_HOOK_FAULT(d) ((d).pair_fault)
#else
#define AUV_HOOK_SKEW(d) 0
#define AUV_HOOK_FAULT(d) 0
#endif

namespace {

// ---- the in-launch hand-over of the sweep's result -------------------------------------------------------------
// An environment's LiDAR wave and the finish wave that runs its reward phase (rewarder.py:78-140, :167-241;
// environment.py:333-347, :375-384) are workgroups of the same launch -- no third launch.  What the reward phase needs
// of the sweep is one 64-bit word per environment (the LiDAR term of the reward, or a marker for "collision"): the
// LiDAR wave stores it last, the finish wave polls for it, consumes it and puts the "empty" marker back.
//   Coherence without device-scope fences (their L2 write-back per wave is what made round 1's attempt 5x slower):
//   * the word goes by relaxed agent-scope atomic store / load (sc1: written through and read past the XCD's
//     L2, which is not coherent with the other seven);
//   * every row the LiDAR wave writes is stored write-through too (WT = true in k2_front / k2_back), and the wave
//     waits for the completion of all its stores before it stores the word.  A finish wave that has seen the
//     word therefore knows that nothing of that environment is in flight or dirty in another L2: its plain stores
//     (reward phase; restore_env, which overwrites the sweep's rows when the episode ended) are the last word
//     whichever XCDs the two ran on.  Rows of other environments share cache lines but not bytes.
//   * the launch places all waves of an environment on the same XCD (workgroups go round-robin over the eight XCDs;
//     every role starts at a multiple of 8 and the dynamics / finish waves take the environments of their own
//     XCD), which keeps the words in one L2; correctness does not depend on it (tests run with the roles skewed
//     onto different XCDs).
//     (Plain stores for the sweep's rows -- complete when the XCD's own L2 has them, which is enough when the
//     finish wave runs on the same XCD -- were measured: +0.6 % with four chains, +1.3 % with one; not worth making
//     correctness depend on the workgroup -> XCD mapping.)
//   * whoever polls, polls for a word of a workgroup with a SMALLER index in the same launch: that one was
//     dispatched earlier and finishes without needing anything from a later one.  The polls are bounded all the
//     same: when one runs out the wave reports through `pair_error` (the next call recovers and reports) instead
//     of hanging the device.
#define PAIR_EMPTY AUV_PAIR_EMPTY
#define PAIR_COLLISION AUV_PAIR_COLLISION
#define PAIR_POLL_LIMIT (1 << 22)
#ifndef ROLES_POLL_SLEEP
#define ROLES_POLL_SLEEP 8          // 64-cycle quanta between two looks at a hand-over word (2, 4 and 16 measured in round 4: no difference, profiles/r04/ab_poll_sleep.jsonl)
#endif
#define ROLES_ABORT_COUNTER 0xffffffffu   // step-counter word of an ABORT packet (a real Vessel._step_counter never gets there)

// A poll has run out.  The wave records which environments it leaves unfinished (`broken`: the caller does, per
// environment), raises the device-wide abort flag -- launches queued behind this one then do nothing instead of consuming
// half-finished hand-overs -- and tells the host (mapped memory: code, and the slice of the launch that reports).
__device__ __forceinline__ void roles_give_up(const AuvDev& d, const int e0, const int ne, const int code, const int lane) {
  if (lane == 0) {
    __hip_atomic_store(d.abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(d.abort_flag + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // "a report is out": a rendezvous kernel that runs out later keeps its code to itself (k_rdv_wait)
    __hip_atomic_store(d.pair_error + 1, e0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(d.pair_error + 2, ne, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(d.pair_error, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

__device__ __forceinline__ void pair_publish_lidar(const AuvDev& d, const int e, const int lane, const int collision,
                                                   const double term) {
  auv_stores_done();                                       // of every lane of this wave (one counter per wave)
  if (AUV_HOOK_FAULT(d) == 1 && e == d.e0) return;         // (test hook: the poll's time-out)
  if (lane == 0)
    __hip_atomic_store(d.pair_word + e, collision ? PAIR_COLLISION : (unsigned long long)__double_as_longlong(term),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// K2 and K3-nav of the launch's environments in one launch of one-wave workgroups: workgroups [0, ne) sweep the LiDAR
// of their environments, workgroups [ne, 2 ne) navigate theirs.  The two are independent given the new vessel state,
// so they run side by side (the LiDAR workgroups are dispatched first and fill the chip; navigation workgroups move
// in as those retire; a wave slot is handed on the moment an environment's sweep ends) -- the concurrency of two
// streams without the ~8 us a cross-stream event wait costs on each side.  Nothing is handed over inside the launch.
__global__ void __launch_bounds__(AUV_BLOCK, AUV_K23_MIN_WAVES) k23_lidar_nav(AuvDev dk, float* __restrict__ obs_out) {
  // (every table through the device-side copy AuvDev::self instead of the kernel arguments -- no scalar register
  // spilled any more -- was tried for the whole kernel: the loads then sit on the dependent chains, 36.3 -> 42.2 us)
  const AuvDev& d = dk;
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x;
  const int ne = d.ne;
  if ((int)blockIdx.x >= ne) {
    const int el = (int)blockIdx.x - ne;
    if (el >= ne) return;
    const int e = auv_uniform(d.e0 + el);
#ifdef AUV_STAMPS
    const unsigned long long t_nav0 = wall_clock64();
#endif
    k3_nav_env(d, e, lane, smem, obs_out);
#ifdef AUV_STAMPS
    if (lane == 0) d.stamps[(size_t)e * 16 + 12] = t_nav0, d.stamps[(size_t)e * 16 + 13] = wall_clock64();
#endif
  } else {
    const int e = auv_uniform(d.e0 + (int)blockIdx.x);
    // next action slot of a captured graph's ring: the dynamics kernel of this step has read the position, the
    // one of the next step has not been launched yet.  The first environment of the LAUNCH advances it: a captured chain
    // covers a slice [e0, e0 + ne) and keeps a ring position of its own (`e == 0` left the chains with e0 > 0
    // on slot 0 for good when a captured chain stepped in this shape)
    if (e == d.e0 && lane == 0 && dk.ring_slots > 1 && dk.ring_slot_host == -1) *dk.ring_pos = (*dk.ring_pos + 1) % dk.ring_slots;
    const Slice L = carve(smem, d);
    AUV_STAMP_DECL
#ifdef AUV_STAMPS
    const unsigned long long t_real0 = wall_clock64();
#endif
    int2 lim0 = make_int2(INT32_MIN, INT32_MIN);           // this lane's cull-limit row: stored by k2_back (see there)
    const int n_act = k2_front(d, e, lane, L, 1, nullptr, 0, nullptr, false, d.cfg.use_lidar ? &lim0 : nullptr);
    if (d.cfg.use_lidar) {
      AUV_STAMP()
#ifdef AUV_STAMPS
      unsigned long long sub[4] = {0, 0, 0, 0};
      k2_stage_and_pairs(d, L, lane, n_act, d.state[2 * (size_t)d.n + e], sub);
      if (lane == 0) d.stamps[(size_t)e * 16 + 7] = sub[0], d.stamps[(size_t)e * 16 + 14] = sub[1], d.stamps[(size_t)e * 16 + 15] = sub[2], d.stamps[(size_t)e * 16 + 6] = sub[3];
#else
      k2_stage_and_pairs(d, L, lane, n_act, d.state[2 * (size_t)d.n + e]);
#endif
      AUV_STAMP()
      double term = 0.0;
      k2_back(d, e, lane, L, n_act, obs_out, &term, &lim0);
      AUV_STAMP()
      AUV_STAMP_FLUSH(e, 0)   // 0: front (A, C, B, S)  1: pairs (D)  2: back (E)
#ifdef AUV_STAMPS
      if (lane == 0) d.stamps[(size_t)e * 16 + 3] = t_real0, d.stamps[(size_t)e * 16 + 4] = wall_clock64();
      if (lane == 0) d.stamps[(size_t)e * 16 + 5] = (unsigned long long)L.sbase[n_act];
#endif
    }
  }
}

// ---- ONE launch per step: four roles --------------------------------------------------------------
// k_step_roles   workgroups [0, nk) integrate the dynamics (Vessel.step, one wave = eight environments, eight lanes
//                each: k1_group); workgroups [nk, nk + nb) sweep the LiDAR of one environment each; workgroups
//                [nk + nb, nk + 2 nb) search the nearest point of the path for one environment each (the wide part of
//                Vessel.navigate); the last nk workgroups -- the finish role, eight environments per wave like the
//                dynamics -- evaluate the navigation's scalar tail and run the reward phase (see there).
//                The sweep, the search and the finish need the state the dynamics role produces in the same launch:
//                it hands each environment a 64-byte packet (x, y, psi, u, v, r, the vessel's step counter, a "ready"
//                mark that is also a checksum of the rest), written through (sc1) by ONE store instruction -- and that
//                is all the dynamics role stores: the STATE rows and the vessel's step counter are written from the
//                packet by the finish wave.  The other roles poll for a mark that matches the payload (the dynamics
//                workgroups have the smallest indices, are dispatched first and wait for nobody; every poll is
//                bounded).  The search leaves its result in a record of the same kind (NAV_HAND), the sweep its word.  The finish wave takes all three marks away again when it
//                has finished the environment's step (the environment's other waves are gone by then: it has seen
//                what each of them stores last), so the next launch finds every mark down.  What is saved against
//                separate launches is the launch ramps and the kernel boundaries between them.  No launch argument
//                changes from step to step, so the shape can be captured in a hipGraph; there the dynamics waves
//                count themselves off and the last one advances the action ring (every one of them has read the
//                position by then).
// (Tried and dropped: the sweep waves also running the navigation's search over the chunk circles for the old pose
// while they wait, handing the survivor list to the navigation wave in one word -- the navigation wave gets 2.5 us
// shorter, but the extra traffic and issue slots stretch the dynamics role's chain from 6 to 7.5 us and the whole
// launch waits for that: 98.4 M against 101.9 M env-steps/s.)
// Dynamics wave b takes the environments 8 (8 (b / 8) + g) + b % 8, g = 0..7: the ones whose other two waves run on
// its own XCD (all three counts are multiples of 8), so the packets stay in one L2.
__device__ __forceinline__ double pair_lane_value(const unsigned long long v, const int src) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// The packet's eighth word is its "ready" mark AND a checksum of the other seven: (xor of words 0..6, xor a constant)
// with bit 0 set; "down" is 0.  A reader accepts the payload only if the mark it loaded WITH it matches the payload,
// so a request served in pieces (new mark, old state) can never pass -- the hand-over does not rest on the 64-byte
// request being served atomically, and costs the reader a few scalar instructions, no second trip.
#define ROLES_MAGIC 0x9e3779b97f4a7c15ull
__device__ __forceinline__ unsigned long long roles_mark(const unsigned long long x) { return (x ^ ROLES_MAGIC) | 1ull; }

// xor of `w` over the eight lanes of the caller's group (lanes 8 g .. 8 g + 7), by DPP moves: quad_perm [1,0,3,2],
// quad_perm [2,3,0,1], row_half_mirror -- no LDS, a dozen VALU instructions at the end of the dynamics' chain
__device__ __forceinline__ unsigned long long roles_group_xor(const unsigned long long w) {
  int lo = (int)(unsigned)w, hi = (int)(unsigned)(w >> 32);
  lo ^= __builtin_amdgcn_update_dpp(0, lo, 0xB1, 0xF, 0xF, true), hi ^= __builtin_amdgcn_update_dpp(0, hi, 0xB1, 0xF, 0xF, true);
  lo ^= __builtin_amdgcn_update_dpp(0, lo, 0x4E, 0xF, 0xF, true), hi ^= __builtin_amdgcn_update_dpp(0, hi, 0x4E, 0xF, 0xF, true);
  lo ^= __builtin_amdgcn_update_dpp(0, lo, 0x141, 0xF, 0xF, true), hi ^= __builtin_amdgcn_update_dpp(0, hi, 0x141, 0xF, 0xF, true);
  return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}

__device__ __forceinline__ unsigned long long roles_lane_word(const unsigned long long v, const int src) {
  return ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src) << 32) |
         (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src);
}

// the state the dynamics role left for environment e in this launch.  0: here it is; 1: gave up polling (reported, the
// environment marked broken); 2: an ABORT packet -- a launch behind a time-out: the wave ends without touching anything
// `tagmix`: 0 for a launch of one step; a launch of several steps mixes the step's number into every mark (roles_tagmix), so
// that a wave of step t + 1 that starts early cannot take step t's packet -- still up -- for its own
__device__ __forceinline__ unsigned long long roles_tagmix(const unsigned long long tag) { return tag * 0xd6e8feb86659fd93ull; }
// `have_first`: the caller has requested the packet already (`v_first`: its lane's word), ahead of other work -- in a launch of
// several steps the packet is usually there when the wave starts, and a wave that asks for it only HERE holds its slot for one more
// trip to memory (~1 us of a 12 us sweep: tools/multi_stamps.py); a packet of another step fails the mark and is polled for as ever
__device__ __forceinline__ int roles_wait_state(const AuvDev& d, const int e, const int lane, EnvPre& pre, const unsigned long long tagmix = 0ull,
                                                const bool have_first = false, const unsigned long long v_first = 0ull) {
  const unsigned long long* pk = d.k1_pkt + 8 * (size_t)e;
  // (polling harder does not pay: with two requests in flight per wave the packet is noticed sooner, but the
  // traffic of 3500 polling waves slows the dynamics role down by more -- 102.3 M against 104.7 M env-steps/s;
  // keeping the early waves quiet until the dynamics are about due moved every workload by +-2 % in no pattern)
  unsigned long long v = 0;
  for (int polls = 0;; polls++) {
    if (have_first && polls == 0) v = v_first;
    else v = __hip_atomic_load(pk + (lane & 7), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // one 64-byte request per wave
    const unsigned long long got = roles_lane_word(v, 7);
    if (got != 0ull) {
      unsigned long long x = roles_lane_word(v, 0);
#pragma unroll
      for (int i = 1; i < 7; i++) x ^= roles_lane_word(v, i);
      if (roles_mark(x ^ tagmix) == got) break;              // mark and payload belong together (and to this step)
    }
    if (polls == (AUV_HOOK_FAULT(d) ? (1 << 12) : PAIR_POLL_LIMIT)) {
      if (lane == 0) auv_st<true>(d.broken + e, (uint8_t)1);
      roles_give_up(d, d.e0, d.ne, 2, lane);
      return 1;
    }
    __builtin_amdgcn_s_sleep(ROLES_POLL_SLEEP);
  }
#pragma unroll
  for (int i = 0; i < 6; i++) pre.s[i] = pair_lane_value(v, i);
  pre.cnt.y = (int)__builtin_amdgcn_readlane((int)(unsigned)v, 6);   // the vessel's step counter of this launch
  return (unsigned)pre.cnt.y == ROLES_ABORT_COUNTER ? 2 : 0;
}

// ---- the finish role: navigation tail + reward / done / auto-reset, eight environments per wave ----
// Evaluated by one wave per environment the navigation's scalar tail keeps three to six lanes busy and was 19 % of the
// step's VALU issue cycles (profiles/r03/valu_budget_polygons50.json).  So the navigation wave only SEARCHES: it leaves
// the nearest segment (A, B, cumulative arclength) in a 64-byte record of NAV_HAND, checksummed like the state packet,
// and ends, handing its slot on.  A finish wave -- workgroups behind all others, group g of eight lanes <->
// environment, the dynamics role's mapping (same XCD as the environment's other waves) -- polls for the state packets
// and the search records of its eight environments, evaluates their tails (nav_tail<8>: the very code of the
// whole-wave form, so the same bits), polls for the sweeps' words, runs the reward phase in each group's first lane
// and takes the three marks down; environments that ended are then restored by the whole wave, one after the other.
// The tails run while the sweeps are still busy: only the reward phase (0.5-0.7 us) follows the last sweep.
// (A first version of this role in round 3 waited for all three hand-overs BEFORE the tail and fetched its table
// pointers with vector loads at the point of use: 38 against 31 us per chain step.  With the tail ahead of the second
// wait and the tables in scalar registers before the waits: 136 M against 130 M env-steps/s with four chains, 107
// against 100 M with one -- profiles/r03/shapes_sweep_finish_role.log.)
__device__ __forceinline__ void roles_publish_search(const AuvDev& d, const int e, const int lane, const NavNear& nr, const unsigned long long tagmix = 0ull) {
  unsigned long long* h = d.nav_hand + 8 * (size_t)e;
  // (wave-uniform values: lane 0 stores the five words one by one -- picking "this lane's word" would make the compiler
  // build a table in scratch memory; words 5 and 6 of the record stay zero)
  const unsigned long long w0 = (unsigned long long)__double_as_longlong(nr.A.x), w1 = (unsigned long long)__double_as_longlong(nr.A.y),
                           w2 = (unsigned long long)__double_as_longlong(nr.B.x), w3 = (unsigned long long)__double_as_longlong(nr.B.y),
                           w4 = (unsigned long long)__double_as_longlong(nr.cum);
  // (the mark goes out right behind the payload, not after its completion: it is a checksum of the payload, so a reader
  // that sees it ahead of a payload word polls again -- this wave stores nothing else)
  if (AUV_HOOK_FAULT(d) == 3 && e == d.e0) return;         // (test hook: the finish wave's time-out)
  if (lane == 0) {
    __hip_atomic_store(h + 0, w0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __hip_atomic_store(h + 1, w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(h + 2, w2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __hip_atomic_store(h + 3, w3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(h + 4, w4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(h + 7, roles_mark(w0 ^ w1 ^ w2 ^ w3 ^ w4 ^ tagmix), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// word `src` of the caller's group of eight lanes
__device__ __forceinline__ unsigned long long roles_group_word(const unsigned long long v, const int src) {
  const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src, K1_GROUP), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src, K1_GROUP);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ double roles_group_value(const unsigned long long v, const int src) {
  return __longlong_as_double((long long)roles_group_word(v, src));
}
// lane c of a group holds word c of a checksummed 64-byte record: does it hold together?
__device__ __forceinline__ bool roles_record_ok(const unsigned long long v, const int c, const unsigned long long tagmix = 0ull) {
  const unsigned long long x = roles_group_xor(c < 7 ? v : 0ull), mark = roles_group_word(v, 7);
  return mark != 0ull && roles_mark(x ^ tagmix) == mark;
}

__device__ __forceinline__ void roles_finish_wave(const AuvDev& dk, const int f, const int lane, float* __restrict__ obs_out,
                                                  float* __restrict__ reward_out, uint8_t* __restrict__ done_out) {
  // This role touches two dozen of the descriptor's tables, mostly while it waits: as kernel arguments they would be
  // fetched, and spilled, at the entry of every wave of every role.  They are read from the descriptor's device-side
  // copy (AuvDev::self) instead, through a pointer typed as constant memory -- scalar loads, issued here, before the
  // waits.  (Through a generic reference to the copy every table pointer is a vector load at its point of use.)  The
  // launch's own slice comes with the arguments.
  const __attribute__((address_space(4))) AuvDev* dc = (const __attribute__((address_space(4))) AuvDev*)dk.self;
  const AuvDev& d = *(const AuvDev*)dc;                           // (restore path, diagnostics)
  StepTabs st;                                                    // the tail's and the reward phase's tables and settings
  st.cfg.min_cumulative_reward = dc->cfg.min_cumulative_reward, st.cfg.min_goal_distance = dc->cfg.min_goal_distance;
  st.cfg.min_path_progress = dc->cfg.min_path_progress, st.cfg.look_ahead_distance = dc->cfg.look_ahead_distance;
  st.cfg.max_timesteps = dc->cfg.max_timesteps, st.cfg.rewarder = dc->cfg.rewarder, st.cfg.test_mode = dc->cfg.test_mode;
  st.cfg.auto_reset = dc->cfg.auto_reset, st.cfg.n_sensors = dc->cfg.n_sensors, st.cfg.use_lidar = dc->cfg.use_lidar;
  st.cfg.obs_channels = dc->cfg.obs_channels, st.pool_ns = dc->pool_ns;
  st.knot_s = dc->knot_s, st.knot_coef = dc->knot_coef;
  st.info64 = dc->info64, st.nav64 = dc->nav64, st.obs64 = dc->obs64, st.rew_path = dc->rew_path, st.reward64 = dc->reward64;
  st.step_info = dc->step_info, st.episode = dc->episode, st.ep_log = dc->ep_log, st.ep_log_count = dc->ep_log_count;
  st.ep_log_cap = dc->ep_log_cap, st.world_idx = dc->world_idx, st.counters = dc->counters;
  st.fw_serial = dc->fw_serial, st.n = dc->n;
  st.ring_slots = 1, st.ring_slot_host = 0, st.ring_pos = nullptr;          // (the dynamics role advances a captured graph's ring)
  unsigned long long* const pair_word = dc->pair_word;
  unsigned long long* const k1_pkt = dc->k1_pkt;
  unsigned long long* const nav_hand = dc->nav_hand;
  const EnvDesc* const env_desc = dc->env_desc;
  const double* const world_scalar = dc->world_scalar;
  double* const state = dc->state;
  const int n_envs = dc->n;
  const int ne = dk.ne, e0 = dk.e0;
  const int g = lane / K1_GROUP, c = lane % K1_GROUP;
  const int er = 8 * (8 * (f / 8) + g) + (f % 8);                 // the dynamics role's mapping
  const bool live = er < ne;
  const int e = e0 + (live ? er : ne - 1);                        // idle groups look at the last environment, store nothing
  // what earlier launches left (requested before the polls)
  int4 cnt = st.counters[e];
  const int w = st.world_idx[e];
  const double cum_in = st.info64[8 * (size_t)e + 4], cte_sum_in = st.info64[8 * (size_t)e + 7];
  const EnvDesc ed = env_desc[e];
  TailIn t;
  t.kn0 = ed.kn0, t.nk = ed.nk;
  {
    const double* ws = world_scalar + 8 * (size_t)ed.w;
    t.L = ws[0], t.goal_x = ws[1], t.goal_y = ws[2];
    t.knot_first = st.knot_s[ed.kn0], t.knot_last = st.knot_s[ed.kn0 + ed.nk - 1];
    t.maxp_in = st.info64[8 * (size_t)e + 5];
  }
  const unsigned long long* pk = k1_pkt + 8 * (size_t)e;
  unsigned long long* hd = nav_hand + 8 * (size_t)e;
  const int limit = AUV_HOOK_FAULT(dk) ? (1 << 12) : PAIR_POLL_LIMIT;
#ifdef AUV_STAMPS
  if (live && c == 0) d.stamps[(size_t)e * 16 + 10] = wall_clock64();   // the finish wave has its slot
#endif
  // ---- the state packet and the search record of every group ----
  unsigned long long vp = 0ull, vh = 0ull;
  bool okp = !live, okh = !live, aborted = false;
  uint8_t* const broken = dc->broken;
  for (int polls = 0;; polls++) {
    if (!okp) vp = __hip_atomic_load(pk + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // one 64-byte request per group
    if (!okh) vh = __hip_atomic_load(hd + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    okp = !live || roles_record_ok(vp, c);
    // an ABORT packet (a launch behind a time-out): no search record, no sweep's word will follow
    aborted = live && okp && (unsigned)roles_group_word(vp, 6) == ROLES_ABORT_COUNTER;
    okh = !live || aborted || roles_record_ok(vh, c);
    if (!__any(!(okp && okh))) break;
    if (polls == limit) {
      if (live && c == 0) auv_st<true>(broken + e, (uint8_t)1);
      roles_give_up(d, e0, ne, 3, lane);
      return;
    }
    __builtin_amdgcn_s_sleep(ROLES_POLL_SLEEP);
  }
  if (__any(aborted)) {
    // the eight environments of a finish wave are the eight of ONE dynamics wave: all of them or none.  The ABORT packets
    // stay up -- this wave does not know whether the environments' sweep and search waves have seen them yet; later
    // launches are aborted too (they overwrite them with their own) and the host's recovery clears every mark
    return;
  }
  t.px = roles_group_value(vp, 0), t.py = roles_group_value(vp, 1), t.psi = roles_group_value(vp, 2);
  t.u = roles_group_value(vp, 3), t.v = roles_group_value(vp, 4), t.r = roles_group_value(vp, 5);
  cnt.y = (int)(unsigned)roles_group_word(vp, 6);                 // the vessel's step counter of this launch
  t.nr.A = make_double2(roles_group_value(vh, 0), roles_group_value(vh, 1));
  t.nr.B = make_double2(roles_group_value(vh, 2), roles_group_value(vh, 3));
  t.nr.cum = roles_group_value(vh, 4);
#ifdef AUV_STAMPS
  if (live && c == 0) d.stamps[(size_t)e * 16 + 9] = wall_clock64();    // state and search result are here
#endif
  NavOut no;
  no.rew_path = no.reached = no.goal = no.progress = no.u = no.v = no.r = no.cte100 = 0.0;
  // a first look at the sweeps' words BEFORE the tail's stores (a look behind them waits for them: with one chain the words
  // are there by the time a finish wave runs, and the poll below is then not entered at all)
  unsigned long long word = live ? __hip_atomic_load(pair_word + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
  if (AUV_RUN_N(dk, 3)) no = nav_tail<K1_GROUP>(st, e, c, live, t, obs_out);
  // STATE rows of the new state (the dynamics role leaves only the packet): lane c of a group holds component c.  (Behind the
  // tail, not in front of it: the tail's loads would wait for this store -- one counter, in issue order.)
  if (live && c < 6) state[(size_t)c * (size_t)n_envs + e] = __longlong_as_double((long long)vp);
#ifdef AUV_STAMPS
  if (live && c == 0) d.stamps[(size_t)e * 16 + 13] = wall_clock64();   // the tail is done
#endif
  // ---- the sweeps' words ----
  for (int polls = 0;; polls++) {
    if (!__any(word == PAIR_EMPTY)) break;
    if (word == PAIR_EMPTY) word = __hip_atomic_load(pair_word + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!__any(word == PAIR_EMPTY)) break;
    if (polls == limit) {
      if (live && c == 0) auv_st<true>(broken + e, (uint8_t)1);
      roles_give_up(d, e0, ne, 1, lane);
      return;
    }
    __builtin_amdgcn_s_sleep(ROLES_POLL_SLEEP);
  }
#ifdef AUV_STAMPS
  if (live && c == 0) d.stamps[(size_t)e * 16 + 7] = wall_clock64();    // the sweep's word is here: start of the reward phase
#endif
  int do_reset = 0;
  if (live && c == 0) {
    // the three marks come down for the next launch (the sweep and the search waves of this environment are gone)
    __hip_atomic_store(pair_word + e, PAIR_EMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(k1_pkt + 8 * (size_t)e + 7, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(hd + 7, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    RewardIn in;
    const int collision = word == PAIR_COLLISION;
    in.closeness_reward = collision ? 0.0 : __longlong_as_double((long long)word);
    in.path_reward = no.rew_path, in.reached = no.reached, in.goal = no.goal, in.progress = no.progress;
    in.u = no.u, in.v = no.v, in.yaw_rate = no.r;
    in.cum = cum_in;
    in.cte100 = no.cte100, in.cte_sum = cte_sum_in;
    st.info64[8 * (size_t)e] = collision;
    do_reset = reward_apply(st, e, collision, cnt, in, reward_out, done_out, false);
  }
  unsigned long long m = __ballot(do_reset);
  if (m) {
    while (m) {
      const int src = __ffsll((long long)m) - 1;
      m &= m - 1;
      const int er2 = auv_uniform(__shfl(e, src, AUV_WAVE));
      const int wr = auv_uniform(__shfl(w, src, AUV_WAVE)), ep = auv_uniform(__shfl(cnt.z, src, AUV_WAVE));
      const AuvDev* dp = dk.self;
      asm volatile("" : "+s"(dp));      // (the copy's tables are fetched inside the loop: hoisted out of it they are spilled, and the
                                        // spill slots keep 36 B of scratch memory enabled for every wave of the launch)
      const AuvDev& dr = *(const AuvDev*)(const __attribute__((address_space(4))) AuvDev*)dp;
      restore_env(dr, er2, auv_next_world_wave(dr, wr, lane), lane, ep, obs_out);
    }
  }
#ifdef AUV_STAMPS
  if (live && c == 0) d.stamps[(size_t)e * 16 + 15] = wall_clock64();
#endif
}

__global__ void __launch_bounds__(AUV_WAVE, AUV_K23_MIN_WAVES) k_step_roles(AuvDev dk, const void* __restrict__ actions,
                                                                           float* __restrict__ obs_out,
                                                                           float* __restrict__ reward_out,
                                                                           uint8_t* __restrict__ done_out) {
  const AuvDev& d = dk;
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x;
  const int ne = d.ne;                                              // environments of this launch: [e0, e0 + ne)
  const int nk = 8 * ((ne + 63) / 64);                              // dynamics workgroups
  const int nb = 8 * ((ne + 7) / 8);                                // LiDAR workgroups
  // (the search workgroups dispatched AHEAD of the LiDAR ones -- they are short, and with one chain they only get their
  // slots when sweeps retire -- was measured: 102.3 against 106.5 M env-steps/s with one chain, 129 against 136 M with
  // four: the sweeps are the long pole and must start first.  Blocks of eight LiDAR and eight search workgroups
  // alternating: 95.6 against 111.6 M with one chain, 130 against 142 M with four.)
  const int b = (int)blockIdx.x;
  if (b < nk) {
    // ---- Vessel.step of eight environments ----
    // (everybody else in the launch waits for these 512 waves: they go first wherever they share a SIMD)
    __builtin_amdgcn_s_setprio(3);
    const int g = lane / K1_GROUP, c = lane % K1_GROUP;
    const int er = 8 * (8 * (b / 8) + g) + (b % 8);
    const bool live = er < ne;
    const int eg = d.e0 + (live ? er : ne - 1);                     // idle groups compute along, store nothing
    const int y = d.counters[eg].y + 1;                             // Vessel._step_counter (vessel.py:247); requested up front
    // a launch queued behind a hand-over time-out (the flag is wave-uniform, a scalar load): the dynamics role hands out
    // ABORT packets instead of states, on which every other wave of the launch ends without touching its environment --
    // the whole decision hangs on THIS wave's one look at the flag, so an environment's four waves always agree
    const int aborted = auv_uniform(*d.abort_flag);
    double t = 0.0;
    if (!aborted) t = k1_group(d, actions, eg, lane);
    unsigned long long* pk = d.k1_pkt + 8 * (size_t)eg;
    const unsigned long long word = aborted ? (c == 6 ? (unsigned long long)ROLES_ABORT_COUNTER : 0ull)
                                            : (c < 6 ? (unsigned long long)__double_as_longlong(t) : (c == 6 ? (unsigned long long)(unsigned)y : 0ull));
    const unsigned long long mark = roles_mark(roles_group_xor(word));
    // The packet is ALL this role stores: payload and mark in ONE store instruction, 64 contiguous bytes per group, and
    // the wave does not wait for it.  The mark is a checksum of the payload, so a reader that sees the mark before all
    // of the payload (should the request ever be served in pieces) just polls again.  STATE and the vessel's step
    // counter are written by the finish wave from the packet (roles_finish_wave) -- the wave that may also overwrite
    // them when the episode ends, so the two stores are ordered by ITS program order, not by a wait here -- and the
    // 0.5-1 us this wave used to wait for its write-through stores before raising the mark are off the head of the
    // launch that everybody else waits for.
    if (live && !(AUV_HOOK_FAULT(d) == 2 && eg == d.e0))       // (test hook: nobody gets the first environment's state)
      __hip_atomic_store(pk + c, c < 7 ? word : mark, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // a captured graph's action ring: every dynamics wave has read the position before it counts itself off, so
    // the last one to do so may move it on
    if (d.ring_slots > 1 && d.ring_slot_host == -1 && lane == 0) {
      const int old = __hip_atomic_fetch_add(d.k1_done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (old == nk - 1) {
        *d.ring_pos = (*d.ring_pos + 1) % d.ring_slots;
        __hip_atomic_store(d.k1_done, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
#ifdef AUV_STAMPS
    if (live && c == 0) d.stamps[(size_t)eg * 16 + 0] = wall_clock64();   // the state of this environment is out
#endif
    return;   // (carrying on as the LiDAR wave of an environment instead of handing the slot to a fresh workgroup was
              // tried: the merged code path costs more scalar-register spills than the later start of 512 sweeps: -2.5 %;
              // with the dynamics in a function of its own (not inlined, arguments by value) they are 1 us slower: -4.5 %.
              // So was the scalar form of the integrator, lanes <-> environments, on 64 waves instead of 512: its
              // chain is 3 us longer and everybody waits for it, 97.2 M against 104.7 M env-steps/s.)
  }
  EnvPre pre;
  EnvDesc ed;
  if (b < nk + nb) {
    // ---- _update + Vessel.perceive of one environment ----
    if (b - nk >= ne) return;
    const int e = auv_uniform(d.e0 + b - nk);
    // (The SIMD's arbiter favours its oldest wave: at equal work the sweeps dispatched last take half as long again as
    // the first, 17 against 12 us, and end the launch -- tools/phase_stamps3.py.  A priority graded by workgroup index
    // evens that out and LOSES 1-2 % either way round: the early finishers make room for navigation waves, whose
    // memory latency then hides behind the late sweeps' arithmetic.  With four roles: a sweep that is behind schedule
    // raising its own priority -- clock read after the front and after the pair sweep, s_setprio 2 beyond 4 / 8 or
    // 5.5 / 11 us since the state arrived -- changes nothing, 135.3-135.9 against 135.6-136.4 M with four chains: the
    // stragglers are not short of issue slots.)
    // while the dynamics role integrates: everything of the sweep that does not need the vessel's new state --
    // descriptor and counters (written by earlier launches), the movers' kinematics, the obstacle records
#ifdef AUV_STAMPS
    if (lane == 0) d.stamps[(size_t)e * 16 + 3] = wall_clock64();
#endif
    // (a launch queued behind a hand-over time-out: nothing is touched.  The dynamics wave's look at the flag is the one
    // that counts -- see there -- this one only keeps the movers from being advanced by a launch that will be aborted)
    if (auv_uniform(*d.abort_flag)) return;
    ed = d.env_desc[e];
    pre.cnt = d.counters[e];                               // t_step, episodes; the step counter comes with the state
    pre.ed = &ed;
    const Slice L = carve(smem, d);
    k2_movers<true>(d, e, lane, L, ed, 1);
    const K2Pre kp = k2_prefetch(d, e, lane, ed);
    k2_stage_beams(d, lane, L);
    // (also tried here: warming the caches with the nearby obstacles' boundary segments -- it has to wait for the
    // obstacle records, and its traffic delays the dynamics role: 102.1 M against 104.5 M env-steps/s without)
#ifdef AUV_STAMPS
    if (lane == 0) d.stamps[(size_t)e * 16 + 1] = wall_clock64();
#endif
    {
      const int ws = roles_wait_state(d, e, lane, pre);
      if (ws) {
        // an ABORT packet although this wave saw the flag down a moment ago: the flag went up in between, and the movers of
        // this environment have been advanced for a step that will not happen -- the recovery resets it
        if (ws == 2 && ed.M > 0 && lane == 0) auv_st<true>(d.broken + e, (uint8_t)1);
        return;
      }
    }
#ifdef AUV_STAMPS
    if (lane == 0) d.stamps[(size_t)e * 16 + 2] = wall_clock64();
#endif
    int n_act = 0;
    int2 lim0 = make_int2(INT32_MIN, INT32_MIN);           // this lane's cull-limit row: stored by k2_back (see there)
    if (AUV_RUN_L(d, 1)) n_act = k2_front<true>(d, e, lane, L, 1, &pre, 1, &kp, true, &lim0);
#ifdef AUV_STAMPS
    if (lane == 0) d.stamps[(size_t)e * 16 + 8] = wall_clock64();      // front (B0, B, C) done
#endif
    if (AUV_RUN_L(d, 3)) k2_stage_and_pairs(d, L, lane, n_act, pre.s[2]);
#ifdef AUV_STAMPS
    if (lane == 0) d.stamps[(size_t)e * 16 + 11] = wall_clock64();     // staging + pair sweep (S, D) done
#endif
    double term = 0.0;
    const int collision = k2_back<true>(d, e, lane, L, n_act, obs_out, &term, &lim0);
#ifdef AUV_STAMPS
    if (lane == 0) d.stamps[(size_t)e * 16 + 4] = wall_clock64();
#endif
    pair_publish_lidar(d, e, lane, collision, term);
#ifdef AUV_STAMPS
    if (lane == 0) d.stamps[(size_t)e * 16 + 14] = wall_clock64();
#endif
  } else if (b < nk + 2 * nb + AUV_HOOK_SKEW(d)) {
    // ---- Vessel.navigate of one environment: the nearest-point search ----
    const int el = b - nk - nb - AUV_HOOK_SKEW(d);
    if (el < 0 || el >= ne) return;
    const int e = auv_uniform(d.e0 + el);
    ed = d.env_desc[e];
    pre.cnt = d.counters[e];
    pre.ed = &ed;
#ifdef AUV_STAMPS
    if (lane == 0) d.stamps[(size_t)e * 16 + 12] = wall_clock64();
#endif
    if (roles_wait_state(d, e, lane, pre)) return;
#ifdef AUV_STAMPS
    if (lane == 0) d.stamps[(size_t)e * 16 + 5] = wall_clock64();
#endif
    // the search only: nearest segment of the path -> NAV_HAND; the finish role takes it from there
    NavNear nr;
    nr.A = nr.B = make_double2(0.0, 0.0), nr.cum = 0.0;
    if (AUV_RUN_N(d, 1)) {
      int* list = (int*)smem;
      const NavSpec sp = nav_bounds(d, e, lane, list, pre.s[0], pre.s[1], &ed);
      if (AUV_RUN_N(d, 2)) nr = nav_nearest(d, e, lane, list, pre.s[0], pre.s[1], sp);
    }
    roles_publish_search(d, e, lane, nr);
#ifdef AUV_STAMPS
    if (lane == 0) d.stamps[(size_t)e * 16 + 6] = wall_clock64();     // the search result is out
#endif
  } else {
    // ---- navigation tail + reward / done / auto-reset of eight environments ----
    const int f = b - nk - 2 * nb - AUV_HOOK_SKEW(d);
    if (f < 0 || f >= nk) return;
    __builtin_amdgcn_s_setprio(2);
    roles_finish_wave(d, f, lane, obs_out, reward_out, done_out);
  }
}

// ---- SEVERAL steps in ONE launch (auv_step_multi) ---------------------------------------------------------
// An open-loop stretch knows its actions ahead (a ring of slots), so nothing but the launch boundary makes step t + 1 of an
// environment wait for the slowest sweep of the whole slice.  k_step_multi is k_step_roles' grid T times over, step-major:
// workgroup b plays role b % per of step b / per.  Workgroups are still dispatched in index order, so every wave's producers --
// its own step's lower roles and the previous step's finish wave -- are resident or done when it gets its slot; as step t's
// waves retire, step t + 1's take their slots, and an environment's next dynamics starts when ITS finish wave is through.
// What a kernel boundary used to do between two steps is done explicitly:
//   * the CARRY record (AuvDev::carry, 24 words per environment): what the next step's roles need of this step's outcome --
//     the state and the counters (dynamics: words 0..7, the very format of the state packet), episode count, cumulative reward,
//     maximum progress, cross-track sum and the table descriptor (sweep, search, finish).  The finish wave writes it last, by
//     agent-scope stores, with two checksum marks that carry the step's number; the next step's waves poll for marks that match
//     THEIR step.  Step 0 of a launch reads the arrays as ever (a kernel boundary lies in front of it), and the last step's finish
//     wave leaves the arrays as ever for the launch that follows.
//   * the rows one wave writes and ANOTHER step's wave reads -- mover states, the cached nearby mask -- are stored write-through
//     (they already were) and, in steps > 0, loaded with agent-scope loads (k2_movers / k2_prefetch <LD>); restore_env stores
//     them write-through too (<WTM>).  Everything else a step writes is output only (or a hint: the path search's starting
//     chunk, where a stale value costs nothing but a wider first bound).
//   * every mark of a step is mixed with the step's number (roles_tagmix), so a packet of step t still up cannot pass for
//     step t + 1's.
// Bitwise the same as T launches of k_step_roles (tests/test_gpu_multi.py).  With a fresh world per reset a slot's tables may be
// rebuilt beside the launch, and only the binding STEP reads them coherently: these kernels are refused there, and k_fresh_multi /
// k_fresh_record (the same body, STEP_MULTI_FW; closed loop: k_fresh_feedback and its two siblings) bind only slots published before
// their call began (auv_device.h: auv_next_world_multi).
#define CARRY_WORDS 24
// The second mark covers words 8..19, which lie in two 64-byte lines that are stored and loaded separately, so a reader CAN see
// the old words 8..15 beside the new words 16..20.  A plain xor of the words lets that pass whenever the changes of two words
// cancel: a cumulative reward and a cross-track sum that both double within their binade (r -> 2 r beside 4 -> 8) flip the same
// exponent bits, and the reader took running sums one step old (tests/test_gpu_nav_edges.py: an environment at rest 4 m off its
// path).  Every word is therefore multiplied by an odd constant of its position before the xor: equal words stay equal, and two
// changed words cancel only if their products differ in the same bits -- 2^-63 for unrelated words.
__device__ __forceinline__ unsigned long long carry_mix(const unsigned long long w, const int i) {
  return w * (ROLES_MAGIC * (unsigned long long)(2 * i + 1));
}

// Diagnostic build only (-DAUV_STAMPS_MULTI, tools/multi_stamps.py): wall-clock stamps of the waves of ONE step in the middle of a
// multi-step launch (the other steps stamp into a dummy half of the array), 16 words per environment:
//   sweep wave   0 role begins  1 the wave's first instruction  2 state packet here  3 all its stores acknowledged  4 pair sweep done  5 word published
//   search wave  6 role begins  7 the wave's first instruction  8 state packet here  9 record published
//   dynamics    10 has its slot 11 carry record here 12 packet stored      finish 13 has its slot 14 sweeps' words here 15 done
// s_waitcnt with vmcnt = 0 and the other counters left open (gfx9 encoding): every load and store of the wave has completed
#define AUV_WAITCNT_VMCNT0 0x0F70
#ifdef AUV_STAMPS_MULTI
#define MSTAMP(e, k) do { if (lane == 0) stamp[(size_t)(e) * 16 + (k)] = wall_clock64(); } while (0)
#define MSTAMP_IF(cond, e, k) do { if (cond) stamp[(size_t)(e) * 16 + (k)] = wall_clock64(); } while (0)
#define MSTAMP_PARAM , unsigned long long* stamp
#define MSTAMP_ARG , stamp
#else
#define MSTAMP(e, k) do { } while (0)
#define MSTAMP_IF(cond, e, k) do { } while (0)
#define MSTAMP_PARAM
#define MSTAMP_ARG
#endif

__device__ __forceinline__ unsigned long long carry_ed_word(const EnvDesc& ed, const int i) {
  switch (i) {
    case 0: return (unsigned long long)ed.k0;
    case 1: return (unsigned long long)ed.m0;
    case 2: return (unsigned long long)ed.p0;
    case 3: return (unsigned long long)ed.c0;
    case 4: return (unsigned long long)ed.kn0;
    case 5: return (unsigned long long)(unsigned)ed.K | ((unsigned long long)(unsigned)ed.M << 32);
    case 6: return (unsigned long long)(unsigned)ed.P | ((unsigned long long)(unsigned)ed.nch << 32);
    default: return (unsigned long long)(unsigned)ed.nk | ((unsigned long long)(unsigned)ed.w << 32);
  }
}
__device__ __forceinline__ void carry_ed_from(EnvDesc& ed, const unsigned long long w[8]) {
  ed.k0 = (long long)w[0], ed.m0 = (long long)w[1], ed.p0 = (long long)w[2], ed.c0 = (long long)w[3], ed.kn0 = (long long)w[4];
  ed.K = (int)(unsigned)w[5], ed.M = (int)(unsigned)(w[5] >> 32), ed.P = (int)(unsigned)w[6], ed.nch = (int)(unsigned)(w[6] >> 32);
  ed.nk = (int)(unsigned)w[7], ed.w = (int)(unsigned)(w[7] >> 32);
}

// a first look at the carry record, requested by the caller ahead of work that must not sit between the wave's start and this
// request (the multi-step sweep: carving its slice, staging the beam table); this lane's word goes to carry_wait_wave as `v_first`
__device__ __forceinline__ unsigned long long carry_request(const AuvDev& d, const int e, const int lane) {
  return lane < CARRY_WORDS ? __hip_atomic_load(d.carry + CARRY_WORDS * (size_t)e + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
}
// one wave, one environment (sweep, search): the carry of the previous step.  0: here it is; 1: gave up (reported, environment
// marked); 2: the abort flag went up meanwhile -- the wave ends without touching anything
__device__ __forceinline__ int carry_wait_wave(const AuvDev& d, const int e, const int lane, const unsigned long long tagmix, EnvDesc& ed, int4& cnt,
                                               const bool have_first = false, const unsigned long long v_first = 0ull) {
  const unsigned long long* cw = d.carry + CARRY_WORDS * (size_t)e;
  unsigned long long v = 0ull;
  for (int polls = 0;; polls++) {
    if (have_first && polls == 0) v = v_first;
    else if (lane < CARRY_WORDS) v = __hip_atomic_load(cw + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long ma = roles_lane_word(v, 7), mb = roles_lane_word(v, 20);
    if (ma != 0ull && mb != 0ull) {
      const unsigned long long vm = carry_mix(v, lane);          // (lane i holds word i: one vector multiply serves words 8..19)
      unsigned long long xa = roles_lane_word(v, 0), xb = roles_lane_word(vm, 8);
#pragma unroll
      for (int i = 1; i < 7; i++) xa ^= roles_lane_word(v, i);
#pragma unroll
      for (int i = 9; i < 20; i++) xb ^= roles_lane_word(vm, i);
      if (roles_mark(xa ^ tagmix) == ma && roles_mark(xb ^ tagmix) == mb) break;
    }
    if ((polls & 31) == 31 && auv_uniform(__hip_atomic_load(d.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) return 2;
    if (polls == (AUV_HOOK_FAULT(d) ? (1 << 12) : PAIR_POLL_LIMIT)) {
      if (lane == 0) auv_st<true>(d.broken + e, (uint8_t)1);
      roles_give_up(d, d.e0, d.ne, 6, lane);
      return 1;
    }
    __builtin_amdgcn_s_sleep(ROLES_POLL_SLEEP);
  }
  unsigned long long w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = roles_lane_word(v, 12 + i);
  carry_ed_from(ed, w);
  const unsigned long long c6 = roles_lane_word(v, 6), c8 = roles_lane_word(v, 8);
  cnt = make_int4((int)(unsigned)c6, (int)(unsigned)(c6 >> 32), (int)(unsigned)c8, 0);
  return 0;
}

// ---- the affine feedback law of a closed-loop launch (auv_step_feedback, k_step_feedback) ----
// Per environment e a gain row G[e][2][8] (fp64); output j (0 thrust, 1 rudder) of step t is
//     x_c = OBS64[e][c], c = 0..5 (the six navigation columns as step t - 1 left them; after an auto-reset the new episode's reset
//           row; for the launch's first step what the arrays hold),  x_6 = 1.0,
//     x_7 = component j of the ring's action in slot (first_slot + t) % n_slots, converted as k1_action converts it (no ring: 0.0),
//     p_c = G[e][j][c] * x_c,   a_j = ((p_0 + p_1) + (p_2 + p_3)) + ((p_4 + p_5) + (p_6 + p_7))
// in fp64, FMA contraction off, exactly this association (host mirror: gym_auv_amd/feedback.py, affine_action).  `a` goes to
// k1_group as `a_in`: the NaN rule and the clip to the action range stay in the dynamics.
// Lane c of a group of eight owns column c.  The group sum is three DPP adds -- quad_perm [1,0,3,2]: p_2k + p_2k+1; quad_perm
// [2,3,0,1]: the quad's two pairs; row_half_mirror: the two quads -- which IS the association above in group lane 0, operand order
// included (the other lanes add the same pairs with the operands swapped: the same bits for numbers); every lane then takes group
// lane 0's bits.  Called by all 64 lanes.
__device__ __forceinline__ double fb_group_sum(double p) {
  p += auv_dpp_f64<0xB1>(p);
  p += auv_dpp_f64<0x4E>(p);
  p += auv_dpp_f64<0x141>(p);
  return k1_group_bcast<0>(p);
}
// x: column c of the OBS64 row (lanes c < 6); g0 / g1: G[e][0][c], G[e][1][c]; r0 / r1: the ring's action of the step the law is for
__device__ __forceinline__ double2 fb_law(const int c, const double x, const double g0, const double g1, const double r0, const double r1) {
  const double x0 = c < 6 ? x : (c == 6 ? 1.0 : r0), x1 = c < 6 ? x : (c == 6 ? 1.0 : r1);
  return make_double2(fb_group_sum(g0 * x0), fb_group_sum(g1 * x1));
}
// lane c of a group holds word 16 + c of a carry record: do the action words (21, 22) and their mark (23) hold together?
__device__ __forceinline__ bool fb_record_ok(const unsigned long long v2, const int c, const unsigned long long tagmix) {
  const unsigned long long x = roles_group_xor((c == 5 || c == 6) ? v2 : 0ull), mark = roles_group_word(v2, 7);
  return mark != 0ull && roles_mark(x ^ tagmix) == mark;
}


// ---- LiDAR sector inputs of the law (auv_step_feedback_sectors, k_step_sector_feedback) ----
// The OBS64 row's closeness columns (from column 6 on: one per beam, or one per sector in the feasibility-pooled configuration) are
// cut into at most 16 sectors by a bounds table b[0..16] (the host pads it with its last entry: the sectors past the caller's K are
// empty ranges); z_k = the maximum of columns b[k] <= i < b[k+1] -- from the first element on with m = v > m ? v : m, +0.0 for an
// empty range -- and with sector gains H[e][2][16]
//     q_k = H[e][j][k] * z_k,   u_j = ((q_0 + q_1) + (q_2 + q_3)) + ((q_4 + q_5) + (q_6 + q_7)),   w_j = the same over q_8..q_15,
//     a_j = s_j + (u_j + w_j),  s_j = fb_law's sum
// fp64, no FMA, this association (host mirror: gym_auv_amd/feedback.py, sector_action).  Lane c of a group of eight owns sectors c
// and 8 + c: u_j and w_j are fb_group_sum of its two products, the last two adds are made alike in every lane.
struct FbBounds {
  int b[17];
};
// lane c's two ranges, (b[c], b[c + 1], b[8 + c], b[9 + c]): the table is a kernel argument by value, wave-uniform, and is taken
// into scalar registers HERE (laundered: left to itself the compiler selects the OFFSET per lane and gathers the four entries from
// the argument segment with vector loads, a memory trip in front of the first sector load); the lane's entries are then chains of
// selects on constant indices
__device__ __forceinline__ int4 fb_ranges(const FbBounds& sb, const int c) {
  int b[17];
#pragma unroll
  for (int i = 0; i < 17; i++) {
    b[i] = sb.b[i];
    asm("" : "+s"(b[i]));
  }
  int4 r = make_int4(b[0], b[1], b[8], b[9]);
#pragma unroll
  for (int i = 1; i < 8; i++) r.x = c == i ? b[i] : r.x, r.y = c == i ? b[i + 1] : r.y, r.z = c == i ? b[8 + i] : r.z, r.w = c == i ? b[9 + i] : r.w;
  return r;
}
#define FB_SECTOR_BATCH 4   // loads in flight per range and trip; what is loaded is consumed at once: no array of a sector's beams
// z of this lane's two sectors.  row6: column 6 of the environment's OBS64 row.  COH: agent-scope loads (the finish wave, behind the
// sweep's pair word and its own store drain), else plain loads (step 0: the arrays, behind the kernel boundary).  Both ranges go
// through one loop, FB_SECTOR_BATCH columns of each per trip; a trip past a range's end (or an empty range) re-reads a column of
// the row -- its last one, or column 6 -- and drops it, so every address stays inside the row and no load sits under a branch.  The
// maximum of a range is taken in ascending column order; a column read twice changes nothing.
template <bool COH>
__device__ __forceinline__ double2 fb_sector_pair(const double* __restrict__ row6_, const int4 rg) {
  // (a global address: through the descriptor's generic pointer these would be flat loads, which count against the LDS counter too)
  const __attribute__((address_space(1))) double* row6 = (const __attribute__((address_space(1))) double*)row6_;
  const int lo0 = rg.x, hi0 = rg.y, lo1 = rg.z, hi1 = rg.w;
  double m0 = 0.0, m1 = 0.0;
  for (int i0 = lo0, i1 = lo1; __any(i0 < hi0 || i1 < hi1); i0 += FB_SECTOR_BATCH, i1 += FB_SECTOR_BATCH) {
    const bool on0 = i0 < hi0, on1 = i1 < hi1;
    double v0[FB_SECTOR_BATCH], v1[FB_SECTOR_BATCH];
#pragma unroll
    for (int k = 0; k < FB_SECTOR_BATCH; k++) {
      const int j0 = on0 ? (i0 + k < hi0 ? i0 + k : hi0 - 1) : 0, j1 = on1 ? (i1 + k < hi1 ? i1 + k : hi1 - 1) : 0;
      if constexpr (COH) {
        v0[k] = __hip_atomic_load(row6 + j0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v1[k] = __hip_atomic_load(row6 + j1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        v0[k] = row6[j0], v1[k] = row6[j1];
      }
    }
    double n0 = i0 == lo0 ? v0[0] : (v0[0] > m0 ? v0[0] : m0), n1 = i1 == lo1 ? v1[0] : (v1[0] > m1 ? v1[0] : m1);
#pragma unroll
    for (int k = 1; k < FB_SECTOR_BATCH; k++) n0 = v0[k] > n0 ? v0[k] : n0, n1 = v1[k] > n1 ? v1[k] : n1;
    m0 = on0 ? n0 : m0, m1 = on1 ? n1 : m1;
  }
  return make_double2(m0, m1);
}
// s: fb_law's sums; z: this lane's two sector inputs; h0 / h1: H[e][0][c], H[e][0][8 + c] / H[e][1][c], H[e][1][8 + c]
__device__ __forceinline__ double2 fb_law_sectors(const double2 s, const double2 z, const double2 h0, const double2 h1) {
  const double u0 = fb_group_sum(h0.x * z.x), w0 = fb_group_sum(h0.y * z.y);
  const double u1 = fb_group_sum(h1.x * z.x), w1 = fb_group_sum(h1.y * z.y);
  return make_double2(s.x + (u0 + w0), s.y + (u1 + w1));
}

// ---- one hidden layer on top of the law (auv_step_feedback_hidden, k_step_hidden_feedback) ----
// Per environment 16 hidden units over 24 inputs, the same for both outputs:
//     v_0..5 = x_0..5 of fb_law,   v_6, v_7 = the two components of the ring's action of the step the law is for (no ring: 0.0),
//     v_8..23 = z_0..15 of the sector law (the same bounds, the same maxima)
//     s = b_h;  for i = 0, 1, ..., 23 in this order  s = s + (w_h[i] * v_i)     (each product and each sum rounded once)
//     y_h = s > 0.0 ? s : +0.0                                    activation 0, relu (a NaN gives +0.0)
//     y_h = s > 1.0 ? 1.0 : (s < -1.0 ? -1.0 : s)                 activation 1, hard tanh (a NaN passes)
//     r_k = V[j][k] * y_k,   ha_j = ((r_0 + r_1) + (r_2 + r_3)) + ((r_4 + r_5) + (r_6 + r_7)),   hb_j = the same over r_8..r_15,
//     a_j = (s_j + (u_j + w_j)) + (ha_j + hb_j)                   the first bracket: fb_law_sectors' result, unchanged
// fp64, no FMA, this association (host mirror: gym_auv_amd/feedback.py, hidden_action).  The parameters: [N][16][28] fp64, row h =
// (w_h[0..23], b_h, V[0][h], V[1][h], pad) -- 224 bytes, so every pair of a row is a 16-byte aligned load.  Lane c of a group of
// eight owns units c and 8 + c, like the sectors: ha_j and hb_j are fb_group_sum of its two products.  Every lane needs all 24
// inputs; they sit one (x), or two (z), per lane of the group and are taken from there by DPP moves (k1_group_bcast) at the moment
// they are multiplied -- no array of inputs, and of the 2 x 27 parameters of a lane only one batch of FB_HIDDEN_BATCH inputs' is
// in registers at a time.
#define FB_HIDDEN_BATCH 8   // inputs per batch: 2 units x 4 pairs in flight, consumed at once
#define FB_HIDDEN_ROW 28    // doubles per unit
typedef double fb_pair __attribute__((ext_vector_type(2)));   // (a native vector: one 16-byte global load)
struct FbHiddenBatch {
  fb_pair p0[FB_HIDDEN_BATCH / 2], p1[FB_HIDDEN_BATCH / 2];     // pairs (w[i], w[i + 1]) of units c and 8 + c
};
// hp: row c of the environment's block (row 8 + c is 8 rows on).  Plain loads: nothing in a launch writes the parameters.
template <int B> __device__ __forceinline__ FbHiddenBatch fb_hidden_request(const double* __restrict__ hp_) {
  const __attribute__((address_space(1))) fb_pair* hp = (const __attribute__((address_space(1))) fb_pair*)hp_;
  FbHiddenBatch w;
#pragma unroll
  for (int k = 0; k < FB_HIDDEN_BATCH / 2; k++)
    w.p0[k] = hp[B * (FB_HIDDEN_BATCH / 2) + k], w.p1[k] = hp[8 * (FB_HIDDEN_ROW / 2) + B * (FB_HIDDEN_BATCH / 2) + k];
  return w;
}
// (b_h, V[0][h]) and (V[1][h], pad) of the lane's two units
struct FbHiddenTail {
  fb_pair bv0, bv1, vp0, vp1;
};
__device__ __forceinline__ FbHiddenTail fb_hidden_request_tail(const double* __restrict__ hp_) {
  const __attribute__((address_space(1))) fb_pair* hp = (const __attribute__((address_space(1))) fb_pair*)hp_;
  FbHiddenTail t;
  static_assert(24 % FB_HIDDEN_BATCH == 0 && FB_HIDDEN_BATCH % 2 == 0, "whole batches of pairs");
  t.bv0 = hp[12], t.bv1 = hp[8 * (FB_HIDDEN_ROW / 2) + 12], t.vp0 = hp[13], t.vp1 = hp[8 * (FB_HIDDEN_ROW / 2) + 13];
  return t;
}
// input I (a constant) in every lane of the group.  x: column c in lanes c < 6; r0, r1: the ring's action; z: the lane's two sectors
template <int I> __device__ __forceinline__ double fb_hidden_input(const double x, const double r0, const double r1, const double2 z) {
  static_assert(I >= 0 && I < 24, "input of the hidden layer");
  if constexpr (I < 6) return k1_group_bcast<I>(x);
  else if constexpr (I == 6) return r0;
  else if constexpr (I == 7) return r1;
  else if constexpr (I < 16) return k1_group_bcast<I - 8>(z.x);
  else return k1_group_bcast<I - 16>(z.y);
}
// batch B: both units' running sums advanced by one product per input, in the order of the inputs
template <int B, int K = 0>
__device__ __forceinline__ void fb_hidden_batch(const FbHiddenBatch& w, const double x, const double r0, const double r1, const double2 z, double& s0, double& s1) {
  if constexpr (K < FB_HIDDEN_BATCH) {
    const double v = fb_hidden_input<B * FB_HIDDEN_BATCH + K>(x, r0, r1, z);
    const fb_pair q0 = w.p0[K / 2], q1 = w.p1[K / 2];
    s0 = s0 + ((K & 1) ? q0.y : q0.x) * v, s1 = s1 + ((K & 1) ? q1.y : q1.x) * v;
    fb_hidden_batch<B, K + 1>(w, x, r0, r1, z, s0, s1);
  }
}
// batches B .. the last: each requested when the one before it has been consumed
template <int B>
__device__ __forceinline__ void fb_hidden_rest(const double* __restrict__ hp, const double x, const double r0, const double r1, const double2 z, double& s0, double& s1) {
  if constexpr (B < 24 / FB_HIDDEN_BATCH) {
    const FbHiddenBatch w = fb_hidden_request<B>(hp);
    fb_hidden_batch<B>(w, x, r0, r1, z, s0, s1);
    fb_hidden_rest<B + 1>(hp, x, r0, r1, z, s0, s1);
  }
}
__device__ __forceinline__ double fb_hidden_activation(const double s, const int activation) {
  const double relu = s > 0.0 ? s : 0.0, ht = s > 1.0 ? 1.0 : (s < -1.0 ? -1.0 : s);
  return activation ? ht : relu;
}
// a: fb_law_sectors' result; x, r0, r1: what fb_law took; z: what fb_law_sectors took; w0 / t: batch 0 and the tail, requested by
// the caller ahead of its sector loop (they do not depend on the observation); hp: as fb_hidden_request's.  Called by all 64 lanes.
__device__ __forceinline__ double2 fb_hidden(const double2 a, const double x, const double r0, const double r1, const double2 z,
                                             const FbHiddenBatch& w0, const FbHiddenTail& t, const double* __restrict__ hp, const int activation) {
  double s0 = t.bv0.x, s1 = t.bv1.x;
  fb_hidden_batch<0>(w0, x, r0, r1, z, s0, s1);
  fb_hidden_rest<1>(hp, x, r0, r1, z, s0, s1);
  const double y0 = fb_hidden_activation(s0, activation), y1 = fb_hidden_activation(s1, activation);
  const double ha0 = fb_group_sum(t.bv0.y * y0), hb0 = fb_group_sum(t.bv1.y * y1);
  const double ha1 = fb_group_sum(t.vp0.x * y0), hb1 = fb_group_sum(t.vp1.x * y1);
  return make_double2(a.x + (ha0 + hb0), a.y + (ha1 + hb1));
}

// FB (k_step_feedback: 1, k_step_sector_feedback: 2, k_step_hidden_feedback: 3): a step that is not the last also forms the NEXT
// step's action by the feedback law and hands it over in words 21..23 of the carry record (fb_gains: [N][2][8]; fb_actions / fb_slot:
// the ring and the next step's slot, or nullptr; FB >= 2: fb_sgains, [N][2][16], and fb_sb, the sector bounds; FB 3: fb_hidden,
// [N][16][28], and fb_activation)
// FW (k_fresh_multi / k_fresh_record; with FB: k_fresh_feedback / _sector_feedback / _hidden_feedback, the argument at those
// kernels): a fresh world per reset.  The reset takes the environment's next slot only if it was published
// before this call began (auv_next_world_multi with `fw_call`, else the world just left, counted), binds it through the coherent
// restore_env and hands the descriptor of the slot it actually took on in the carry record; the episode log's world column is
// environment + N * serial of the world the carry record names.
template <bool MULTI, int FB = 0, int FW = 0>
__device__ __forceinline__ void roles_finish_wave_multi(const AuvDev& dk, const int f, const int lane, float* __restrict__ obs_out,
                                                        float* __restrict__ reward_out, uint8_t* __restrict__ done_out, const int step,
                                                        const bool last_step, const unsigned long long tagmix, const unsigned long long tagmix_prev MSTAMP_PARAM,
                                                        const double* __restrict__ fb_gains = nullptr, const void* __restrict__ fb_actions = nullptr,
                                                        const int fb_slot = 0, const double* __restrict__ fb_sgains = nullptr,
                                                        const FbBounds* fb_sb = nullptr, const double* __restrict__ fb_hidden_tab = nullptr,
                                                        const int fb_activation = 0, const unsigned int fw_call = 0u) {
  // (roles_finish_wave with the previous step's outcome from the carry record instead of the arrays, and its own outcome into
  // the record at the end; the arithmetic in between is the very same code)
  const __attribute__((address_space(4))) AuvDev* dc = (const __attribute__((address_space(4))) AuvDev*)dk.self;
  const AuvDev& d = *(const AuvDev*)dc;
  StepTabs st;
  st.cfg.min_cumulative_reward = dc->cfg.min_cumulative_reward, st.cfg.min_goal_distance = dc->cfg.min_goal_distance;
  st.cfg.min_path_progress = dc->cfg.min_path_progress, st.cfg.look_ahead_distance = dc->cfg.look_ahead_distance;
  st.cfg.max_timesteps = dc->cfg.max_timesteps, st.cfg.rewarder = dc->cfg.rewarder, st.cfg.test_mode = dc->cfg.test_mode;
  st.cfg.auto_reset = dc->cfg.auto_reset, st.cfg.n_sensors = dc->cfg.n_sensors, st.cfg.use_lidar = dc->cfg.use_lidar;
  st.cfg.obs_channels = dc->cfg.obs_channels, st.pool_ns = dc->pool_ns;
  st.knot_s = dc->knot_s, st.knot_coef = dc->knot_coef;
  st.info64 = dc->info64, st.nav64 = dc->nav64, st.obs64 = dc->obs64, st.rew_path = dc->rew_path, st.reward64 = dc->reward64;
  st.step_info = dc->step_info, st.episode = dc->episode, st.ep_log = dc->ep_log, st.ep_log_count = dc->ep_log_count;
  st.ep_log_cap = dc->ep_log_cap, st.world_idx = dc->world_idx, st.counters = dc->counters;
  st.fw_serial = nullptr, st.n = dc->n;
  if constexpr (FW) st.fw_serial = dc->fw_serial;
  st.ring_slots = 1, st.ring_slot_host = 0, st.ring_pos = nullptr;
  unsigned long long* const pair_word = dc->pair_word;
  unsigned long long* const k1_pkt = dc->k1_pkt;
  unsigned long long* const nav_hand = dc->nav_hand;
  unsigned long long* const carry = dc->carry;
  const EnvDesc* const env_desc = dc->env_desc;
  const double* const world_scalar = dc->world_scalar;
  double* const state = dc->state;
  uint8_t* const broken = dc->broken;
  const int n_envs = dc->n;
  const int ne = dk.ne, e0 = dk.e0;
  const int g = lane / K1_GROUP, c = lane % K1_GROUP;
  const int er = 8 * (8 * (f / 8) + g) + (f % 8);
  const bool live = er < ne;
  const int e = e0 + (live ? er : ne - 1);
  const int limit = AUV_HOOK_FAULT(dk) ? (1 << 12) : PAIR_POLL_LIMIT;
  int4 cnt;
  double cum_in, cte_sum_in, maxp_in;
  EnvDesc ed;
  unsigned long long* const cw = carry + CARRY_WORDS * (size_t)e;
  if (step == 0) {
    cnt = st.counters[e];
    cum_in = st.info64[8 * (size_t)e + 4], cte_sum_in = st.info64[8 * (size_t)e + 7], maxp_in = st.info64[8 * (size_t)e + 5];
    ed = env_desc[e];
  } else {
    // ---- the previous step's carry: words c, 8 + c, 16 + c of the group's environment ----
    // (idle groups wait for nobody: the record of the environment they shadow -- the launch's last -- belongs to ITS waves, and
    // its finish wave of this step may overwrite it before a foreign reader has looked; they take that environment's table
    // descriptor from the array instead -- possibly a step old, always a valid one: their table reads stay in bounds and their
    // results are dropped)
    unsigned long long v0 = 0ull, v1 = 0ull, v2 = 0ull;
    bool ok = !live;
    for (int polls = 0;; polls++) {
      if (!ok) {
        v0 = __hip_atomic_load(cw + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v1 = __hip_atomic_load(cw + 8 + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v2 = __hip_atomic_load(cw + 16 + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      const unsigned long long xb = roles_group_xor(carry_mix(v1, 8 + c)) ^ roles_group_xor(c < 4 ? carry_mix(v2, 16 + c) : 0ull), mb = roles_group_word(v2, 4);
      ok = !live || (roles_record_ok(v0, c, tagmix_prev) && mb != 0ull && roles_mark(xb ^ tagmix_prev) == mb);
      if (!__any(!ok)) break;
      if ((polls & 31) == 31 && auv_uniform(__hip_atomic_load(dc->abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) return;
      if (polls == limit) {
        if (live && c == 0) auv_st<true>(broken + e, (uint8_t)1);
        roles_give_up(d, e0, ne, 6, lane);
        return;
      }
      __builtin_amdgcn_s_sleep(ROLES_POLL_SLEEP);
    }
    const unsigned long long c6 = roles_group_word(v0, 6), c8 = roles_group_word(v1, 0);
    cnt = make_int4((int)(unsigned)c6, (int)(unsigned)(c6 >> 32), (int)(unsigned)c8, 0);
    cum_in = roles_group_value(v1, 1), maxp_in = roles_group_value(v1, 2), cte_sum_in = roles_group_value(v1, 3);
    unsigned long long w[8];
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = roles_group_word(v1, 4 + i);
#pragma unroll
    for (int i = 0; i < 4; i++) w[4 + i] = roles_group_word(v2, i);
    carry_ed_from(ed, w);
    if (!live) ed = env_desc[e];
  }
  const int w = ed.w;
  TailIn t;
  t.kn0 = ed.kn0, t.nk = ed.nk;
  {
    const double* ws = world_scalar + 8 * (size_t)ed.w;
    t.L = ws[0], t.goal_x = ws[1], t.goal_y = ws[2];
    t.knot_first = st.knot_s[ed.kn0], t.knot_last = st.knot_s[ed.kn0 + ed.nk - 1];
    t.maxp_in = maxp_in;
  }
  const unsigned long long* pk = k1_pkt + 8 * (size_t)e;
  unsigned long long* hd = nav_hand + 8 * (size_t)e;
  // ---- the state packet and the search record of every group (this step's) ----
  unsigned long long vp = 0ull, vh = 0ull;
  bool okp = !live, okh = !live, aborted = false;
  for (int polls = 0;; polls++) {
    if (!okp) vp = __hip_atomic_load(pk + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!okh) vh = __hip_atomic_load(hd + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    okp = !live || roles_record_ok(vp, c, tagmix);
    aborted = live && okp && (unsigned)roles_group_word(vp, 6) == ROLES_ABORT_COUNTER;
    okh = !live || aborted || roles_record_ok(vh, c, tagmix);
    if (!__any(!(okp && okh))) break;
    if (polls == limit) {
      if (live && c == 0) auv_st<true>(broken + e, (uint8_t)1);
      roles_give_up(d, e0, ne, 3, lane);
      return;
    }
    __builtin_amdgcn_s_sleep(ROLES_POLL_SLEEP);
  }
  if (__any(aborted)) return;
  t.px = roles_group_value(vp, 0), t.py = roles_group_value(vp, 1), t.psi = roles_group_value(vp, 2);
  t.u = roles_group_value(vp, 3), t.v = roles_group_value(vp, 4), t.r = roles_group_value(vp, 5);
  cnt.y = (int)(unsigned)roles_group_word(vp, 6);
  t.nr.A = make_double2(roles_group_value(vh, 0), roles_group_value(vh, 1));
  t.nr.B = make_double2(roles_group_value(vh, 2), roles_group_value(vh, 3));
  t.nr.cum = roles_group_value(vh, 4);
  NavOut no;
  no.rew_path = no.reached = no.goal = no.progress = no.u = no.v = no.r = no.cte100 = no.maxp = 0.0;
  unsigned long long word = live ? __hip_atomic_load(pair_word + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
  no = nav_tail<K1_GROUP>(st, e, c, live, t, obs_out);
  if (live && c < 6) state[(size_t)c * (size_t)n_envs + e] = __longlong_as_double((long long)vp);
  for (int polls = 0;; polls++) {
    if (!__any(word == PAIR_EMPTY)) break;
    if (word == PAIR_EMPTY) word = __hip_atomic_load(pair_word + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!__any(word == PAIR_EMPTY)) break;
    if (polls == limit) {
      if (live && c == 0) auv_st<true>(broken + e, (uint8_t)1);
      roles_give_up(d, e0, ne, 1, lane);
      return;
    }
    __builtin_amdgcn_s_sleep(ROLES_POLL_SLEEP);
  }
  MSTAMP_IF(live && c == 0, e, 14);
  int do_reset = 0;
  double co[2] = {0.0, 0.0};
  if (live && c == 0) {
    __hip_atomic_store(pair_word + e, PAIR_EMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(k1_pkt + 8 * (size_t)e + 7, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(hd + 7, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    RewardIn in;
    const int collision = word == PAIR_COLLISION;
    in.closeness_reward = collision ? 0.0 : __longlong_as_double((long long)word);
    in.path_reward = no.rew_path, in.reached = no.reached, in.goal = no.goal, in.progress = no.progress;
    in.u = no.u, in.v = no.v, in.yaw_rate = no.r;
    in.cum = cum_in;
    in.cte100 = no.cte100, in.cte_sum = cte_sum_in;
    st.info64[8 * (size_t)e] = collision;
    if constexpr (FW) do_reset = reward_apply(st, e, collision, cnt, in, reward_out, done_out, false, co, w);
    else do_reset = reward_apply(st, e, collision, cnt, in, reward_out, done_out, false, co);
  }
  unsigned long long m = __ballot(do_reset);
  const unsigned long long m_reset = m;
  int w_next = w;                                          // (FW: the slot this group's environment was restored into)
  while (m) {
    const int src = __ffsll((long long)m) - 1;
    m &= m - 1;
    const int er2 = auv_uniform(__shfl(e, src, AUV_WAVE));
    const int wr = auv_uniform(__shfl(w, src, AUV_WAVE)), ep = auv_uniform(__shfl(cnt.z, src, AUV_WAVE));
    const AuvDev* dp = dk.self;
    asm volatile("" : "+s"(dp));
    const AuvDev& dr = *(const AuvDev*)(const __attribute__((address_space(4))) AuvDev*)dp;
    if constexpr (FW) {
      int w2 = 0;
      if (lane == 0) w2 = auv_next_world_multi(dr, wr, fw_call);
      w2 = auv_uniform(w2);
      w_next = lane / K1_GROUP == src / K1_GROUP ? w2 : w_next;
      restore_env<true, true>(dr, er2, w2, lane, ep, obs_out);
    } else {
      restore_env<false, true>(dr, er2, (int)(((long long)wr + dr.n) % dr.n_worlds), lane, ep, obs_out);
    }
  }
  if (last_step) return;                                   // (the launch that follows reads the arrays, behind a kernel boundary)
  // ---- this step's outcome into the carry record ----
  // every store the next step's waves depend on -- the marks taken down, a restored environment's mover / nearby rows -- is
  // complete before the record can be seen
  auv_stores_done();
  unsigned long long w0, w1, w2;
  {
    // group lane 0 ran the reward phase: its counters, cumulative reward, cross-track sum and the tail's maximum progress
    const int cx = __shfl(cnt.x, 0, K1_GROUP), cy = __shfl(cnt.y, 0, K1_GROUP), cz = __shfl(cnt.z, 0, K1_GROUP);
    const double cum = __shfl(co[0], 0, K1_GROUP), cte = __shfl(co[1], 0, K1_GROUP), maxp = __shfl(no.maxp, 0, K1_GROUP);
    w0 = c < 6 ? vp : (unsigned long long)(unsigned)cx | ((unsigned long long)(unsigned)cy << 32);
    w1 = c == 0 ? (unsigned long long)(unsigned)cz
                : (c == 1 ? (unsigned long long)__double_as_longlong(cum)
                          : (c == 2 ? (unsigned long long)__double_as_longlong(maxp) : (c == 3 ? (unsigned long long)__double_as_longlong(cte) : carry_ed_word(ed, c - 4))));
    w2 = c < 4 ? carry_ed_word(ed, 4 + c) : 0ull;
  }
  if (m_reset & (0xffull << (8 * g))) {
    // this group's environment was restored: what the restore has just written (this wave's own stores, complete: read past L1)
    const size_t n = (size_t)n_envs;
    const int4 rc = make_int4(0, 0, __shfl(cnt.z, 0, K1_GROUP), 0);
    const EnvDesc ne_ = auv_make_desc<true>(d, FW ? w_next : (int)(((long long)w + d.n) % d.n_worlds));
    const double sv = c < 6 ? __hip_atomic_load(state + (size_t)c * n + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    const double iv = (c >= 1 && c <= 3) ? __hip_atomic_load(st.info64 + 8 * (size_t)e + (c == 1 ? 4 : (c == 2 ? 5 : 7)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    w0 = c < 6 ? (unsigned long long)__double_as_longlong(sv) : 0ull;          // counters x = y = 0
    w1 = c == 0 ? (unsigned long long)(unsigned)rc.z : (c <= 3 ? (unsigned long long)__double_as_longlong(iv) : carry_ed_word(ne_, c - 4));
    w2 = c < 4 ? carry_ed_word(ne_, 4 + c) : 0ull;
  }
  const unsigned long long ma = roles_mark(roles_group_xor(c < 7 ? w0 : 0ull) ^ tagmix);
  const unsigned long long mb = roles_mark(roles_group_xor(carry_mix(w1, 8 + c)) ^ roles_group_xor(c < 4 ? carry_mix(w2, 16 + c) : 0ull) ^ tagmix);
  unsigned long long w2hi = 0ull;                           // words 21..23 (FB; else written as zero)
  if constexpr (FB) {
    // the next step's action.  x_0..5 are read back from the OBS64 row: the tail forms them in group lane 0 and keeps them to
    // itself, a restored environment's come from its reset row -- either way this wave's own stores, complete (above), so one
    // agent-scope load past L1 serves both cases.  x_7, the ring's action of step t + 1, is known at launch: it is fetched HERE, in
    // the same trip as the row and the gains, so that p_6 + p_7 is formed inside the one sum and the association is the law's (the
    // dynamics wave adding p_7 to a finished sum would be another association).
    // (the environment's index and the tables laundered / fetched HERE: addresses formed ahead of the restore loop are held across
    // it in vector registers the wave does not have -- two spilled pairs and a private segment for every wave of the launch)
    int ef = e;
    asm volatile("" : "+v"(ef));
    const AuvDev* dp = dk.self;
    asm volatile("" : "+s"(dp));
    const AuvDev& df = *(const AuvDev*)(const __attribute__((address_space(4))) AuvDev*)dp;
    const int S = df.cfg.n_sensors;
    const double x = c < 6 ? __hip_atomic_load(df.obs64 + (size_t)ef * (6 + S) + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    const double g0 = fb_gains[16 * (size_t)ef + c], g1 = fb_gains[16 * (size_t)ef + 8 + c];
    double r0 = 0.0, r1 = 0.0;
    if (fb_actions) k1_action(dk, fb_actions, ef, &r0, &r1, fb_slot);
    double2 a = fb_law(c, x, g0, g1, r0, r1);
    if constexpr (FB >= 2) {
      // the sector inputs: the closeness columns of the same row.  The sweep stored them write-through and drained them before it
      // published the pair word this wave has polled (k2_back, pair_publish_lidar); a restored environment's are this wave's own
      // completed stores -- agent-scope loads past L1 serve both, like x above.  Addresses from the laundered index and descriptor.
      const double* hp = fb_sgains + 32 * (size_t)ef + c;
      const double2 h0 = make_double2(hp[0], hp[8]), h1 = make_double2(hp[16], hp[24]);      // (requested ahead of the sector loop)
      if constexpr (FB == 3) {
        // the hidden layer: its first batch of weights, the biases and the output rows are requested ahead of the sector loop too
        // (they do not depend on the observation), the other two batches behind it, where their registers are free
        const double* wp = fb_hidden_tab + (size_t)(16 * FB_HIDDEN_ROW) * (size_t)ef + FB_HIDDEN_ROW * c;
        const FbHiddenBatch w0 = fb_hidden_request<0>(wp);
        const FbHiddenTail wt = fb_hidden_request_tail(wp);
        const double2 z = fb_sector_pair<true>(df.obs64 + (size_t)ef * (6 + S) + 6, fb_ranges(*fb_sb, c));
        a = fb_hidden(fb_law_sectors(a, z, h0, h1), x, r0, r1, z, w0, wt, wp, fb_activation);
      } else {
        const double2 z = fb_sector_pair<true>(df.obs64 + (size_t)ef * (6 + S) + 6, fb_ranges(*fb_sb, c));
        a = fb_law_sectors(a, z, h0, h1);
      }
    }
    const unsigned long long wa = (unsigned long long)__double_as_longlong(a.x), wb = (unsigned long long)__double_as_longlong(a.y);
    // (the mark is built like the state line's: a checksum of its payload mixed with the step's number, loaded with it in one request)
    w2hi = c == 5 ? wa : (c == 6 ? wb : (c == 7 ? roles_mark(wa ^ wb ^ tagmix) : 0ull));
  }
  if (live) {
    __hip_atomic_store(cw + c, c < 7 ? w0 : ma, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(cw + 8 + c, w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(cw + 16 + c, c < 4 ? w2 : (c == 4 ? mb : w2hi), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The descriptor is the kernel's FIRST argument: offset 0 of the argument segment.  Read through the segment pointer (laundered, so that
// the compiler cannot prove the loads safe to speculate) its fields are fetched where a role uses them -- not every field any role
// uses, in four or five dependent batches with scalar registers spilled in between, at the top of every wave (0.8 us of a 6 us search
// wave: tools/multi_stamps.py).  k_step_multi: 176 -> 186 M env-steps/s at 64 steps per launch, 160 -> 171 M over the driver's 20-step
// window; k_step_roles: 151 -> 150 M on four chains, so the one-step launch keeps the by-value reference
// (profiles/r05/ab_descriptor_through_segment_pointer.jsonl).
#define AUV_KERNARG_DESC(name)                                                                                                                       \
  const __attribute__((address_space(4))) void* name##_kp_ = (const __attribute__((address_space(4))) void*)__builtin_amdgcn_kernarg_segment_ptr(); \
  asm volatile("" : "+s"(name##_kp_));                                                                                                               \
  const AuvDev& name = *(const AuvDev*)(const __attribute__((address_space(4))) AuvDev*)name##_kp_

__global__ void __launch_bounds__(AUV_WAVE, AUV_K23_MIN_WAVES) k_step_multi(AuvDev dk, const void* __restrict__ actions, float* __restrict__ obs_out,
                                                                           float* __restrict__ reward_out, uint8_t* __restrict__ done_out,
                                                                           const int n_steps, const int first_slot, const int n_slots,
                                                                           const unsigned long long seq0, const int lead_dyn, const int lag_fin, const unsigned magic_c) {
  AUV_KERNARG_DESC(d);
#define STEP_MULTI_REC 0
#define STEP_MULTI_FB 0
#include "k_step_multi_body.inc"
#undef STEP_MULTI_FB
#undef STEP_MULTI_REC
}

// The recording launch (auv_step_multi_record): k_step_multi with the three output rows of step k at k * stride.  A kernel of its
// own, so that the plain launch keeps its argument list and its code (the body is the same text: k_step_multi_body.inc).
__global__ void __launch_bounds__(AUV_WAVE, AUV_K23_MIN_WAVES) k_step_record(AuvDev dk, const void* __restrict__ actions, float* __restrict__ obs_out,
                                                                            float* __restrict__ reward_out, uint8_t* __restrict__ done_out,
                                                                            const int n_steps, const int first_slot, const int n_slots,
                                                                            const unsigned long long seq0, const int lead_dyn, const int lag_fin, const unsigned magic_c,
                                                                            const unsigned long long obs_stride, const unsigned long long reward_stride,
                                                                            const unsigned long long done_stride) {
  AUV_KERNARG_DESC(d);
#define STEP_MULTI_REC 1
#define STEP_MULTI_FB 0
#include "k_step_multi_body.inc"
#undef STEP_MULTI_FB
#undef STEP_MULTI_REC
}

// A fresh world on every reset in launches of several steps (auv_fresh_worlds_multi): k_step_multi and k_step_record whose finish
// wave resets through the gated slot choice (STEP_MULTI_FW; roles_finish_wave_multi<.., FW>).  fw_call: the number of the call this
// launch belongs to.  Two further inclusions of the body: the other six keep their argument lists and their code.
__global__ void __launch_bounds__(AUV_WAVE, AUV_K23_MIN_WAVES) k_fresh_multi(AuvDev dk, const void* __restrict__ actions, float* __restrict__ obs_out,
                                                                            float* __restrict__ reward_out, uint8_t* __restrict__ done_out,
                                                                            const int n_steps, const int first_slot, const int n_slots,
                                                                            const unsigned long long seq0, const int lead_dyn, const int lag_fin, const unsigned magic_c,
                                                                            const unsigned int fw_call) {
  AUV_KERNARG_DESC(d);
#define STEP_MULTI_REC 0
#define STEP_MULTI_FB 0
#define STEP_MULTI_FW 1
#include "k_step_multi_body.inc"
#undef STEP_MULTI_FW
#undef STEP_MULTI_FB
#undef STEP_MULTI_REC
}

__global__ void __launch_bounds__(AUV_WAVE, AUV_K23_MIN_WAVES) k_fresh_record(AuvDev dk, const void* __restrict__ actions, float* __restrict__ obs_out,
                                                                             float* __restrict__ reward_out, uint8_t* __restrict__ done_out,
                                                                             const int n_steps, const int first_slot, const int n_slots,
                                                                             const unsigned long long seq0, const int lead_dyn, const int lag_fin, const unsigned magic_c,
                                                                             const unsigned long long obs_stride, const unsigned long long reward_stride,
                                                                             const unsigned long long done_stride, const unsigned int fw_call) {
  AUV_KERNARG_DESC(d);
#define STEP_MULTI_REC 1
#define STEP_MULTI_FB 0
#define STEP_MULTI_FW 1
#include "k_step_multi_body.inc"
#undef STEP_MULTI_FW
#undef STEP_MULTI_FB
#undef STEP_MULTI_REC
}

// The closed-loop launch (auv_step_feedback): k_step_record whose action of step t is the affine feedback law (fb_law, above) of the
// OBS64 row step t - 1 left, formed by that step's finish wave and handed to this step's dynamics wave in words 21..23 of the carry
// record.  A third inclusion of the body, so that the open-loop kernels keep their argument lists and their code.  gains: [N][2][8]
// fp64; actions: the ring (x_7) or nullptr; act_rec: [n_steps][N][2] fp64 or nullptr.
__global__ void __launch_bounds__(AUV_WAVE, AUV_K23_MIN_WAVES) k_step_feedback(AuvDev dk, const void* __restrict__ actions, float* __restrict__ obs_out,
                                                                              float* __restrict__ reward_out, uint8_t* __restrict__ done_out,
                                                                              const int n_steps, const int first_slot, const int n_slots,
                                                                              const unsigned long long seq0, const int lead_dyn, const int lag_fin, const unsigned magic_c,
                                                                              const unsigned long long obs_stride, const unsigned long long reward_stride,
                                                                              const unsigned long long done_stride, const double* __restrict__ gains,
                                                                              double* __restrict__ act_rec) {
  AUV_KERNARG_DESC(d);
#define STEP_MULTI_REC 1
#define STEP_MULTI_FB 1
#include "k_step_multi_body.inc"
#undef STEP_MULTI_FB
#undef STEP_MULTI_REC
}

// The closed-loop launch with LiDAR sector inputs (auv_step_feedback_sectors): k_step_feedback whose law also sees the closeness
// columns of the OBS64 row, as at most 16 sector maxima (fb_sector_pair, fb_law_sectors).  A fourth inclusion of the body: the other
// three keep their argument lists and their code.  sgains: [N][2][16] fp64; sb: the bounds, by value (wave-uniform: scalar registers).
__global__ void __launch_bounds__(AUV_WAVE, AUV_K23_MIN_WAVES) k_step_sector_feedback(AuvDev dk, const void* __restrict__ actions, float* __restrict__ obs_out,
                                                                                      float* __restrict__ reward_out, uint8_t* __restrict__ done_out,
                                                                                      const int n_steps, const int first_slot, const int n_slots,
                                                                                      const unsigned long long seq0, const int lead_dyn, const int lag_fin, const unsigned magic_c,
                                                                                      const unsigned long long obs_stride, const unsigned long long reward_stride,
                                                                                      const unsigned long long done_stride, const double* __restrict__ gains,
                                                                                      double* __restrict__ act_rec, const double* __restrict__ sgains,
                                                                                      const FbBounds sb) {
  AUV_KERNARG_DESC(d);
#define STEP_MULTI_REC 1
#define STEP_MULTI_FB 2
#include "k_step_multi_body.inc"
#undef STEP_MULTI_FB
#undef STEP_MULTI_REC
}

// The closed-loop launch with one hidden layer in the law (auv_step_feedback_hidden): k_step_sector_feedback whose action also takes
// 16 hidden units over the 24 inputs the law already holds (fb_hidden).  A fifth inclusion of the body: the other four keep their
// argument lists and their code.  hidden: [N][16][28] fp64; activation: 0 relu, 1 hard tanh (wave-uniform).
__global__ void __launch_bounds__(AUV_WAVE, AUV_K23_MIN_WAVES) k_step_hidden_feedback(AuvDev dk, const void* __restrict__ actions, float* __restrict__ obs_out,
                                                                                      float* __restrict__ reward_out, uint8_t* __restrict__ done_out,
                                                                                      const int n_steps, const int first_slot, const int n_slots,
                                                                                      const unsigned long long seq0, const int lead_dyn, const int lag_fin, const unsigned magic_c,
                                                                                      const unsigned long long obs_stride, const unsigned long long reward_stride,
                                                                                      const unsigned long long done_stride, const double* __restrict__ gains,
                                                                                      double* __restrict__ act_rec, const double* __restrict__ sgains,
                                                                                      const FbBounds sb, const double* __restrict__ hidden, const int activation) {
  AUV_KERNARG_DESC(d);
#define STEP_MULTI_REC 1
#define STEP_MULTI_FB 3
#include "k_step_multi_body.inc"
#undef STEP_MULTI_FB
#undef STEP_MULTI_REC
}

// The closed-loop launches on a fresh world per reset (auv_fresh_worlds_multi(h, 2)): the three kernels above with the gated slot
// choice of k_fresh_record (STEP_MULTI_FB 1 / 2 / 3 with STEP_MULTI_FW 1), `fw_call` last.  Three further inclusions of the body: the
// other ten kernels of this file keep their argument lists and their code.
// Why the action handed over at a reset step is the law of the world actually bound -- with nothing added to what FB and FW each
// already rely on (roles_finish_wave_multi<true, FB, 1>):
//   * the restore loop writes the environment's OBS64 row -- all 6 + S columns -- from the reset row of slot w2, which is what
//     auv_next_world_multi returned: the next slot if it was published before this call began, else (counted) the world just left.
//     restore_env<true, true> reads that reset row with agent-scope loads in either case; the stores are THIS wave's;
//   * auv_stores_done() stands between the restore loop and the FB block, and the FB block reads x_0..5 (FB >= 2: the closeness
//     columns too) back from that row with agent-scope loads past L1 -- the argument of the cycling bank's closed loop, which does
//     not ask where the restore took the row from.  Without a reset the row is the tail's and the sweep's, as there;
//   * the carry record's descriptor words are auv_make_desc<true>(w_next), w_next = w2 of the group whose environment was restored:
//     the next step's sweep, search and finish waves read the tables of the slot whose reset row the action was formed from, and a
//     slot taken has a stamp below this call's number, so plain loads of its tables are sound for the rest of the launch
//     (auv_next_world_multi);
//   * words 21..23 carry the action and a mark mixed with the step's number as before; the dynamics wave accepts the record only
//     when both marks are the previous step's.  Step 0 forms the law from the arrays behind the kernel boundary, as before.
__global__ void __launch_bounds__(AUV_WAVE, AUV_K23_MIN_WAVES) k_fresh_feedback(AuvDev dk, const void* __restrict__ actions, float* __restrict__ obs_out,
                                                                               float* __restrict__ reward_out, uint8_t* __restrict__ done_out,
                                                                               const int n_steps, const int first_slot, const int n_slots,
                                                                               const unsigned long long seq0, const int lead_dyn, const int lag_fin, const unsigned magic_c,
                                                                               const unsigned long long obs_stride, const unsigned long long reward_stride,
                                                                               const unsigned long long done_stride, const double* __restrict__ gains,
                                                                               double* __restrict__ act_rec, const unsigned int fw_call) {
  AUV_KERNARG_DESC(d);
#define STEP_MULTI_REC 1
#define STEP_MULTI_FB 1
#define STEP_MULTI_FW 1
#include "k_step_multi_body.inc"
#undef STEP_MULTI_FW
#undef STEP_MULTI_FB
#undef STEP_MULTI_REC
}

__global__ void __launch_bounds__(AUV_WAVE, AUV_K23_MIN_WAVES) k_fresh_sector_feedback(AuvDev dk, const void* __restrict__ actions, float* __restrict__ obs_out,
                                                                                       float* __restrict__ reward_out, uint8_t* __restrict__ done_out,
                                                                                       const int n_steps, const int first_slot, const int n_slots,
                                                                                       const unsigned long long seq0, const int lead_dyn, const int lag_fin, const unsigned magic_c,
                                                                                       const unsigned long long obs_stride, const unsigned long long reward_stride,
                                                                                       const unsigned long long done_stride, const double* __restrict__ gains,
                                                                                       double* __restrict__ act_rec, const double* __restrict__ sgains,
                                                                                       const FbBounds sb, const unsigned int fw_call) {
  AUV_KERNARG_DESC(d);
#define STEP_MULTI_REC 1
#define STEP_MULTI_FB 2
#define STEP_MULTI_FW 1
#include "k_step_multi_body.inc"
#undef STEP_MULTI_FW
#undef STEP_MULTI_FB
#undef STEP_MULTI_REC
}

__global__ void __launch_bounds__(AUV_WAVE, AUV_K23_MIN_WAVES) k_fresh_hidden_feedback(AuvDev dk, const void* __restrict__ actions, float* __restrict__ obs_out,
                                                                                       float* __restrict__ reward_out, uint8_t* __restrict__ done_out,
                                                                                       const int n_steps, const int first_slot, const int n_slots,
                                                                                       const unsigned long long seq0, const int lead_dyn, const int lag_fin, const unsigned magic_c,
                                                                                       const unsigned long long obs_stride, const unsigned long long reward_stride,
                                                                                       const unsigned long long done_stride, const double* __restrict__ gains,
                                                                                       double* __restrict__ act_rec, const double* __restrict__ sgains,
                                                                                       const FbBounds sb, const double* __restrict__ hidden, const int activation,
                                                                                       const unsigned int fw_call) {
  AUV_KERNARG_DESC(d);
#define STEP_MULTI_REC 1
#define STEP_MULTI_FB 3
#define STEP_MULTI_FW 1
#include "k_step_multi_body.inc"
#undef STEP_MULTI_FW
#undef STEP_MULTI_FB
#undef STEP_MULTI_REC
}

// Behind a closed-loop launch: k_record_last where any of the three records may be missing (a missing one was written in place)
__global__ void __launch_bounds__(256) k_feedback_last(const float* __restrict__ obs_last, const float* __restrict__ reward_last,
                                                       const uint8_t* __restrict__ done_last, float* __restrict__ obs, float* __restrict__ reward,
                                                       uint8_t* __restrict__ done, const int e0, const int ne, const int D, const int32_t* __restrict__ abort_flag) {
  if (*abort_flag) return;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t o0 = (size_t)e0 * (size_t)D;
  if (obs_last && i < (size_t)ne * (size_t)D) obs[o0 + i] = obs_last[o0 + i];
  if (reward_last && i < (size_t)ne) reward[e0 + i] = reward_last[e0 + i];
  if (done_last && i < (size_t)ne) done[e0 + i] = done_last[e0 + i];
}

// Behind a recording launch, on its stream: the record's LAST row of the slice [e0, e0 + ne) into the handle-wide obs / reward / done
// buffers, which hold the last step's values after every kind of step.  obs_last == nullptr: the launch kept no observation record
// and wrote obs itself.  Nothing is copied behind an aborted launch (rows that were not reached hold what the caller passed).
__global__ void __launch_bounds__(256) k_record_last(const float* __restrict__ obs_last, const float* __restrict__ reward_last,
                                                     const uint8_t* __restrict__ done_last, float* __restrict__ obs, float* __restrict__ reward,
                                                     uint8_t* __restrict__ done, const int e0, const int ne, const int D, const int32_t* __restrict__ abort_flag) {
  if (*abort_flag) return;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t o0 = (size_t)e0 * (size_t)D;
  if (obs_last && i < (size_t)ne * (size_t)D) obs[o0 + i] = obs_last[o0 + i];
  if (i < (size_t)ne) reward[e0 + i] = reward_last[e0 + i], done[e0 + i] = done_last[e0 + i];
}

// ---- inside a captured graph of several steps: reward / done / auto-reset of step t and Vessel.step of step t + 1
// in ONE launch (the actions of an open-loop stretch are in the ring already, so nothing sits between the two).
// Lanes <-> environments for both: the scalar form of the dynamics (k1_env: the same operations in the same order
// as the eight-lane kernel, bit-identical) has the same dependent chain, and 64 of them share a wave.
__global__ void __launch_bounds__(AUV_WAVE) k31_reward_dyn(AuvDev d, const void* __restrict__ actions, float* __restrict__ obs_out,
                                                           float* __restrict__ reward_out, uint8_t* __restrict__ done_out) {
  const int lane = threadIdx.x;
  const int e = blockIdx.x * AUV_WAVE + lane;
  int do_reset = 0, w = 0;
  int4 cnt = make_int4(0, 0, 0, 0);
  if (e < d.n) {
    cnt = d.counters[e];
    w = d.world_idx[e];
    const int collision = d.collision[e];
    d.info64[8 * (size_t)e] = collision;
    do_reset = reward_block(d, e, collision, cnt, false, 0.0, nullptr, reward_out, done_out, false);
  }
  unsigned long long m = __ballot(do_reset);
  const bool any_reset = m != 0;
  while (m) {
    const int src = __ffsll((long long)m) - 1;
    m &= m - 1;
    const int er = auv_uniform(__shfl(e, src, AUV_WAVE));
    const int wr = auv_uniform(__shfl(w, src, AUV_WAVE)), ep = __shfl(cnt.z, src, AUV_WAVE);
    restore_env(d, er, auv_next_world_wave(d, wr, lane), lane, ep, obs_out);
  }
  // a restored environment's state was written by lane 0, its dynamics below read it from another lane
  if (any_reset) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  if (e < d.n) k1_env(d, e, actions, true);
}

// ---- load-time probe of what the in-launch hand-overs rely on ----------------------------------------------------
// The one-launch shape lets a wave poll for a word that a workgroup with a SMALLER index of the same
// launch stores.  That terminates if workgroups are dispatched in index order (a poller's producer is resident or
// done by the time the poller gets a slot) -- what gfx950 does, but HIP does not promise it.  k_probe_order has the
// step's structure without its arithmetic: `np` producers (a short wait, then an sc1 word each), behind them `nc`
// consumers that poll their producer's word and publish a word of their own, a third generation that polls the
// second's and publishes, and nc / 8 waves of a fourth that poll eight words of each earlier generation -- like
// dynamics / sweep / search / finish, every workgroup one wave with the step's LDS footprint, and several times more
// workgroups than the chip has slots.  Any poll that runs out (bounded: ~20 ms) counts a failure; the host then keeps
// the handle on the three-launch shape (auv_capi.hip: probe_dispatch_order).  `words`: np + 2 nc of them, zeroed.
__global__ void __launch_bounds__(AUV_WAVE) k_probe_order(unsigned int* __restrict__ words, int np, int nc, unsigned int tag,
                                                          unsigned int* __restrict__ failures) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int b = (int)blockIdx.x, lane = threadIdx.x;
  if (lane == 0) smem[0] = 1;   // (touch the allocation so that it is not optimised away)
  unsigned int* mine = words + b;
  const unsigned int* src = nullptr;
  if (b >= np + 2 * nc) {                                      // fourth generation: eight of each of the others
    const int q = b - np - 2 * nc;
    if (lane < 8) src = words + np + nc + 8 * q + lane;
    else if (lane < 16) src = words + np + 8 * q + (lane - 8);
    else if (lane < 24) src = words + (8 * q + (lane - 16)) % np;
  } else if (b >= np + nc) src = words + np + (b - np - nc);   // third generation: its own second-generation wave
  else if (b >= np) src = words + (b - np) % np;               // second generation: one of the producers
  if (b >= np) {
    int polls = 0;
    for (;;) {
      const bool there = !src || __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == tag;
      if (!__any(!there)) break;
      if (++polls == (1 << 14)) {
        if (lane == 0) atomicAdd(failures, 1u);
        return;
      }
      __builtin_amdgcn_s_sleep(32);
    }
  } else {
    __builtin_amdgcn_s_sleep(40), __builtin_amdgcn_s_sleep(40);   // ~2 us, like the dynamics' chain
  }
  if (lane == 0 && b < np + 2 * nc) __hip_atomic_store(mine, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a wave that does nothing for `ticks` of the 100 MHz wall clock (auv_streams_overlap: do two streams run side by side?)
__global__ void k_spin(unsigned long long ticks) {
  const unsigned long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

// ---- rendezvous of the sub-batch chains with the caller's stream, on the device (auv_step_async / auv_step_wait,
// AUV_RDV_DEVICE) ----------------------------------------------------------------------------------------------------
// VecEnv.step_async / step_wait (scripts/run.py:293-296) order K chains on K streams against the stream the actions
// come from and the results go to.  With HIP events that is a record + K waits before the step and K records + K waits
// behind it, each hop a barrier packet the command processors resolve in ~8 us.  Here the hops are one-wave kernels
// and two words in device memory:
//   caller's stream   k_rdv_publish(ready, t)   behind whatever produced the actions: "the actions of step t are there"
//   chain i's stream  k_rdv_wait(ready, t)      in front of its launch of step t (holds ONE wave slot, not a launch's)
//                     k_rdv_arrive(done)        behind it: "chain i has finished a step"
//   caller's stream   k_rdv_wait(done, target)  in step_wait: all chains have arrived
// Visibility rides on the kernel boundaries: the producer's kernel has ended (release) before the publish kernel
// starts, the waiting kernel ends before the chain's step starts (acquire); likewise behind the step.  Every waiter
// waits for something that was SUBMITTED before it, so streams sharing a hardware queue (FIFO) cannot deadlock; the
// waits are bounded by the wall clock all the same and report through pair_error (4: actions, 5: chains).
__global__ void k_rdv_publish(unsigned long long* word, unsigned long long seq) {
  if (threadIdx.x == 0) __hip_atomic_store(word, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ void k_rdv_arrive(unsigned long long* word) {
  if (threadIdx.x == 0) __hip_atomic_fetch_add(word, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ void k_rdv_wait(const unsigned long long* word, unsigned long long target, int32_t* err, int code, unsigned long long limit_ticks,
                           int32_t* abort_flag, int32_t* report) {
  if (threadIdx.x != 0) return;
  const unsigned long long t0 = wall_clock64();                    // 100 MHz
  int polls = 0;
  while (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
    if (wall_clock64() - t0 > limit_ticks) {
      // A chain's gate that runs out (abort_flag given: code 4) must not let its step run on actions that may not be there:
      // the device-wide abort flag goes up FIRST, so the launch behind this kernel -- and every launch queued behind it, on
      // any stream -- hands out ABORT packets and leaves its environments untouched (k_step_roles), exactly as behind a
      // hand-over time-out.  The code is published only if no other report is pending: a hand-over time-out (codes 1-3)
      // reported by an earlier launch must reach the host as such -- its recovery is the superset.
      if (abort_flag) __hip_atomic_store(abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      // (arbitrated on a DEVICE word, `report`: no read-modify-write on the mapped host word)
      if (__hip_atomic_exchange(report, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
        __hip_atomic_store(err, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return;
    }
    // eager for the first few microseconds (a step's rendezvous), then a poll per ~2 us: a chain's gate may sit here for as long
    // as the caller's stream is busy with something else -- a PPO update between two rollouts -- and should not cost anything
    if (++polls < 256) __builtin_amdgcn_s_sleep(2);
    else __builtin_amdgcn_s_sleep(127);
  }
}

}  // namespace

void auv_launch_rdv_publish(unsigned long long* word, unsigned long long seq, hipStream_t st) {
  hipLaunchKernelGGL(k_rdv_publish, dim3(1), dim3(AUV_WAVE), 0, st, word, seq);
}
void auv_launch_rdv_arrive(unsigned long long* word, hipStream_t st) { hipLaunchKernelGGL(k_rdv_arrive, dim3(1), dim3(AUV_WAVE), 0, st, word); }
void auv_launch_rdv_wait(const unsigned long long* word, unsigned long long target, int32_t* err, int code, double limit_s, int32_t* abort_flag,
                         int32_t* report, hipStream_t st) {
  hipLaunchKernelGGL(k_rdv_wait, dim3(1), dim3(AUV_WAVE), 0, st, word, target, err, code, (unsigned long long)(limit_s * 1e8), abort_flag, report);
}

void auv_launch_spin(unsigned long long ticks, hipStream_t st) { hipLaunchKernelGGL(k_spin, dim3(1), dim3(AUV_WAVE), 0, st, ticks); }

hipError_t auv_launch_probe(unsigned int* words, int np, int nc, unsigned int tag, unsigned int* failures, uint32_t lds, hipStream_t st) {
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)k_probe_order, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_probe_order, dim3(np + 2 * nc + nc / 8), dim3(AUV_WAVE), lds, st, words, np, nc, tag, failures);
  return hipGetLastError();
}

void auv_launch_k31(const AuvDev& d0, const void* actions, int dtype, float* obs, float* reward, uint8_t* done, hipStream_t st) {
  AuvDev d = d0;
  d.act_f64 = dtype == AUV_F64;
  const dim3 grid((d.n + AUV_WAVE - 1) / AUV_WAVE), block(AUV_WAVE);
  hipLaunchKernelGGL(k31_reward_dyn, grid, block, 0, st, d, actions, obs, reward, done);
}

// the navigation role keeps its chunk list at the start of the wave's slice
bool auv_k23_ok(const AuvDev& d) { return NAV_SCRATCH_BYTES(d.nch_max) <= k2_slice_bytes(d); }

// K2 + K3-nav side by side: ONE wave per workgroup, so a wave slot is handed on the moment an environment's sweep
// ends -- the navigation workgroups queued behind the LiDAR ones start (and end) earlier.
void auv_launch_k23(const AuvDev& d, float* obs, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
  const size_t lds = k2_slice_bytes(d);
  hipExtLaunchKernelGGL(k23_lidar_nav, dim3(2 * d.ne), dim3(AUV_WAVE), (uint32_t)lds, st, ev0, ev1, 0, d, obs);
}

// ---- the one-launch step (needs a LiDAR sweep: its word is what the finish wave finishes the step on) ----
bool auv_roles_ok(const AuvDev& d) { return auv_k23_ok(d) && d.cfg.use_lidar; }

void auv_launch_step_roles(const AuvDev& d0, const void* actions, int dtype, float* obs, float* reward, uint8_t* done,
                           hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
  AuvDev d = d0;
  d.act_f64 = dtype == AUV_F64;
  const uint32_t lds = (uint32_t)k2_slice_bytes(d);
  const int nk = 8 * ((d.ne + 63) / 64), nb = 8 * ((d.ne + 7) / 8);
  const dim3 grid(nk + 2 * nb + AUV_HOOK_SKEW(d) + nk), block(AUV_WAVE);
  hipExtLaunchKernelGGL(k_step_roles, grid, block, lds, st, ev0, ev1, 0, d, actions, obs, reward, done);
}

// order: 0 step-major; 1 cohort-pipelined where the slice has whole cohorts for it (lead / lag clamped: auv_multi_geom.h)
void auv_launch_step_multi(const AuvDev& d0, const void* actions, int dtype, float* obs, float* reward, uint8_t* done, int n_steps,
                           int first_slot, int n_slots, unsigned long long seq0, int order, int lead, int lag, hipStream_t st, unsigned int fw_call) {
  AuvDev d = d0;
  d.act_f64 = dtype == AUV_F64;
  d.ring_slots = 1;
  const uint32_t lds = (uint32_t)k2_slice_bytes(d);
  const AuvMultiGeom g = auv_multi_geom(d.ne, n_steps, order, lead, lag);      // (the host has checked that the grid fits)
  const dim3 grid((unsigned)auv_multi_grid(g)), block(AUV_WAVE);
  // fw_call != 0: a fresh world per reset, this launch belongs to multi-step call number fw_call
  if (fw_call)
    hipLaunchKernelGGL(k_fresh_multi, grid, block, lds, st, d, actions, obs, reward, done, n_steps, first_slot, n_slots, seq0, g.lead, g.lag, g.magic, fw_call);
  else
    hipLaunchKernelGGL(k_step_multi, grid, block, lds, st, d, actions, obs, reward, done, n_steps, first_slot, n_slots, seq0, g.lead, g.lag, g.magic);
}

// the recording form: step k's rows at obs_rec + k N D, reward_rec + k N, done_rec + k N (obs_rec == nullptr: no observation record,
// every step writes `obs`); then the last row into obs / reward / done
void auv_launch_step_record(const AuvDev& d0, const void* actions, int dtype, float* obs, float* reward, uint8_t* done, float* obs_rec,
                            float* reward_rec, uint8_t* done_rec, int n_steps, int first_slot, int n_slots, unsigned long long seq0, int order,
                            int lead, int lag, hipStream_t st, unsigned int fw_call) {
  AuvDev d = d0;
  d.act_f64 = dtype == AUV_F64;
  d.ring_slots = 1;
  const uint32_t lds = (uint32_t)k2_slice_bytes(d);
  const AuvMultiGeom g = auv_multi_geom(d.ne, n_steps, order, lead, lag);      // (the host has checked that the grid fits)
  const dim3 grid((unsigned)auv_multi_grid(g)), block(AUV_WAVE);
  const int D = auv_obs_cols(d.cfg, d.pool_ns);
  const unsigned long long n = (unsigned long long)d.n, obs_stride = obs_rec ? n * (unsigned long long)D : 0ull;
  if (fw_call)                                                                   // (as auv_launch_step_multi)
    hipLaunchKernelGGL(k_fresh_record, grid, block, lds, st, d, actions, obs_rec ? obs_rec : obs, reward_rec, done_rec, n_steps, first_slot, n_slots, seq0,
                       g.lead, g.lag, g.magic, obs_stride, n, n, fw_call);
  else
    hipLaunchKernelGGL(k_step_record, grid, block, lds, st, d, actions, obs_rec ? obs_rec : obs, reward_rec, done_rec, n_steps, first_slot, n_slots, seq0,
                       g.lead, g.lag, g.magic, obs_stride, n, n);
  const size_t last = (size_t)(n_steps - 1), items = (size_t)d.ne * (size_t)(obs_rec ? D : 1);
  hipLaunchKernelGGL(k_record_last, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, obs_rec ? obs_rec + last * obs_stride : nullptr,
                     reward_rec + last * n, done_rec + last * n, obs, reward, done, d.e0, d.ne, D, d.abort_flag);
}

// the closed-loop form: the record launch with the gain table, an optional ring and an optional action record; each of the three
// output records may be missing (that output's every step then goes to obs / reward / done, and nothing is copied for it)
// (sector_gains / sector_bounds: nullptr, or [N][2][16] fp64 and the table of 17 -- k_step_sector_feedback is launched instead;
// hidden: nullptr, or with those two the [N][16][28] fp64 block and `activation` -- k_step_hidden_feedback; fw_call != 0: the
// k_fresh_* kernel of the same law)
void auv_launch_step_feedback(const AuvDev& d0, const double* gains, const void* actions, int dtype, float* obs, float* reward, uint8_t* done,
                              float* obs_rec, float* reward_rec, uint8_t* done_rec, double* act_rec, int n_steps, int first_slot, int n_slots,
                              unsigned long long seq0, int order, int lead, int lag, hipStream_t st, const double* sector_gains,
                              const int32_t* sector_bounds, const double* hidden, int activation, unsigned int fw_call) {
  AuvDev d = d0;
  d.act_f64 = dtype == AUV_F64;
  d.ring_slots = 1;
  const uint32_t lds = (uint32_t)k2_slice_bytes(d);
  const AuvMultiGeom g = auv_multi_geom(d.ne, n_steps, order, lead, lag);      // (the host has checked that the grid fits)
  const dim3 grid((unsigned)auv_multi_grid(g)), block(AUV_WAVE);
  const int D = auv_obs_cols(d.cfg, d.pool_ns);
  const unsigned long long n = (unsigned long long)d.n, obs_stride = obs_rec ? n * (unsigned long long)D : 0ull;
  // fw_call != 0: a fresh world per reset, this launch belongs to multi-step call number fw_call (as auv_launch_step_record)
  float* const o = obs_rec ? obs_rec : obs;
  float* const r = reward_rec ? reward_rec : reward;
  uint8_t* const dn = done_rec ? done_rec : done;
  const unsigned long long rs = reward_rec ? n : 0ull, ds = done_rec ? n : 0ull;
  if (hidden) {
    FbBounds sb;
    for (int i = 0; i < 17; i++) sb.b[i] = sector_bounds[i];
    if (fw_call)
      hipLaunchKernelGGL(k_fresh_hidden_feedback, grid, block, lds, st, d, actions, o, r, dn, n_steps, first_slot, n_slots, seq0, g.lead, g.lag, g.magic,
                         obs_stride, rs, ds, gains, act_rec, sector_gains, sb, hidden, activation, fw_call);
    else
      hipLaunchKernelGGL(k_step_hidden_feedback, grid, block, lds, st, d, actions, o, r, dn, n_steps, first_slot, n_slots, seq0, g.lead, g.lag, g.magic,
                         obs_stride, rs, ds, gains, act_rec, sector_gains, sb, hidden, activation);
  } else if (sector_gains) {
    FbBounds sb;
    for (int i = 0; i < 17; i++) sb.b[i] = sector_bounds[i];
    if (fw_call)
      hipLaunchKernelGGL(k_fresh_sector_feedback, grid, block, lds, st, d, actions, o, r, dn, n_steps, first_slot, n_slots, seq0, g.lead, g.lag, g.magic,
                         obs_stride, rs, ds, gains, act_rec, sector_gains, sb, fw_call);
    else
      hipLaunchKernelGGL(k_step_sector_feedback, grid, block, lds, st, d, actions, o, r, dn, n_steps, first_slot, n_slots, seq0, g.lead, g.lag, g.magic,
                         obs_stride, rs, ds, gains, act_rec, sector_gains, sb);
  } else if (fw_call) {
    hipLaunchKernelGGL(k_fresh_feedback, grid, block, lds, st, d, actions, o, r, dn, n_steps, first_slot, n_slots, seq0, g.lead, g.lag, g.magic, obs_stride,
                       rs, ds, gains, act_rec, fw_call);
  } else {
    hipLaunchKernelGGL(k_step_feedback, grid, block, lds, st, d, actions, o, r, dn, n_steps, first_slot, n_slots, seq0, g.lead, g.lag, g.magic, obs_stride,
                       rs, ds, gains, act_rec);
  }
  if (!obs_rec && !reward_rec && !done_rec) return;
  const size_t last = (size_t)(n_steps - 1), items = (size_t)d.ne * (size_t)(obs_rec ? D : 1);
  hipLaunchKernelGGL(k_feedback_last, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, obs_rec ? obs_rec + last * obs_stride : nullptr,
                     reward_rec ? reward_rec + last * n : nullptr, done_rec ? done_rec + last * n : nullptr, obs, reward, done, d.e0, d.ne, D,
                     d.abort_flag);
}

// The stage's capacity for a bank (S, k_max, m_max known): the largest that gives the one-launch step its best occupancy (see
// k2_lidar.hip) and still leaves room for the search role's chunk list; asked of the runtime, not computed (allocation granule).
int auv_pick_seg_cap(const AuvDev& d0) {
  AuvDev d = d0;
  int best = K2_SEG_CAP, best_occ = -1;
  for (int cap = K2_SEG_CAP; cap >= K2_SEG_CAP_MIN; cap -= 2) {
    d.seg_cap = cap;
    const size_t b = k2_slice_bytes(d);
    if (b < NAV_SCRATCH_BYTES(d.nch_max)) break;
    int occ = 0;
    if (b > 64 * 1024 || hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_step_roles, AUV_WAVE, b) != hipSuccess) occ = 0;
    if (occ > best_occ) best_occ = occ, best = cap;
  }
  return best;
}

uint32_t auv_step_lds_bytes(const AuvDev& d) { return (uint32_t)k2_slice_bytes(d); }

hipError_t auv_step_fused_prepare(const AuvDev& d) {
  const size_t b = k2_slice_bytes(d);
  if (b <= 64 * 1024) return hipSuccess;
  hipError_t e = hipFuncSetAttribute((const void*)k23_lidar_nav, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute((const void*)k_step_multi, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute((const void*)k_step_record, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute((const void*)k_fresh_multi, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute((const void*)k_fresh_record, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute((const void*)k_step_feedback, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute((const void*)k_step_sector_feedback, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute((const void*)k_step_hidden_feedback, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute((const void*)k_fresh_feedback, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute((const void*)k_fresh_sector_feedback, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute((const void*)k_fresh_hidden_feedback, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
  if (e != hipSuccess) return e;
  return hipFuncSetAttribute((const void*)k_step_roles, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
}
