// auv_capi_step.hip — the C ABI's step entries (include/auv_hip.h): reset, every step shape (whole batch, slice, pipelined, several
// steps per launch with their record and feedback forms, async / wait with the rendezvous), both graph forms, the timed steps, the
// stand-alone kernels of a step, and the recovery from a hand-over time-out.  enqueue_step sits here, beside every auv_step* entry
// that calls it.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "auv_host.h"
#include "auv_multi_geom.h"

using namespace auv_host;

namespace auv_host {

int recover_from_timeout(auv_handle* h, float* obs_now) {
  AuvDev& d = h->d;
  const int code = *(volatile int32_t*)h->pair_error_host;
  const int fe0 = ((volatile int32_t*)h->pair_error_host)[1], fne = ((volatile int32_t*)h->pair_error_host)[2];
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  drop_graphs(h);
  const size_t n = (size_t)d.n;
  h->async_pending = 0;
  if (h->rdv) HIP_TRY(hipMemset(h->rdv, 0, AUV_RDV_BYTES));
  h->rdv_seq = h->rdv_target = 0;
  const bool rendezvous = code == 4 || code == 5;
  if (rendezvous) {
    // a rendezvous kernel of auv_step_async / auv_step_wait gave up: the in-launch hand-overs have nothing to do with it and
    // stay in use; the device-word rendezvous does not -- events from now on (they cannot run out)
    h->rdv_timeouts += 1;
    h->rdv_device_ok = false;
  } else {
    h->handover_timeouts += 1;
    h->handover_ok = false;
  }
  // Which environments were left half-stepped?  Exactly those are reset; every other environment is consistent: it completed
  // the steps of the launches that ran, and launches queued behind the time-out did nothing (ABORT packets, k_step_roles --
  // also behind a chain's gate that ran out: its step was NOT taken on actions that may not have been there).  The marks of
  // the aborted launches are still up: cleared here whatever the code was (the rendezvous branch used to return
  // with abort_flag up, and every later one-launch step then did nothing, silently).
  std::vector<uint8_t> broken(n ? n : 1, 0);
  HIP_TRY(hipMemcpy(broken.data(), d.broken, n, hipMemcpyDeviceToHost));
  int n_broken = 0;
  for (size_t e = 0; e < n; e++) n_broken += broken[e] != 0;
  std::vector<unsigned long long> empty(n ? n : 1, AUV_PAIR_EMPTY);
  HIP_TRY(hipMemcpy(d.pair_word, empty.data(), n * sizeof(unsigned long long), hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d.k1_pkt, 0, 8 * n * sizeof(unsigned long long)));
  HIP_TRY(hipMemset(d.nav_hand, 0, 8 * n * sizeof(unsigned long long)));
  HIP_TRY(hipMemset(d.carry, 0, 24 * n * sizeof(unsigned long long)));
  HIP_TRY(hipMemset(d.k1_done, 0, AUV_MAX_CHAINS * sizeof(int32_t)));
  if (n_broken) auv_launch_reset(d, d.broken, nullptr, obs_now, nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemset(d.broken, 0, n));
  HIP_TRY(hipMemset(d.abort_flag, 0, 4 * sizeof(int32_t)));
  memset(h->pair_error_host, 0, 4 * sizeof(int32_t));
  h->last_reset_envs = n_broken;
  if (rendezvous)
    return fail(AUV_ESTATE, "step_async / step_wait rendezvous timed out (%s).  %s  %d environment(s) were reset; the handle orders its chains "
                            "by HIP events from now on (AUV_RDV_EVENTS); this error is reported once",
                code == 4 ? "a chain waited in vain for the caller's stream to publish the actions" : "the caller's stream waited in vain for the chains to arrive",
                code == 4 ? "The step of that chain, and every launch queued behind it, was NOT executed (no environment stepped on actions that were not "
                            "there); chains whose gates had opened did step, so the slices may be one step apart."
                          : "The chains' steps were executed; work enqueued behind step_wait may have read results that were not ready.",
                n_broken);
  h->last_timeout_e0 = fe0, h->last_timeout_ne = fne;
  return fail(AUV_ESTATE, "in-launch hand-over timed out (%s) in the launch over environments [%d, %d): the %d environment(s) whose step "
                          "was left unfinished are back in their reset state (reset observation in OBS64%s); all "
                          "others keep their state, but steps enqueued behind the time-out were not executed.  The handle steps in "
                          "the three-launch shape from now on (no in-launch hand-over); this error is reported once",
              code == 2 ? "a sweep or search wave waited in vain for the dynamics role's state"
                        : code == 6 ? "a wave of a launch of several steps waited in vain for the previous step's finish wave"
                        : (code == 3 ? "a finish wave waited in vain for a state packet or a search record" : "a finish wave waited in vain for a sweep's word"),
              fe0, fe0 + fne, n_broken, obs_now ? " and in this call's observation buffer" : "");
}

// One step of the environments [e0, e0 + ne) on `st`, in the shape effective_mode() names.  Works the same eagerly
// and under stream capture.
// `skip_k1`: the dynamics of this step were done by the previous step's fused kernel; `fuse_next`: this step's
// reward phase also runs the dynamics of the NEXT step (both only inside a captured graph of several steps)
// `chain`: inside a captured chain (auv_graph_capture_chains) the launch uses the ring position / count-off word of its chain
int enqueue_step(auv_handle_t* h, int mode, int e0, int ne, const void* actions, int32_t dtype, float* obs, float* reward,
                 uint8_t* done, hipStream_t st, bool capturing, bool skip_k1, bool fuse_next, int chain) {
  // The action ring belongs to captured graphs only: an eager step reads `actions` as ONE plain
  // [N][2] buffer and neither reads nor advances the ring position (a caller that launches
  // eagerly can pass a different pointer every step).
  AuvDev d = h->d;
  if (!capturing) d.ring_slots = 1;
  d.e0 = e0, d.ne = ne;
  d.ring_pos += chain, d.k1_done += chain;
  if (mode == AUV_STEP_ONE_LAUNCH) {
    // dynamics, LiDAR sweep, navigation search and finish as four roles of ONE launch (csrc/k_step_fused.hip: k_step_roles;
    // inside a captured graph its dynamics role advances the action ring)
    auv_launch_step_roles(d, actions, dtype, obs, reward, done, st);
    return AUV_OK;
  }
  // K1 -> [K2 and K3-nav side by side in one launch] -> K3-reward: no hand-over inside a launch
  if (!auv_k23_ok(d)) return fail(AUV_EINVAL, "path too long for the navigation's chunk list (%d chunks)", d.nch_max);
  if (!skip_k1) auv_launch_k1(d, actions, dtype, st);
  auv_launch_k23(d, obs, st);                         // (advances a captured graph's action ring)
  AuvDev dr = d;
  if (d.ring_slots > 1) dr.ring_slot_host = -2;       // ... so the reward phase does not
  if (fuse_next) auv_launch_k31(dr, actions, dtype, obs, reward, done, st);
  else auv_launch_k3_reward(dr, obs, reward, done, d.cfg.use_lidar ? 0 : 1, st);
  return AUV_OK;
}

int check_slices(const auv_handle_t* h, int32_t n_slices, const int32_t* bounds, const void* streams, const char* who) {
  if (n_slices < 1 || n_slices > AUV_MAX_CHAINS || !bounds || !streams) return fail(AUV_EINVAL, "%s: bad arguments (1 .. %d slices)", who, AUV_MAX_CHAINS);
  if (bounds[0] != 0 || bounds[n_slices] != h->d.n) return fail(AUV_EINVAL, "%s: bounds must run from 0 to %d", who, h->d.n);
  for (int i = 0; i < n_slices; i++)
    if (bounds[i + 1] <= bounds[i]) return fail(AUV_EINVAL, "%s: empty or reversed slice %d", who, i);
  return AUV_OK;
}

int check_actions(const void* actions_dev, int32_t action_dtype, const char* who) {
  if (!actions_dev) return fail(AUV_EINVAL, "%s: null actions", who);
  if (action_dtype != AUV_F32 && action_dtype != AUV_F64) return fail(AUV_EINVAL, "%s: bad action dtype", who);
  // the kernels fetch an environment's (thrust, rudder) pair with one load
  if ((uintptr_t)actions_dev & (action_dtype == AUV_F64 ? 15 : 7))
    return fail(AUV_EINVAL, "%s: the action buffer must be %d-byte aligned", who, action_dtype == AUV_F64 ? 16 : 8);
  return AUV_OK;
}

}  // namespace auv_host

// Do the kernels of the device-word rendezvous get to run side by side on these streams RIGHT NOW?  The pattern of one
// step_async / step_wait with nothing at stake: publish on the caller's stream, on every chain stream a gate, 20 us of a
// do-nothing wave (standing for the step) and the count-off, one wait on the caller's stream -- every wait limited to 50 ms,
// reporting code 6 (no abort, no recovery).  Where dispatches are serialised (a counter-collecting profiler executes one kernel
// at a time, in an order of its own) a waiting kernel sits in front of what it waits for: the trial then costs 50-100 ms ONCE
// and the handle orders its chains by events from then on -- round 4 lost two profiling runs to 300 s of silence instead.
// Synchronises the streams involved (once per set of streams).
static int rdv_trial(auv_handle* h, hipStream_t cs) {
  const size_t nr = h->async_streams.size();
  h->rdv_seq += 1;
  auv_launch_rdv_publish(h->rdv, h->rdv_seq, cs);
  for (size_t j = 0; j < nr; j++) {
    hipStream_t st = h->async_streams[j];
    auv_launch_rdv_wait(h->rdv, h->rdv_seq, h->d.pair_error, 6, 0.05, nullptr, h->d.abort_flag + 2, st);
    auv_launch_spin(2000, st);
    auv_launch_rdv_arrive(h->rdv + 16, st);
  }
  h->rdv_target += nr;
  auv_launch_rdv_wait(h->rdv + 16, h->rdv_target, h->d.pair_error, 6, 0.05, nullptr, h->d.abort_flag + 2, cs);
  HIP_TRY(hipGetLastError());
  for (size_t j = 0; j < nr; j++) HIP_TRY(hipStreamSynchronize(h->async_streams[j]));
  HIP_TRY(hipStreamSynchronize(cs));
  h->rdv_tried = h->async_streams;
  {
    // (a hand-over time-out of a step still in flight on some chain may have crossed the trial's report on the one host word:
    // the device-side flag is the truth)
    int32_t up = 0;
    HIP_TRY(hipMemcpy(&up, h->d.abort_flag, sizeof(up), hipMemcpyDeviceToHost));
    const int32_t seen = *(volatile int32_t*)h->pair_error_host;
    if (up && (seen == 0 || seen == 6)) {
      h->rdv_device_ok = false;
      *(volatile int32_t*)h->pair_error_host = 1;
      return AUV_OK;                                   // the next call's PAIR_CHECK recovers
    }
  }
  if (*(volatile int32_t*)h->pair_error_host == 6) {
    *(volatile int32_t*)h->pair_error_host = 0;
    HIP_TRY(hipMemset(h->d.abort_flag + 2, 0, sizeof(int32_t)));
    HIP_TRY(hipMemset(h->rdv, 0, AUV_RDV_BYTES));
    h->rdv_seq = h->rdv_target = 0;
    h->rdv_device_ok = false;
    h->rdv_timeouts += 1;
  }
  return AUV_OK;
}

extern "C" {

int auv_reset(auv_handle_t* h, const uint8_t* mask_dev, const int32_t* world_idx_dev, float* obs_dev, void* stream) {
  REQUIRE_READY(h);
  hipStream_t st = (hipStream_t)stream;
  if (h->fw.on && world_idx_dev)
    return fail(AUV_EINVAL, "auv_reset: with a fresh world per reset the library chooses the world (an environment's next unseen slot)");
  auv_launch_reset(h->d, mask_dev, world_idx_dev, obs_dev, st);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

int auv_step(auv_handle_t* h, const void* actions_dev, int32_t action_dtype, float* obs_dev, float* reward_dev,
             uint8_t* done_dev, void* stream) {
  REQUIRE_READY(h);
  int rc = check_actions(actions_dev, action_dtype, "auv_step");
  if (rc) return rc;
  PAIR_CHECK_ON(h, stream, true, obs_dev);
  if (h->fw.on) {
    const int32_t whole[2] = {0, h->d.n};
    rc = fw_tick(h, 1, whole, &stream);
    if (rc) return rc;
  }
  rc = enqueue_step(h, effective_mode(h, h->d.n), 0, h->d.n, actions_dev, action_dtype, obs_dev, reward_dev, done_dev,
                    (hipStream_t)stream, false);
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

int auv_step_slice(auv_handle_t* h, int32_t e0, int32_t ne, const void* actions_dev, int32_t action_dtype, float* obs_dev,
                   float* reward_dev, uint8_t* done_dev, void* stream) {
  REQUIRE_READY(h);
  int rc = check_actions(actions_dev, action_dtype, "auv_step_slice");
  if (rc) return rc;
  if (e0 < 0 || ne < 1 || (int64_t)e0 + ne > h->d.n) return fail(AUV_EINVAL, "auv_step_slice: slice [%d, %d) outside [0, %d)", e0, e0 + ne, h->d.n);
  PAIR_CHECK_ON(h, stream, true, obs_dev);
  rc = enqueue_step(h, effective_mode(h, ne), e0, ne, actions_dev, action_dtype, obs_dev, reward_dev, done_dev, (hipStream_t)stream, false);
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

int auv_step_pipelined(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const void* actions_dev,
                       int32_t action_dtype, float* obs_dev, float* reward_dev, uint8_t* done_dev) {
  REQUIRE_READY(h);
  int rc = check_actions(actions_dev, action_dtype, "auv_step_pipelined");
  if (rc) return rc;
  rc = check_slices(h, n_slices, bounds, streams, "auv_step_pipelined");
  if (rc) return rc;
  PAIR_CHECK(h, obs_dev);
  rc = fw_tick(h, n_slices, bounds, streams);
  for (int i = 0; i < n_slices && rc == AUV_OK; i++)
    rc = enqueue_step(h, effective_mode(h, bounds[i + 1] - bounds[i]), bounds[i], bounds[i + 1] - bounds[i], actions_dev, action_dtype,
                      obs_dev, reward_dev, done_dev, (hipStream_t)streams[i], false);
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

// A multi-step call in fresh-world mode (auv_fresh_worlds_multi): its number, handed to every chain's launch; fw_multi_begin puts the
// one-wave kernel that announces the call directly in front of a chain's launch (auv_device.h: auv_next_world_multi has the argument).
static unsigned int fw_multi_call(auv_handle* h) { return h->fw.on ? ++h->fw.multi_call : 0u; }
static void fw_multi_begin(auv_handle* h, unsigned int call, hipStream_t st) {
  if (call) auv_launch_fw_call(h->d.fw_ctl, call, st);
}

// what auv_step_multi, auv_step_multi_record and auv_step_feedback refuse, before anything launches and before any step number is spent
// `ring_optional`: a NULL ring is allowed (auv_step_feedback: x_7 = 0); `state_rc`: the code of the refusals that hang on the handle's
// configuration (auv_step_feedback reports every refusal as AUV_EINVAL)
static int check_multi(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const void* actions_dev, int32_t action_dtype,
                       int32_t n_slots, int32_t first_slot, int32_t n_steps, const char* who, bool ring_optional = false, int state_rc = AUV_ESTATE,
                       bool fresh_kernels = false) {
  int rc = (ring_optional && !actions_dev) ? AUV_OK : check_actions(actions_dev, action_dtype, who);
  if (rc) return rc;
  rc = check_slices(h, n_slices, bounds, streams, who);
  if (rc) return rc;
  if (n_slots < 1 || first_slot < 0 || first_slot >= n_slots || n_steps < 1 || n_steps > 1024)
    return fail(AUV_EINVAL, "%s: n_slots >= 1, 0 <= first_slot < n_slots, 1 <= n_steps <= 1024", who);
  // (`fresh_kernels`: the entry has kernels that bind only slots published before the call began -- used once the handle has opted in)
  if (h->fw.on && !(fresh_kernels && h->fw.multi))
    return fail(state_rc, "%s: not with a fresh world per reset (a slot's tables may be rebuilt beside the launch)", who);
  if (h->fw.on)
    for (int s = 0; s < n_slices; s++)
      if (stream_capturing((hipStream_t)streams[s]))
        return fail(state_rc, "%s: with a fresh world per reset not on a stream that is being captured (the call's number is a launch argument)", who);
  if (h->d.k_max > AUV_WAVE) return fail(state_rc, "%s: more than 64 obstacles per world", who);
  for (int i = 0; i < n_slices; i++) {
    const int ne = bounds[i + 1] - bounds[i];
    if (effective_mode(h, ne) != AUV_STEP_ONE_LAUNCH) return fail(state_rc, "%s: needs the one-launch shape for every slice", who);
    // the grid that will be launched, in work-items: the dispatch packet holds a 32-bit count
    const AuvMultiGeom g = auv_multi_geom(ne, n_steps, h->multi_order, h->multi_lead, h->multi_lag);
    if (!auv_multi_fits(g))
      return fail(AUV_EINVAL, "%s: %llu work-items in one launch of %d environments x %d steps (at most 2^32 - 1)", who,
                  auv_multi_grid(g) * AUV_MULTI_WG_LANES, ne, (int)n_steps);
  }
  return AUV_OK;
}

int auv_step_multi(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const void* actions_dev, int32_t action_dtype,
                   int32_t n_slots, int32_t first_slot, int32_t n_steps, float* obs_dev, float* reward_dev, uint8_t* done_dev) {
  REQUIRE_READY(h);
  const int rc = check_multi(h, n_slices, bounds, streams, actions_dev, action_dtype, n_slots, first_slot, n_steps, "auv_step_multi", false, AUV_ESTATE, true);
  if (rc) return rc;
  PAIR_CHECK(h, obs_dev);
  const unsigned long long seq0 = h->multi_seq;
  h->multi_seq += (unsigned long long)n_steps;
  const unsigned int call = fw_multi_call(h);
  for (int i = 0; i < n_slices; i++) {
    AuvDev d = h->d;
    d.e0 = bounds[i], d.ne = bounds[i + 1] - bounds[i];
    fw_multi_begin(h, call, (hipStream_t)streams[i]);
    auv_launch_step_multi(d, actions_dev, action_dtype, obs_dev, reward_dev, done_dev, n_steps, first_slot, n_slots, seq0, h->multi_order, h->multi_lead,
                          h->multi_lag, (hipStream_t)streams[i], call);
  }
  HIP_TRY(hipGetLastError());
  return fw_tick(h, n_slices, bounds, streams, n_steps, true);   // (behind the launches: the pass finds what this call has left)
}

int auv_step_multi_record(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const void* actions_dev,
                          int32_t action_dtype, int32_t n_slots, int32_t first_slot, int32_t n_steps, float* obs_dev, float* reward_dev,
                          uint8_t* done_dev, float* obs_rec, float* reward_rec, uint8_t* done_rec) {
  REQUIRE_READY(h);
  const int rc = check_multi(h, n_slices, bounds, streams, actions_dev, action_dtype, n_slots, first_slot, n_steps, "auv_step_multi_record", false, AUV_ESTATE, true);
  if (rc) return rc;
  if (!reward_rec || !done_rec) return fail(AUV_EINVAL, "auv_step_multi_record: reward_rec and done_rec are required (only obs_rec may be NULL)");
  if (!obs_dev || !reward_dev || !done_dev) return fail(AUV_EINVAL, "auv_step_multi_record: null obs / reward / done buffer");
  // the tail stores an observation row's six navigation features as three float pairs when the row width is even (k3_nav_reward.hip,
  // nav_tail): every row of the record then starts an even number of floats behind obs_rec
  const int D = auv_obs_cols(h->d.cfg, h->d.pool_ns);
  if (obs_rec && ((uintptr_t)obs_rec & ((D & 1) ? 3 : 7)))
    return fail(AUV_EINVAL, "auv_step_multi_record: obs_rec must be %d-byte aligned (observation rows of %d floats)", (D & 1) ? 4 : 8, D);
  if ((uintptr_t)reward_rec & 3) return fail(AUV_EINVAL, "auv_step_multi_record: reward_rec must be 4-byte aligned");
  PAIR_CHECK(h, obs_dev);
  const unsigned long long seq0 = h->multi_seq;
  h->multi_seq += (unsigned long long)n_steps;
  const unsigned int call = fw_multi_call(h);
  for (int i = 0; i < n_slices; i++) {
    AuvDev d = h->d;
    d.e0 = bounds[i], d.ne = bounds[i + 1] - bounds[i];
    fw_multi_begin(h, call, (hipStream_t)streams[i]);
    auv_launch_step_record(d, actions_dev, action_dtype, obs_dev, reward_dev, done_dev, obs_rec, reward_rec, done_rec, n_steps, first_slot, n_slots, seq0,
                           h->multi_order, h->multi_lead, h->multi_lag, (hipStream_t)streams[i], call);
  }
  HIP_TRY(hipGetLastError());
  return fw_tick(h, n_slices, bounds, streams, n_steps, true);   // (as auv_step_multi)
}

// auv_step_feedback (`sectors` false) and auv_step_feedback_sectors: the same checks and the same launch, the second with the sector
// gains and the bounds table (padded here to 17 entries with its last one: the sectors past n_sectors are empty ranges)
// auv_step_feedback_hidden (`hidden`, with `sectors`): the sector entry's checks plus the hidden block's and the activation's
static int step_feedback_any(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const double* gains_dev, const void* actions_dev,
                             int32_t action_dtype, int32_t n_slots, int32_t first_slot, int32_t n_steps, float* obs_dev, float* reward_dev,
                             uint8_t* done_dev, float* obs_rec, float* reward_rec, uint8_t* done_rec, double* act_rec, const char* who, bool sectors,
                             const double* sector_gains_dev, const int32_t* sector_bounds_host, int32_t n_sectors, bool hidden = false,
                             const double* hidden_dev = nullptr, int32_t activation = 0) {
  REQUIRE_READY(h);
  if (!gains_dev || ((uintptr_t)gains_dev & 7)) return fail(AUV_EINVAL, "%s: gains_dev must be a non-NULL, 8-byte aligned [N][2][8] fp64 table", who);
  int32_t sb[17];
  if (sectors) {
    if (!sector_gains_dev || ((uintptr_t)sector_gains_dev & 7))
      return fail(AUV_EINVAL, "%s: sector_gains_dev must be a non-NULL, 8-byte aligned [N][2][16] fp64 table", who);
    if (!sector_bounds_host) return fail(AUV_EINVAL, "%s: null sector_bounds_host", who);
    if (!h->d.cfg.use_lidar) return fail(AUV_EINVAL, "%s: sector inputs need the LiDAR (use_lidar is off)", who);
    if (n_sectors < 1 || n_sectors > 16) return fail(AUV_EINVAL, "%s: n_sectors must be 1 .. 16, got %d", who, n_sectors);
    const int L = h->d.pool_ns ? h->d.pool_ns : h->d.cfg.n_sensors;                    // the row's closeness columns
    for (int k = 0; k <= n_sectors; k++)
      if (sector_bounds_host[k] < (k ? sector_bounds_host[k - 1] : 0) || sector_bounds_host[k] > L)
        return fail(AUV_EINVAL, "%s: sector bounds must be ascending within [0, %d] (entry %d is %d)", who, L, k, sector_bounds_host[k]);
    for (int k = 0; k < 17; k++) sb[k] = sector_bounds_host[k < n_sectors ? k : n_sectors];
  }
  if (hidden) {
    if (!hidden_dev || ((uintptr_t)hidden_dev & 15))
      return fail(AUV_EINVAL, "%s: hidden_dev must be a non-NULL, 16-byte aligned [N][16][28] fp64 block", who);
    if (activation != 0 && activation != 1) return fail(AUV_EINVAL, "%s: activation must be 0 (relu) or 1 (hard tanh), got %d", who, activation);
  }
  if (actions_dev && n_slots < 1) return fail(AUV_EINVAL, "%s: n_slots >= 1 with a ring", who);
  if (!actions_dev) n_slots = 1, first_slot = 0, action_dtype = AUV_F32;               // no ring: x_7 = 0, nothing is read
  // (a fresh world per reset: only where the handle has opted in for the closed loop too -- auv_fresh_worlds_multi(h, 2))
  const int rc = check_multi(h, n_slices, bounds, streams, actions_dev, action_dtype, n_slots, first_slot, n_steps, who, true, AUV_EINVAL, h->fw.feedback);
  if (rc) return rc;
  if (!obs_dev || !reward_dev || !done_dev) return fail(AUV_EINVAL, "%s: null obs / reward / done buffer", who);
  const int D = auv_obs_cols(h->d.cfg, h->d.pool_ns);                                    // (see auv_step_multi_record)
  if (obs_rec && ((uintptr_t)obs_rec & ((D & 1) ? 3 : 7)))
    return fail(AUV_EINVAL, "%s: obs_rec must be %d-byte aligned (observation rows of %d floats)", who, (D & 1) ? 4 : 8, D);
  if ((uintptr_t)reward_rec & 3) return fail(AUV_EINVAL, "%s: reward_rec must be 4-byte aligned", who);
  if ((uintptr_t)act_rec & 7) return fail(AUV_EINVAL, "%s: act_rec must be 8-byte aligned", who);
  PAIR_CHECK(h, obs_dev);
  const unsigned long long seq0 = h->multi_seq;
  h->multi_seq += (unsigned long long)n_steps;
  const unsigned int call = fw_multi_call(h);
  for (int i = 0; i < n_slices; i++) {
    AuvDev d = h->d;
    d.e0 = bounds[i], d.ne = bounds[i + 1] - bounds[i];
    fw_multi_begin(h, call, (hipStream_t)streams[i]);
    auv_launch_step_feedback(d, gains_dev, actions_dev, action_dtype, obs_dev, reward_dev, done_dev, obs_rec, reward_rec, done_rec, act_rec, n_steps,
                             first_slot, n_slots, seq0, h->multi_order, h->multi_lead, h->multi_lag, (hipStream_t)streams[i],
                             sectors ? sector_gains_dev : nullptr, sectors ? sb : nullptr, hidden ? hidden_dev : nullptr, activation, call);
  }
  HIP_TRY(hipGetLastError());
  return fw_tick(h, n_slices, bounds, streams, n_steps, true);   // (as auv_step_multi)
}

int auv_step_feedback(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const double* gains_dev, const void* actions_dev,
                      int32_t action_dtype, int32_t n_slots, int32_t first_slot, int32_t n_steps, float* obs_dev, float* reward_dev, uint8_t* done_dev,
                      float* obs_rec, float* reward_rec, uint8_t* done_rec, double* act_rec) {
  return step_feedback_any(h, n_slices, bounds, streams, gains_dev, actions_dev, action_dtype, n_slots, first_slot, n_steps, obs_dev, reward_dev, done_dev,
                           obs_rec, reward_rec, done_rec, act_rec, "auv_step_feedback", false, nullptr, nullptr, 0);
}

int auv_step_feedback_sectors(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const double* gains_dev,
                              const void* actions_dev, int32_t action_dtype, int32_t n_slots, int32_t first_slot, int32_t n_steps, float* obs_dev,
                              float* reward_dev, uint8_t* done_dev, float* obs_rec, float* reward_rec, uint8_t* done_rec, double* act_rec,
                              const double* sector_gains_dev, const int32_t* sector_bounds_host, int32_t n_sectors) {
  return step_feedback_any(h, n_slices, bounds, streams, gains_dev, actions_dev, action_dtype, n_slots, first_slot, n_steps, obs_dev, reward_dev, done_dev,
                           obs_rec, reward_rec, done_rec, act_rec, "auv_step_feedback_sectors", true, sector_gains_dev, sector_bounds_host, n_sectors);
}

int auv_step_feedback_hidden(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const double* gains_dev,
                             const void* actions_dev, int32_t action_dtype, int32_t n_slots, int32_t first_slot, int32_t n_steps, float* obs_dev,
                             float* reward_dev, uint8_t* done_dev, float* obs_rec, float* reward_rec, uint8_t* done_rec, double* act_rec,
                             const double* sector_gains_dev, const int32_t* sector_bounds_host, int32_t n_sectors, const double* hidden_dev,
                             int32_t activation) {
  return step_feedback_any(h, n_slices, bounds, streams, gains_dev, actions_dev, action_dtype, n_slots, first_slot, n_steps, obs_dev, reward_dev, done_dev,
                           obs_rec, reward_rec, done_rec, act_rec, "auv_step_feedback_hidden", true, sector_gains_dev, sector_bounds_host, n_sectors, true,
                           hidden_dev, activation);
}

int auv_set_multi_order(auv_handle_t* h, int32_t order, int32_t lead, int32_t lag) {
  if (!h || order < 0 || order > 1 || lead < 0 || lag < 0 || lead > 4096 || lag > 4096) return fail(AUV_EINVAL, "auv_set_multi_order: order 0 / 1, lead and lag in [0, 4096]");
  h->multi_order = order, h->multi_lead = lead, h->multi_lag = lag;
  return AUV_OK;
}

int auv_lidar_stage(auv_handle_t* h, int32_t segments, int32_t* out_segments) {
  REQUIRE_READY(h);
  if (segments != 0) {
    if (segments < 32 || segments > 96 || (segments & 1)) return fail(AUV_EINVAL, "auv_lidar_stage: segments must be 0 (report) or even, 32 .. 96");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());                      // (launches in flight carry the old stage by value: let them end first)
    AuvDev d = h->d;
    d.seg_cap = segments;
    if (!auv_k23_ok(d)) return fail(AUV_EINVAL, "auv_lidar_stage: a %d-segment slice cannot hold the navigation's chunk list", segments);
    HIP_TRY(auv_k2_prepare(d));
    HIP_TRY(auv_step_fused_prepare(d));
    h->d.seg_cap = segments;
    if (h->fw.on) h->fw.shadow.seg_cap = segments;         // (the refill pass's captured graph keeps the stage it was captured with)
  }
  if (out_segments) *out_segments = h->d.seg_cap;
  return AUV_OK;
}

int auv_step_async(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const void* actions_dev,
                   int32_t action_dtype, float* obs_dev, float* reward_dev, uint8_t* done_dev, void* caller_stream, int32_t rendezvous) {
  REQUIRE_READY(h);
  int rc = check_actions(actions_dev, action_dtype, "auv_step_async");
  if (rc) return rc;
  rc = check_slices(h, n_slices, bounds, streams, "auv_step_async");
  if (rc) return rc;
  if (rendezvous != AUV_RDV_EVENTS && rendezvous != AUV_RDV_DEVICE && rendezvous != AUV_RDV_CP)
    return fail(AUV_EINVAL, "auv_step_async: rendezvous must be one of AUV_RDV_*");
  if (h->async_pending) return fail(AUV_ESTATE, "auv_step_async: the previous step has not been waited for (auv_step_wait)");
  PAIR_CHECK(h, obs_dev);
  HIP_TRY(hipSetDevice(h->device));
  rc = fw_tick(h, n_slices, bounds, streams);
  if (rc) return rc;
  hipStream_t cs = (hipStream_t)caller_stream;
  h->async_streams.clear();
  for (int i = 0; i < n_slices; i++)
    if ((hipStream_t)streams[i] != cs) h->async_streams.push_back((hipStream_t)streams[i]);
  const size_t nr = h->async_streams.size();         // chains on streams of their own: the others are in stream order already
  if (nr && rendezvous != AUV_RDV_EVENTS && !h->rdv) return fail(AUV_ESTATE, "auv_step_async: rendezvous words missing (no bank loaded?)");
  if (nr && rendezvous == AUV_RDV_DEVICE) {
    // The device-word rendezvous needs (i) the one-launch shape for every slice -- a gate that runs out stops its step by
    // ABORT packets, which only that shape reads -- and (ii) streams that run side by side NOW.  (ii) is tried before the
    // first real step on a set of streams (rdv_trial: 50 ms, no step at stake); a trial or a real wait that has run out
    // demotes the handle to events for good.
    bool one_launch = true;
    for (int i = 0; i < n_slices; i++) one_launch = one_launch && effective_mode(h, bounds[i + 1] - bounds[i]) == AUV_STEP_ONE_LAUNCH;
    if (!one_launch || !h->rdv_device_ok) rendezvous = AUV_RDV_EVENTS;
    else if (h->rdv_tried != h->async_streams && !stream_capturing(cs)) {
      int rc_t = rdv_trial(h, cs);
      if (rc_t) return rc_t;
      if (!h->rdv_device_ok) rendezvous = AUV_RDV_EVENTS;
    }
  }
  if (nr && rendezvous == AUV_RDV_EVENTS) {
    if (!h->ev_actions) HIP_TRY(hipEventCreateWithFlags(&h->ev_actions, hipEventDisableTiming));
    while (h->ev_chain.size() < nr) {
      hipEvent_t e;
      HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      h->ev_chain.push_back(e);
    }
    HIP_TRY(hipEventRecord(h->ev_actions, cs));                                    // behind whatever produced the actions
  } else if (nr) {
    h->rdv_seq += 1;
    if (rendezvous == AUV_RDV_DEVICE) auv_launch_rdv_publish(h->rdv, h->rdv_seq, cs);
    else HIP_TRY(hipStreamWriteValue64(cs, h->rdv, h->rdv_seq, 0));
  }
  size_t j = 0;
  for (int i = 0; i < n_slices && rc == AUV_OK; i++) {
    hipStream_t st = (hipStream_t)streams[i];
    const bool remote = st != cs;
    if (remote) {
      if (rendezvous == AUV_RDV_EVENTS) HIP_TRY(hipStreamWaitEvent(st, h->ev_actions, 0));
      else if (rendezvous == AUV_RDV_DEVICE) auv_launch_rdv_wait(h->rdv, h->rdv_seq, h->d.pair_error, 4, h->rdv_limit_s, h->d.abort_flag, h->d.abort_flag + 1, st);
      else HIP_TRY(hipStreamWaitValue64(st, h->rdv, h->rdv_seq, hipStreamWaitValueGte, ~0ull));
    }
    rc = enqueue_step(h, effective_mode(h, bounds[i + 1] - bounds[i]), bounds[i], bounds[i + 1] - bounds[i], actions_dev, action_dtype,
                      obs_dev, reward_dev, done_dev, st, false);
    if (remote && rc == AUV_OK) {
      if (rendezvous == AUV_RDV_EVENTS) HIP_TRY(hipEventRecord(h->ev_chain[j], st));
      else if (rendezvous == AUV_RDV_DEVICE) auv_launch_rdv_arrive(h->rdv + 16, st);
      else HIP_TRY(hipStreamWriteValue64(st, h->rdv + 32 + 16 * j, h->rdv_seq, 0));
      j++;
    }
  }
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  if (rendezvous == AUV_RDV_DEVICE) h->rdv_target += nr;
  h->async_pending = 1 + rendezvous;
  return AUV_OK;
}

int auv_step_wait(auv_handle_t* h, void* caller_stream) {
  REQUIRE_READY(h);
  if (!h->async_pending) return fail(AUV_ESTATE, "auv_step_wait: no step pending (auv_step_async)");
  const int rendezvous = h->async_pending - 1;
  hipStream_t cs = (hipStream_t)caller_stream;
  const size_t nr = h->async_streams.size();
  h->async_pending = 0;
  if (nr) {
    if (rendezvous == AUV_RDV_EVENTS) {
      for (size_t j = 0; j < nr; j++) HIP_TRY(hipStreamWaitEvent(cs, h->ev_chain[j], 0));
    } else if (rendezvous == AUV_RDV_DEVICE) {
      auv_launch_rdv_wait(h->rdv + 16, h->rdv_target, h->d.pair_error, 5, h->rdv_limit_s, nullptr, h->d.abort_flag + 1, cs);   // ONE wait for all chains
      HIP_TRY(hipGetLastError());
    } else {
      for (size_t j = 0; j < nr; j++) HIP_TRY(hipStreamWaitValue64(cs, h->rdv + 32 + 16 * j, h->rdv_seq, hipStreamWaitValueGte, ~0ull));
    }
  }
  return AUV_OK;
}

int auv_set_rendezvous_limit(auv_handle_t* h, double seconds) {
  if (!h || !(seconds > 0.0) || seconds > 3600.0) return fail(AUV_EINVAL, "auv_set_rendezvous_limit: seconds must be in (0, 3600]");
  h->rdv_limit_s = seconds;
  return AUV_OK;
}

int auv_graph_capture_chains(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, const void* actions_dev, int32_t action_dtype,
                             float* obs_dev, float* reward_dev, uint8_t* done_dev, int32_t n_steps, int32_t one_graph) {
  REQUIRE_READY(h);
  int rc = check_actions(actions_dev, action_dtype, "auv_graph_capture_chains");
  if (rc) return rc;
  rc = check_slices(h, n_slices, bounds, bounds, "auv_graph_capture_chains");   // (the chains' streams are named at replay)
  if (rc) return rc;
  if (n_steps < 1 || n_steps > 4096) return fail(AUV_EINVAL, "auv_graph_capture_chains: n_steps must be in [1, 4096]");
  PAIR_CHECK(h, obs_dev);
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  drop_graphs(h);
  if (h->graph) {
    HIP_TRY(hipGraphDestroy(h->graph));
    h->graph = nullptr;
  }
  if (!h->cap_stream) HIP_TRY(hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking));
  // every chain starts at slot 0 of the ring and keeps a position of its own (advanced by its own dynamics waves)
  HIP_TRY(hipMemset(h->d.ring_pos, 0, AUV_MAX_CHAINS * sizeof(int32_t)));
  HIP_TRY(hipMemset(h->d.k1_done, 0, AUV_MAX_CHAINS * sizeof(int32_t)));
  h->chain_bounds.assign(bounds, bounds + n_slices + 1), h->chain_steps = n_steps, h->graph_steps = n_steps;
  if (!one_graph) {
    // K linear graphs, replayed on K streams of the caller's choice (auv_graph_launch_chains): which hardware queue a
    // chain runs on stays the caller's decision, as for eager chains
    for (int i = 0; i < n_slices; i++) {
      const int ne = bounds[i + 1] - bounds[i];
      HIP_TRY(hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal));
      for (int32_t k = 0; k < n_steps && rc == AUV_OK; k++)
        rc = enqueue_step(h, effective_mode(h, ne), bounds[i], ne, actions_dev, action_dtype, obs_dev, reward_dev, done_dev, h->cap_stream,
                          true, false, false, i);
      hipGraph_t g = nullptr;
      hipError_t ce = hipStreamEndCapture(h->cap_stream, &g);
      if (rc) return rc;
      HIP_TRY(ce);
      h->chain_graph.push_back(g);
      hipGraphExec_t ge = nullptr;
      HIP_TRY(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
      h->chain_exec.push_back(ge);
    }
    return AUV_OK;
  }
  // ONE graph whose K branches are the chains (fork behind the root, join at the end): replayed with auv_graph_launch,
  // the runtime picks the streams of the branches
  while ((int)h->fork_streams.size() < n_slices - 1) {
    hipStream_t st;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    h->fork_streams.push_back(st);
  }
  while ((int)h->ev_chain.size() < n_slices) {
    hipEvent_t e;
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    h->ev_chain.push_back(e);
  }
  HIP_TRY(hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal));
  hipError_t fe = hipEventRecord(h->ev_chain[0], h->cap_stream);
  for (int i = 1; i < n_slices && fe == hipSuccess; i++) fe = hipStreamWaitEvent(h->fork_streams[i - 1], h->ev_chain[0], 0);
  for (int i = 0; i < n_slices && rc == AUV_OK && fe == hipSuccess; i++) {
    const int ne = bounds[i + 1] - bounds[i];
    hipStream_t st = i == 0 ? h->cap_stream : h->fork_streams[i - 1];
    for (int32_t k = 0; k < n_steps && rc == AUV_OK; k++)
      rc = enqueue_step(h, effective_mode(h, ne), bounds[i], ne, actions_dev, action_dtype, obs_dev, reward_dev, done_dev, st, true, false,
                        false, i);
  }
  for (int i = 1; i < n_slices && fe == hipSuccess; i++) {
    fe = hipEventRecord(h->ev_chain[i], h->fork_streams[i - 1]);
    if (fe == hipSuccess) fe = hipStreamWaitEvent(h->cap_stream, h->ev_chain[i], 0);
  }
  hipError_t ce = hipStreamEndCapture(h->cap_stream, &h->graph);
  if (rc) return rc;
  HIP_TRY(fe);
  HIP_TRY(ce);
  HIP_TRY(hipGraphInstantiate(&h->graph_exec, h->graph, nullptr, nullptr, 0));
  return AUV_OK;
}

int auv_graph_launch_chains(auv_handle_t* h, int32_t n_slices, void* const* streams) {
  REQUIRE_READY(h);
  if (!streams || n_slices != (int32_t)h->chain_exec.size() || n_slices < 1)
    return fail(AUV_ESTATE, "auv_graph_launch_chains: %d streams for %d captured chains", n_slices, (int)h->chain_exec.size());
  PAIR_CHECK(h, nullptr);
  {
    int rc_t = fw_tick(h, n_slices, h->chain_bounds.data(), streams, h->chain_steps);
    if (rc_t) return rc_t;
  }
  for (int i = 0; i < n_slices; i++) HIP_TRY(hipGraphLaunch(h->chain_exec[i], (hipStream_t)streams[i]));
  return AUV_OK;
}

int auv_step_pipelined_timed(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const void* actions_dev,
                             int32_t action_dtype, float* obs_dev, float* reward_dev, uint8_t* done_dev, float* out_ms) {
  REQUIRE_READY(h);
  int rc = check_actions(actions_dev, action_dtype, "auv_step_pipelined_timed");
  if (rc) return rc;
  if (n_slices < 1 || !bounds || !streams || !out_ms) return fail(AUV_EINVAL, "auv_step_pipelined_timed: bad arguments");
  if (bounds[0] != 0 || bounds[n_slices] != h->d.n) return fail(AUV_EINVAL, "auv_step_pipelined_timed: bounds must run from 0 to %d", h->d.n);
  PAIR_CHECK(h, obs_dev);
  while ((int)h->slice_ev.size() < 2 * n_slices) {
    hipEvent_t e;
    HIP_TRY(hipEventCreate(&e));
    h->slice_ev.push_back(e);
  }
  for (int i = 0; i < n_slices; i++) {
    const int ne = bounds[i + 1] - bounds[i];
    if (ne < 1) return fail(AUV_EINVAL, "auv_step_pipelined_timed: empty slice %d", i);
    if (effective_mode(h, ne) != AUV_STEP_ONE_LAUNCH) return fail(AUV_ESTATE, "auv_step_pipelined_timed: needs the one-launch shape");
    AuvDev d = h->d;
    d.ring_slots = 1;
    d.e0 = bounds[i], d.ne = ne;
    auv_launch_step_roles(d, actions_dev, action_dtype, obs_dev, reward_dev, done_dev, (hipStream_t)streams[i], h->slice_ev[2 * i],
                          h->slice_ev[2 * i + 1]);
  }
  HIP_TRY(hipGetLastError());
  for (int i = 0; i < n_slices; i++) {
    HIP_TRY(hipEventSynchronize(h->slice_ev[2 * i + 1]));
    HIP_TRY(hipEventElapsedTime(&out_ms[i], h->slice_ev[2 * i], h->slice_ev[2 * i + 1]));
  }
  return AUV_OK;
}

int auv_step_dynamics(auv_handle_t* h, const void* actions_dev, int32_t action_dtype, void* stream) {
  REQUIRE_READY(h);
  {
    int rc_a = check_actions(actions_dev, action_dtype, "auv_step_dynamics");
    if (rc_a) return rc_a;
  }
  auv_launch_k1(h->d, actions_dev, action_dtype, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

int auv_lidar(auv_handle_t* h, int32_t advance_movers, void* stream) {
  REQUIRE_READY(h);
  auv_launch_k2(h->d, advance_movers ? 1 : 0, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

int auv_nav_reward(auv_handle_t* h, int32_t mode, float* obs_dev, float* reward_dev, uint8_t* done_dev, void* stream) {
  REQUIRE_READY(h);
  if (mode < 0 || mode > 2) return fail(AUV_EINVAL, "auv_nav_reward: mode must be 0, 1 or 2");
  auv_launch_k3(h->d, mode, obs_dev, reward_dev, done_dev, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

int auv_graph_capture(auv_handle_t* h, const void* actions_dev, int32_t action_dtype, float* obs_dev,
                      float* reward_dev, uint8_t* done_dev, void* stream) {
  return auv_graph_capture_steps(h, actions_dev, action_dtype, obs_dev, reward_dev, done_dev, 1, stream);
}

int auv_graph_capture_steps(auv_handle_t* h, const void* actions_dev, int32_t action_dtype, float* obs_dev,
                            float* reward_dev, uint8_t* done_dev, int32_t n_steps, void* stream) {
  REQUIRE_READY(h);
  (void)stream;
  if (n_steps < 1 || n_steps > 4096) return fail(AUV_EINVAL, "auv_graph_capture_steps: n_steps must be in [1, 4096]");
  {
    int rc_a = check_actions(actions_dev, action_dtype, "auv_graph_capture");
    if (rc_a) return rc_a;
  }
  PAIR_CHECK(h, obs_dev);
  if (!h->cap_stream) HIP_TRY(hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking));
  drop_graphs(h);
  if (h->graph) {
    HIP_TRY(hipGraphDestroy(h->graph));
    h->graph = nullptr;
  }
  HIP_TRY(hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal));
  int rc = AUV_OK;
  // inside the graph, step k's reward phase and step k+1's dynamics share a launch (side-by-side shape with a LiDAR
  // sweep: the shapes whose reward kernel maps lanes to environments)
  // (also when the handle steps in the one-launch shape: replayed launches cost ~3 us more than eager ones on this
  // stack, and inside a graph of several steps the fused reward + dynamics launch makes up for more of that than the
  // one launch does -- 97.6 M against 96.6 M env-steps/s at 16 steps per graph, 95.3 against 90.6 M at 8192 x 256 --
  // and the bits are the same.  A graph of ONE step keeps the handle's own shape.)
  h->graph_steps = n_steps;
  const bool fuse = n_steps > 1 && auv_k23_ok(h->d) && h->d.cfg.use_lidar;
  const int mode = fuse ? AUV_STEP_SIDE_BY_SIDE : effective_mode(h, h->d.n);
  for (int32_t k = 0; k < n_steps && rc == AUV_OK; k++)
    rc = enqueue_step(h, mode, 0, h->d.n, actions_dev, action_dtype, obs_dev, reward_dev, done_dev, h->cap_stream, true,
                      fuse && k > 0, fuse && k + 1 < n_steps);
  hipError_t ce = hipStreamEndCapture(h->cap_stream, &h->graph);
  if (rc) return rc;
  HIP_TRY(ce);
  HIP_TRY(hipGraphInstantiate(&h->graph_exec, h->graph, nullptr, nullptr, 0));
  return AUV_OK;
}

int auv_graph_launch(auv_handle_t* h, void* stream) {
  REQUIRE_READY(h);
  if (!h->graph_exec) return fail(AUV_ESTATE, "auv_graph_launch: no captured graph");
  PAIR_CHECK(h, nullptr);
  if (h->fw.on) {
    const int32_t whole[2] = {0, h->d.n};
    int rc_t = fw_tick(h, 1, whole, &stream, h->graph_steps);
    if (rc_t) return rc_t;
  }
  HIP_TRY(hipGraphLaunch(h->graph_exec, (hipStream_t)stream));
  return AUV_OK;
}

int auv_step_timed(auv_handle_t* h, const void* actions_dev, int32_t action_dtype, float* obs_dev, float* reward_dev,
                   uint8_t* done_dev, void* stream, float* out_ms4) {
  REQUIRE_READY(h);
  if (!out_ms4) return fail(AUV_EINVAL, "auv_step_timed: null argument");
  {
    int rc_a = check_actions(actions_dev, action_dtype, "auv_step_timed");
    if (rc_a) return rc_a;
  }
  PAIR_CHECK(h, obs_dev);
  hipStream_t st = (hipStream_t)stream;
  for (auto& e : h->ev)
    if (!e) HIP_TRY(hipEventCreate(&e));
  AuvDev d = h->d;
  d.ring_slots = 1;   // eager: `actions_dev` is one plain [N][2] buffer (see enqueue_step)
  // every dispatch of the step is stamped with its own start and stop event (hipExtLaunchKernel): the
  // elapsed times are the kernels' own durations, as a kernel trace reports them, without the gaps
  int nk;
  const int mode = effective_mode(h, d.n);
  if (mode == AUV_STEP_ONE_LAUNCH) {
    auv_launch_step_roles(d, actions_dev, action_dtype, obs_dev, reward_dev, done_dev, st, h->ev[0], h->ev[1]);
    nk = 1;
  } else {
    if (!auv_k23_ok(d)) return fail(AUV_EINVAL, "auv_step_timed: path too long for the side-by-side launch");
    auv_launch_k1(d, actions_dev, action_dtype, st, h->ev[0], h->ev[1]);
    auv_launch_k23(d, obs_dev, st, h->ev[2], h->ev[3]);
    auv_launch_k3_reward(d, obs_dev, reward_dev, done_dev, d.cfg.use_lidar ? 0 : 1, st, h->ev[4], h->ev[5]);
    nk = 3;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventSynchronize(h->ev[2 * nk - 1]));
  out_ms4[1] = out_ms4[2] = 0.0f;
  for (int i = 0; i < nk; i++) HIP_TRY(hipEventElapsedTime(&out_ms4[i], h->ev[2 * i], h->ev[2 * i + 1]));
  HIP_TRY(hipEventElapsedTime(&out_ms4[3], h->ev[0], h->ev[2 * nk - 1]));   // whole step, first start to last stop
  return AUV_OK;
}

}  // extern "C"
