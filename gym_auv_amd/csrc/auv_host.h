// auv_host.h — what the host files of the C ABI share (auv_capi.hip, auv_capi_step.hip, auv_capi_learn.hip, auv_capi_aux.hip): the
// handle, error reporting, the checks every entry starts with, device-memory pools, and the few helpers called across files.
// Internal: not installed, included by no kernel file.  The helpers live in namespace auv_host, so none of them can collide with
// an entry of the ABI; each is defined once, in the file named beside its declaration.
#ifndef AUV_HOST_H
#define AUV_HOST_H
#include <hip/hip_runtime.h>

#include <vector>

#include "auv_device.h"
#include "auv_generate.h"
#include "auv_launch.h"

namespace auv_host {
// records the message auv_last_error() returns (thread-local, auv_capi.hip) and returns `code`
int fail(int code, const char* fmt, ...);
}  // namespace auv_host

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess) return auv_host::fail(AUV_EHIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                                __FILE__, __LINE__);                          \
  } while (0)

struct auv_handle {
  AuvDev d;
  int device;
  bool worlds_loaded;
  bool bank_seen = false;        // a bank has been loaded or generated once: the observation's layout is fixed from then on
  std::vector<uint32_t> pool_word_host;   // auv_set_obs_pooling: [S] sector word per sensor (AuvDev::pool_word), empty when off
  std::vector<void*> env_allocs, bank_allocs;
  hipStream_t cap_stream;
  hipGraph_t graph;
  hipGraphExec_t graph_exec;
  int step_mode;                 // AUV_STEP_* as requested (include/auv_hip.h)
  int32_t* pair_error_host;      // pinned, mapped: set by a wave of the one-launch step that gave up polling
  // in-launch hand-overs (the one-launch shape): allowed only while the load-time probe of the dispatch
  // order has passed and no poll has ever run out on this handle
  bool handover_ok;
  int probe_failures;            // of the last probe (0 = the dispatch order is what the hand-overs rely on)
  int handover_timeouts;         // polls that ran out over the life of the handle (each one disables the hand-overs)
  int last_timeout_e0, last_timeout_ne, last_reset_envs;   // the launch that reported the last time-out; environments its recovery reset
  hipEvent_t ev[6];
  std::vector<hipEvent_t> slice_ev;   // auv_step_pipelined_timed: start / stop event per sub-batch launch
  // auv_step_async / auv_step_wait: the chains of the pending step that do NOT run on the caller's stream, and how
  // they are ordered against it (0: no step pending, else 1 + AUV_RDV_*)
  int async_pending;
  std::vector<hipStream_t> async_streams;
  hipEvent_t ev_actions;              // AUV_RDV_EVENTS: recorded on the caller's stream behind the actions
  std::vector<hipEvent_t> ev_chain;   //                 recorded behind each chain's launch
  unsigned long long* rdv;            // AUV_RDV_DEVICE / _CP: words in device (signal) memory, one 128-byte line each:
                                      //   [0] actions-ready sequence, [16] chains-arrived count, [32 + 16 j] chain j's sequence
  unsigned long long rdv_seq, rdv_target;
  double rdv_limit_s;                 // how long a rendezvous kernel waits before it gives up (pair_error 4 / 5)
  bool rdv_device_ok;                 // AUV_RDV_DEVICE may be used: false once a trial or a real rendezvous has run out -- events from then on
  std::vector<hipStream_t> rdv_tried; // the remote streams the device rendezvous has been tried on (auv_step_async: rdv_trial)
  int rdv_timeouts;                   // rendezvous waits that ran out over the life of the handle (trial included)
  // captured chains (auv_graph_capture_chains): one linear graph per sub-batch, replayed on the sub-batch's stream
  std::vector<hipGraph_t> chain_graph;
  std::vector<hipGraphExec_t> chain_exec;
  std::vector<hipStream_t> fork_streams;   // side streams of the one-graph (fork / join) form
  std::vector<int32_t> chain_bounds;       // the slices of the captured chains
  int chain_steps = 1, graph_steps = 1;    // steps per replay of the captured chains / of the one graph
  unsigned long long multi_seq = 0;        // auv_step_multi: step numbers handed out so far (every mark of a step carries its number)
  int multi_order = 1, multi_lead = 16, multi_lag = 30;   // auv_set_multi_order: workgroup order of a launch of several steps
  // auv_render: the geometry pass's outputs and the device copy of the index list, for `render_cap` frames
  std::vector<void*> render_allocs;
  int render_cap = 0;
  // the index list travels through one of four pinned host slots (an event per slot: a slot is reused once the copy out of it is done)
  int32_t* r_pin = nullptr;
  hipEvent_t r_pin_ev[4] = {nullptr, nullptr, nullptr, nullptr};
  unsigned r_seq = 0;
#ifdef AUV_RENDER_DIAG
  unsigned long long* r_diag = nullptr;
#endif
  int32_t* r_idx = nullptr; double* r_cam = nullptr; double4* r_dyn = nullptr; double4* r_ray = nullptr; uint8_t* r_q = nullptr; int32_t* r_tlen = nullptr;
  unsigned int* snap_skipped = nullptr;    // [1] device: pairs auv_snapshot / auv_restore skipped for an index out of range (restarts with every bank)
  // on-device generation (auv_generate_worlds): shape of the slot bank, 0 = packed upload
  int gen_worlds, gen_moving, gen_static, gen_grid;
  GenOut gen;
  // a fresh world on every reset (auv_fresh_worlds_create): the refill pass and its bookkeeping
  struct Fresh {
    bool on = false;
    int depth = 0, cap = 0, period = 0, n_draws = 0;
    unsigned long long seed = 0;
    long long env_base = 0;
    hipStream_t side = nullptr;               // the refill pass's stream: a plain stream of the library's, or the caller's choice
    bool side_owned = false;                  // (auv_fresh_worlds_set_stream: one that shares no hardware queue with the chains)
    std::vector<void*> allocs;                // shadow environments + queue / state words
    AuvDev shadow;                            // `cap` environments nobody steps: where a regenerated slot's reset rows are computed
    FwBatch batch;                            // device: the pass in flight on `side`
    int32_t* batch_block = nullptr;           // [1 + 3 cap]: count, slot[], env[], serial[] (one D2H copy per pass)
    double* draws = nullptr;                  // [cap][n_draws]
    int32_t* env_next_serial = nullptr;       // [N]
    static const int NEV = 64;                // pacing events (ring): a pass starts when chain 0 has reached the step it was enqueued behind
    hipEvent_t pace[NEV];
    unsigned long long issued = 0, calls = 0, paced = 0;   // passes enqueued, step calls counted, pacing events handed out
    bool multi = false;                       // auv_fresh_worlds_multi: launches of several steps allowed (k_fresh_multi / k_fresh_record)
    bool feedback = false;                    // auv_fresh_worlds_multi(h, 2): the closed-loop entries too (k_fresh_feedback and its siblings)
    unsigned int multi_call = 0;             // multi-step calls so far: the number the next one's launches carry is this + 1
    hipGraphExec_t pass_exec = nullptr;       // the pass as ONE graph launch (captured at create)
    hipGraph_t pass_graph = nullptr;
  } fw;
};

// From how many environments per launch on the three-launch shape is used by AUV_STEP_AUTO.  With the four-role step
// the one launch is ahead at every size measured (one chain, tools/archive/auto_threshold.sh: 139.3 against 129.5 M env-steps/s
// at 8192 environments per launch, 149.1 / 141.4 M at 16384, 149.9 / 145.8 M at 32768): the margin halves with every
// doubling -- many rounds of waves per slot leave little to gain by hiding a launch boundary -- so beyond what was
// measured the fence-free shape is the default.  (With three roles the crossover was at 16384.)
#define AUV_AUTO_THREE_LAUNCHES_FROM 65536
#define AUV_MAX_CHAINS 64      // sub-batch chains per handle (BatchedAuvEnv.set_sub_batches allows up to 64)
#define AUV_RDV_WORDS (32 + 16 * AUV_MAX_CHAINS)       // rendezvous words, one 128-byte line each (auv_handle::rdv)
#define AUV_RDV_BYTES (AUV_RDV_WORDS * sizeof(unsigned long long))

namespace auv_host {

// The shape a step of `ne` environments is actually launched in: the requested one, degraded to the fence-free
// three-launch shape where the in-launch hand-overs may not be used (probe failed / a poll timed out / no LiDAR).
inline int effective_mode(const auv_handle* h, int ne) {
  int m = h->step_mode;
  if (m == AUV_STEP_AUTO) m = ne >= AUV_AUTO_THREE_LAUNCHES_FROM ? AUV_STEP_SIDE_BY_SIDE : AUV_STEP_ONE_LAUNCH;
  if (m != AUV_STEP_SIDE_BY_SIDE && (!h->handover_ok || !auv_roles_ok(h->d))) m = AUV_STEP_SIDE_BY_SIDE;
  return m;
}

// auv_capi.hip
void drop_graphs(auv_handle* h);
int fw_tick(auv_handle* h, int n_slices, const int32_t* bounds, void* const* streams, int n_steps = 1, bool all_chains = false);
// auv_capi_step.hip
int recover_from_timeout(auv_handle* h, float* obs_now);
int check_slices(const auv_handle* h, int32_t n_slices, const int32_t* bounds, const void* streams, const char* who);
int check_actions(const void* actions_dev, int32_t action_dtype, const char* who);
int enqueue_step(auv_handle* h, int mode, int e0, int ne, const void* actions, int32_t dtype, float* obs, float* reward, uint8_t* done,
                 hipStream_t st, bool capturing, bool skip_k1 = false, bool fuse_next = false, int chain = 0);

inline bool stream_capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return cs == hipStreamCaptureStatusActive;
}

template <typename T>
int dev_alloc(std::vector<void*>& pool, T** out, size_t count) {
  void* p = nullptr;
  size_t bytes = (count ? count : 1) * sizeof(T);
  HIP_TRY(hipMalloc(&p, bytes));
  HIP_TRY(hipMemset(p, 0, bytes));
  pool.push_back(p);
  *out = (T*)p;
  return AUV_OK;
}

template <typename T, typename U>
int dev_upload(std::vector<void*>& pool, const T** out, const U* host, size_t count_T) {
  T* p = nullptr;
  int rc = dev_alloc(pool, &p, count_T);
  if (rc) return rc;
  if (count_T) HIP_TRY(hipMemcpy(p, host, count_T * sizeof(T), hipMemcpyHostToDevice));
  *out = p;
  return AUV_OK;
}

inline void free_pool(std::vector<void*>& pool) {
  for (void* p : pool) (void)hipFree(p);
  pool.clear();
}

}  // namespace auv_host

// A wave of the one-launch step that gave up polling has left its environment's step unfinished.  The
// next call on the handle notices (mapped host word), repairs the handle -- hand-over words cleared, EVERY
// environment put back into its reset state, three-launch shape from now on -- and reports AUV_ESTATE once.
#define PAIR_CHECK(h, obs) PAIR_CHECK_ON(h, nullptr, false, obs)
// `st`: the stream the call will enqueue on.  While that stream is being CAPTURED (a torch CUDAGraph around auv_step /
// auv_step_slice, examples/ppo.py) the recovery -- device synchronisation, copies, a reset launch on the null stream --
// would be illegal and would surface as a HIP capture error: the call then only reports AUV_ESTATE; the first call
// outside a capture recovers.
// `obs`: the observation buffer of THIS call (NULL if it has none): where the recovery writes the reset rows of the environments it
// resets -- never a pointer remembered from an earlier call (the caller may have freed or rotated that buffer).
#define PAIR_CHECK_ON(h, st, have_st, obs)                                       \
  do {                                                                           \
    if ((h)->pair_error_host && *(volatile int32_t*)(h)->pair_error_host) {      \
      if ((have_st) && auv_host::stream_capturing((hipStream_t)(st)))            \
        return auv_host::fail(AUV_ESTATE, "a hand-over time-out is pending and this stream is being captured: nothing was enqueued; " \
                                "the next call outside a capture recovers and reports");      \
      int _rc = auv_host::recover_from_timeout(h, (float*)(obs));                \
      if (_rc) return _rc;                                                       \
    }                                                                            \
  } while (0)

#define REQUIRE_READY(h)                                                          \
  do {                                                                            \
    if (!(h)) return auv_host::fail(AUV_EINVAL, "null handle");                   \
    if (!(h)->worlds_loaded) return auv_host::fail(AUV_ESTATE, "auv_load_worlds not called"); \
  } while (0)

#endif  // AUV_HOST_H
