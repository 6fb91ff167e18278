// auv_capi_learn.hip — the C ABI's learning entries (include/auv_hip.h): the fused policy launches (act, eval, stacked, normalising) and
// their rollouts, auv_gae, the fold and the return pass of the running normalisation, the population of policies, and the PPO updater object.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>

#include "auv_host.h"
#include "auv_policy_mfma.h"
#include "auv_ppo.h"

using namespace auv_host;

extern "C" {

// the hidden widths of a forward launch: the entries without _arch evaluate the reference's net
static const auv_policy_arch_t POLICY_ARCH_REF = {POL_H1, POL_H2, POL_H3};
size_t auv_policy_param_floats(int32_t obs_dim) { return auv_policy_param_floats_arch(obs_dim, &POLICY_ARCH_REF); }

static int check_policy_arch(const auv_policy_arch_t* a, const void* params_bf16, const char* who) {
  if (!a) return fail(AUV_EINVAL, "%s: null arch", who);
  if (!pol_arch_listed(a->h1, a->h2, a->h3)) {
    char list[256] = "";                                  // "(256, 128, 64), (128, 128, 64), ..."
    pol_arch_any([&](auto t) {
      const size_t n = strlen(list);
      snprintf(list + n, sizeof(list) - n, "%s(%d, %d, %d)", n ? ", " : "", t.H1, t.H2, t.H3);
      return false;
    });
    return fail(AUV_EINVAL, "%s: hidden widths (%d, %d, %d) are not compiled in: one of %s", who, a->h1, a->h2, a->h3, list);
  }
  if (params_bf16 && !pol_arch_is_ref(a->h1, a->h2, a->h3))
    return fail(AUV_EINVAL, "%s: hidden widths (%d, %d, %d) are evaluated in exact f32 only (params_bf16 must be NULL)", who, a->h1, a->h2, a->h3);
  return AUV_OK;
}

size_t auv_policy_param_floats_arch(int32_t obs_dim, const auv_policy_arch_t* arch) {
  if (obs_dim <= 0 || !arch || !pol_arch_listed(arch->h1, arch->h2, arch->h3)) return 0;
  return auv_policy_param_floats_impl(arch->h1, arch->h2, arch->h3, obs_dim);
}

static int check_policy_io(const auv_handle_t* h, int32_t e0, int32_t ne, const auv_policy_io_t* io, const auv_policy_arch_t* a, const char* who) {
  if (!io) return fail(AUV_EINVAL, "%s: null io", who);
  int rca = check_policy_arch(a, io->params_bf16, who);
  if (rca) return rca;
  const int D = auv_obs_cols(h->d.cfg, h->d.pool_ns);
  if (io->obs_dim != D) return fail(AUV_EINVAL, "%s: obs_dim %d, the handle's observation has %d columns", who, io->obs_dim, D);
  if (e0 < 0 || ne < 1 || (int64_t)e0 + ne > h->d.n) return fail(AUV_EINVAL, "%s: slice [%d, %d) outside [0, %d)", who, e0, e0 + ne, h->d.n);
  if (io->T < 1) return fail(AUV_EINVAL, "%s: T must be >= 1", who);
  if (io->env_base < 0 || io->env_base > e0 || (int64_t)e0 + ne - io->env_base > io->ld)
    return fail(AUV_EINVAL, "%s: slice [%d, %d) does not fit a rollout row of %d environments starting at environment %d", who, e0, e0 + ne, io->ld, io->env_base);
  if (!io->obs || !io->params || !io->ctr || !io->reward_in || !io->done_in || !io->actions_out || !io->A || !io->LP || !io->V || !io->R || !io->Dn)
    return fail(AUV_EINVAL, "%s: null buffer", who);
  if (((uintptr_t)io->params & 15) || ((uintptr_t)io->params_bf16 & 15) || ((uintptr_t)io->actions_out & 7) || ((uintptr_t)io->ctr & 7))
    return fail(AUV_EINVAL, "%s: params must be 16-byte, actions_out and ctr 8-byte aligned", who);
  if (auv_policy_lds_bytes(a->h1, a->h2, a->h3, io->obs_dim) > 160 * 1024)
    return fail(AUV_EINVAL, "%s: observation too wide for the policy kernel's LDS tile", who);
  return AUV_OK;
}

int auv_gae(auv_handle_t* h, const float* R, const float* V, const float* Dn, const float* last_v, float gamma, float lam, float* adv_out,
            float* ret_out, int32_t T, int32_t N, void* stream) {
  if (!h) return fail(AUV_EINVAL, "null handle");
  if (!R || !V || !Dn || !last_v || !adv_out || !ret_out || T < 1 || N < 1) return fail(AUV_EINVAL, "auv_gae: bad arguments");
  HIP_TRY(hipSetDevice(h->device));
  auv_launch_gae(R, V, Dn, last_v, gamma, lam, adv_out, ret_out, T, N, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

// ---- the policy on arbitrary rows (include/auv_hip.h, auv_policy_eval; kernel: k9_policy_eval.hip) ----
static int policy_eval_impl(int32_t device, const auv_policy_eval_t* ev, const auv_policy_arch_t* a, void* stream, bool squash = false) {
  if (!ev) return fail(AUV_EINVAL, "auv_policy_eval: null ev");
  int rca = check_policy_arch(a, nullptr, "auv_policy_eval");
  if (rca) return rca;
  if (device < 0) return fail(AUV_EINVAL, "auv_policy_eval: device %d", device);
  if (ev->obs_dim < 1) return fail(AUV_EINVAL, "auv_policy_eval: obs_dim %d < 1", ev->obs_dim);
  if (ev->obs_dim > 16384 || auv_policy_lds_bytes(a->h1, a->h2, a->h3, ev->obs_dim) > 160 * 1024)
    return fail(AUV_EINVAL, "auv_policy_eval: obs_dim %d is too wide for the policy kernel's LDS tile", ev->obs_dim);
  if (ev->M < 0) return fail(AUV_EINVAL, "auv_policy_eval: M = %d < 0", ev->M);
  const bool want_pi = ev->mu || ev->action || ev->logp, want_v = ev->value != nullptr;
  if (!want_pi && !want_v) return fail(AUV_EINVAL, "auv_policy_eval: no output asked for (mu, action, value, logp are all NULL)");
  if (ev->logp && !ev->A) return fail(AUV_EINVAL, "auv_policy_eval: logp needs the actions A");
  if (!ev->params || !ev->X) return fail(AUV_EINVAL, "auv_policy_eval: null %s", !ev->params ? "params" : "X");
  if (ev->ldx < ev->obs_dim) return fail(AUV_EINVAL, "auv_policy_eval: ldx %lld < obs_dim %d", (long long)ev->ldx, ev->obs_dim);
  if (ev->action && ev->action_ld < 2) return fail(AUV_EINVAL, "auv_policy_eval: action_ld %d < 2", ev->action_ld);
  if ((uintptr_t)ev->params & 15) return fail(AUV_EINVAL, "auv_policy_eval: params must be 16-byte aligned");
  if (((uintptr_t)ev->X & 3) || ((uintptr_t)ev->A & 3) || ((uintptr_t)ev->mu & 3) || ((uintptr_t)ev->action & 3) || ((uintptr_t)ev->value & 3) ||
      ((uintptr_t)ev->logp & 3) || ((uintptr_t)ev->idx & 7))
    return fail(AUV_EINVAL, "auv_policy_eval: float buffers must be 4-byte, idx 8-byte aligned");
  if (ev->M == 0) return AUV_OK;
  HIP_TRY(hipSetDevice(device));
  if (squash) {
    HIP_TRY(auv_policy_squash_prepare(a->h1, a->h2, a->h3, ev->obs_dim, true));
    auv_launch_policy_eval_squash(a->h1, a->h2, a->h3, *ev, want_pi, want_v, (hipStream_t)stream);
  } else {
    HIP_TRY(auv_policy_eval_prepare(a->h1, a->h2, a->h3, ev->obs_dim));
    auv_launch_policy_eval(a->h1, a->h2, a->h3, *ev, want_pi, want_v, (hipStream_t)stream);
  }
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}
// (the messages name auv_policy_eval: the checks are its own)
int auv_policy_eval_squash(int32_t device, const auv_policy_eval_t* ev, void* stream) {
  return policy_eval_impl(device, ev, &POLICY_ARCH_REF, stream, true);
}
int auv_policy_eval_squash_arch(int32_t device, const auv_policy_eval_t* ev, const auv_policy_arch_t* arch, void* stream) {
  return policy_eval_impl(device, ev, arch, stream, true);
}
int auv_policy_eval(int32_t device, const auv_policy_eval_t* ev, void* stream) { return policy_eval_impl(device, ev, &POLICY_ARCH_REF, stream); }
int auv_policy_eval_arch(int32_t device, const auv_policy_eval_t* ev, const auv_policy_arch_t* arch, void* stream) {
  return policy_eval_impl(device, ev, arch, stream);
}

// ---- rollouts: a launch that acts, then a step of the environment, per slice on its own stream, n_steps times ----
// The loop the three rollout calls share.  launch(i, k, flushing): the acting launch of slice i in front of step k of this call and,
// flushing, the one behind the last step (k == n_steps) that only books what that step has left; actions_of(i): the [N][2] float
// buffer the launch writes and the step reads.  The caller has checked its arguments, run PAIR_CHECK and prepared its kernel.  The
// first error stops the enqueuing and is returned before anything is flushed.
extern "C++" template <class ActionsOf, class Launch>
static int rollout_loop(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, float* obs_dev, float* reward_dev,
                        uint8_t* done_dev, int32_t n_steps, int32_t flush, ActionsOf actions_of, Launch launch) {
  int rc = AUV_OK;
  for (int32_t k = 0; k < n_steps; k++) {
    if (rc == AUV_OK) rc = fw_tick(h, n_slices, bounds, streams);
    for (int i = 0; i < n_slices && rc == AUV_OK; i++) {
      const int ne = bounds[i + 1] - bounds[i];
      launch(i, k, false);
      rc = enqueue_step(h, effective_mode(h, ne), bounds[i], ne, actions_of(i), AUV_F32, obs_dev, reward_dev, done_dev,
                        (hipStream_t)streams[i], false);
    }
  }
  if (rc) return rc;
  if (flush)
    for (int i = 0; i < n_slices; i++) launch(i, n_steps, true);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

// t0 / gstep0 of a policy rollout (per slice; both or neither): the host names every launch's rollout position and generator step
// (a rollout is a plain loop of launches, the values are known on the host) -- the launches then neither read nor count off on
// io.ctr, which is worth ~4 us per launch.  NULL: the device counters, as auv_policy_act; the kernel is told -1.
struct RolloutCounters {
  const int64_t *t0, *gstep0;
  bool paired() const { return (!t0) == (!gstep0); }
  bool negative(int i) const { return t0 && (t0[i] < 0 || gstep0[i] < 0); }
  long long t(int i, int32_t k) const { return t0 ? t0[i] + k : -1; }
  long long gstep(int i, int32_t k) const { return t0 ? gstep0[i] + k : -1; }
};

// ---- the four act launches behind the sixteen act / rollout entries: one variant trait each ----
// V::io_t the entry's io struct; V::check one slice's io (check_policy_io first, then the variant's own); V::check_uniform what must
// agree between the slices of a rollout; V::prepare / V::launch the kernel file's pair; V::actions_out the [N][2] buffer the launch
// writes and the step reads.
namespace {
struct PolicyPlain {
  typedef auv_policy_io_t io_t;
  static int check(const auv_handle_t* h, int32_t e0, int32_t ne, const io_t* io, const auv_policy_arch_t* a, const char* who) {
    return check_policy_io(h, e0, ne, io, a, who);
  }
  static int check_uniform(const io_t*, int, const char*) { return AUV_OK; }
  static hipError_t prepare(const auv_policy_arch_t* a, const io_t& io) { return auv_policy_prepare(a->h1, a->h2, a->h3, io.obs_dim); }
  static void launch(const auv_policy_arch_t* a, const io_t& io, int32_t e0, int32_t ne, hipStream_t st, long long t, long long gstep) {
    auv_launch_policy(a->h1, a->h2, a->h3, io, e0, ne, st, t, gstep);
  }
  static float* actions_out(const io_t& io) { return io.actions_out; }
};

// the launch of a tanh-squashed policy (k17_policy_squash.hip) in the place of the plain one: the same checks, exact f32 only
struct PolicySquash : PolicyPlain {
  static int check(const auv_handle_t* h, int32_t e0, int32_t ne, const io_t* io, const auv_policy_arch_t* a, const char* who) {
    int rc = check_policy_io(h, e0, ne, io, a, who);
    if (rc) return rc;
    if (io->params_bf16) return fail(AUV_EINVAL, "%s: a squashed policy is evaluated in exact f32 only (params_bf16 must be NULL)", who);
    return AUV_OK;
  }
  static hipError_t prepare(const auv_policy_arch_t* a, const io_t& io) { return auv_policy_squash_prepare(a->h1, a->h2, a->h3, io.obs_dim, false); }
  static void launch(const auv_policy_arch_t* a, const io_t& io, int32_t e0, int32_t ne, hipStream_t st, long long t, long long gstep) {
    auv_launch_policy_squash(a->h1, a->h2, a->h3, io, e0, ne, st, t, gstep);
  }
};

// frame-stacked observations (include/auv_hip.h, auv_policy_stack; kernels: k12_policy_stacked.hip)
struct PolicyStacked {
  typedef auv_policy_stack_t io_t;
  static int check(const auv_handle_t* h, int32_t e0, int32_t ne, const io_t* s, const auv_policy_arch_t* a, const char* who) {
    if (!s) return fail(AUV_EINVAL, "%s: null io", who);
    if (s->frames < 1 || s->frames > AUV_MAX_FRAMES) return fail(AUV_EINVAL, "%s: frames = %d outside [1, %d]", who, s->frames, AUV_MAX_FRAMES);
    int rc = check_policy_io(h, e0, ne, &s->io, a, who);
    if (rc) return rc;
    if (s->io.params_bf16) return fail(AUV_EINVAL, "%s: stacked rows are evaluated in exact f32 only (params_bf16 must be NULL)", who);
    const int64_t width = (int64_t)s->frames * s->io.obs_dim;
    if (width > 16384 || auv_policy_stacked_lds_bytes(a->h1, a->h2, a->h3, (int)width) > 160 * 1024)
      return fail(AUV_EINVAL, "%s: %d frames of %d columns are too wide for the policy kernel's LDS tile", who, s->frames, s->io.obs_dim);
    if (s->frames > 1) {
      if (!s->hist || !s->stk) return fail(AUV_EINVAL, "%s: null hist or stk", who);
      if (((uintptr_t)s->hist & 15) || ((uintptr_t)s->stk & 7)) return fail(AUV_EINVAL, "%s: hist must be 16-byte, stk 8-byte aligned", who);
    }
    return AUV_OK;
  }
  static int check_uniform(const io_t* ios, int i, const char* who) {
    if (ios[i].frames != ios[0].frames) return fail(AUV_EINVAL, "%s: slice %d has %d frames, slice 0 has %d", who, i, ios[i].frames, ios[0].frames);
    return AUV_OK;
  }
  static hipError_t prepare(const auv_policy_arch_t* a, const io_t& s) { return auv_policy_stacked_prepare(a->h1, a->h2, a->h3, s.frames * s.io.obs_dim); }
  static void launch(const auv_policy_arch_t* a, const io_t& s, int32_t e0, int32_t ne, hipStream_t st, long long t, long long gstep) {
    auv_launch_policy_stacked(a->h1, a->h2, a->h3, s, e0, ne, st, t, gstep);
  }
  static float* actions_out(const io_t& s) { return s.io.actions_out; }
};

// running normalisation (include/auv_hip.h, auv_policy_norm; kernels: k16_policy_norm.hip)
struct PolicyNorm {
  typedef auv_policy_norm_t io_t;
  static int check(const auv_handle_t* h, int32_t e0, int32_t ne, const io_t* s, const auv_policy_arch_t* a, const char* who) {
    if (!s) return fail(AUV_EINVAL, "%s: null io", who);
    int rc = check_policy_io(h, e0, ne, &s->io, a, who);
    if (rc) return rc;
    if (s->io.params_bf16) return fail(AUV_EINVAL, "%s: normalised rows are evaluated in exact f32 only (params_bf16 must be NULL)", who);
    if (!s->table || ((uintptr_t)s->table & 7)) return fail(AUV_EINVAL, "%s: table must be an 8-byte aligned device pointer", who);
    if (!s->part || !s->pcnt) return fail(AUV_EINVAL, "%s: null part or pcnt", who);
    if (((uintptr_t)s->part & 3) || ((uintptr_t)s->pcnt & 3)) return fail(AUV_EINVAL, "%s: part and pcnt must be 4-byte aligned", who);
    if (!(s->clip_obs > 0.0f)) return fail(AUV_EINVAL, "%s: clip_obs must be > 0", who);
    const int tiles = (ne + POL_ROWS - 1) / POL_ROWS;
    if (s->part_base < 0 || (int64_t)s->part_base + tiles > s->part_ld)
      return fail(AUV_EINVAL, "%s: %d tiles from part_base %d do not fit part_ld = %d", who, tiles, s->part_base, s->part_ld);
    return AUV_OK;
  }
  static int check_uniform(const io_t*, int, const char*) { return AUV_OK; }
  static hipError_t prepare(const auv_policy_arch_t* a, const io_t& s) { return auv_policy_norm_prepare(a->h1, a->h2, a->h3, s.io.obs_dim); }
  static void launch(const auv_policy_arch_t* a, const io_t& s, int32_t e0, int32_t ne, hipStream_t st, long long t, long long gstep) {
    auv_launch_policy_norm(a->h1, a->h2, a->h3, s, e0, ne, st, t, gstep);
  }
  static float* actions_out(const io_t& s) { return s.io.actions_out; }
};
}  // namespace

// one acting launch of the slice [e0, e0 + ne) on `stream`: the counters live on the device (io.ctr)
extern "C++" template <class V>
static int policy_act_impl(auv_handle_t* h, int32_t e0, int32_t ne, const typename V::io_t* io, const auv_policy_arch_t* a, void* stream,
                           const char* who) {
  REQUIRE_READY(h);
  int rc = V::check(h, e0, ne, io, a, who);
  if (rc) return rc;
  HIP_TRY(V::prepare(a, *io));
  V::launch(a, *io, e0, ne, (hipStream_t)stream, -1, -1);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

// the rollout loop with a variant's launch: the t0 / gstep0 contract above, every slice on its own stream
extern "C++" template <class V>
static int policy_rollout_impl(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const typename V::io_t* ios,
                               const auv_policy_arch_t* a, float* obs_dev, float* reward_dev, uint8_t* done_dev, int32_t n_steps, int32_t flush,
                               const int64_t* t0, const int64_t* gstep0, const char* who) {
  REQUIRE_READY(h);
  const RolloutCounters ctr = {t0, gstep0};
  int rc = check_slices(h, n_slices, bounds, streams, who);
  if (rc) return rc;
  if (!ios || n_steps < 0 || !ctr.paired()) return fail(AUV_EINVAL, "%s: bad arguments", who);
  for (int i = 0; i < n_slices; i++) {
    rc = V::check(h, bounds[i], bounds[i + 1] - bounds[i], ios + i, a, who);
    if (rc) return rc;
    rc = check_actions(V::actions_out(ios[i]), AUV_F32, who);
    if (rc) return rc;
    rc = V::check_uniform(ios, i, who);
    if (rc) return rc;
    if (ctr.negative(i)) return fail(AUV_EINVAL, "%s: negative counter for slice %d", who, i);
  }
  PAIR_CHECK(h, obs_dev);
  HIP_TRY(V::prepare(a, ios[0]));
  return rollout_loop(
      h, n_slices, bounds, streams, obs_dev, reward_dev, done_dev, n_steps, flush, [&](int i) { return V::actions_out(ios[i]); },
      [&](int i, int32_t k, bool) {
        V::launch(a, ios[i], bounds[i], bounds[i + 1] - bounds[i], (hipStream_t)streams[i], ctr.t(i, k), ctr.gstep(i, k));
      });
}

// the sixteen entries: (act, rollout) x (plain, squash, stacked, norm) x (the reference's widths, _arch), each under its own name
int auv_policy_act(auv_handle_t* h, int32_t e0, int32_t ne, const auv_policy_io_t* io, void* stream) {
  return policy_act_impl<PolicyPlain>(h, e0, ne, io, &POLICY_ARCH_REF, stream, "auv_policy_act");
}
int auv_policy_act_arch(auv_handle_t* h, int32_t e0, int32_t ne, const auv_policy_io_t* io, const auv_policy_arch_t* arch, void* stream) {
  return policy_act_impl<PolicyPlain>(h, e0, ne, io, arch, stream, "auv_policy_act_arch");
}
int auv_policy_rollout(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const auv_policy_io_t* ios, float* obs_dev,
    float* reward_dev, uint8_t* done_dev, int32_t n_steps, int32_t flush, const int64_t* t0, const int64_t* gstep0) {
  return policy_rollout_impl<PolicyPlain>(h, n_slices, bounds, streams, ios, &POLICY_ARCH_REF, obs_dev, reward_dev, done_dev, n_steps, flush, t0, gstep0, "auv_policy_rollout");
}
int auv_policy_rollout_arch(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const auv_policy_io_t* ios, const auv_policy_arch_t* arch,
    float* obs_dev, float* reward_dev, uint8_t* done_dev, int32_t n_steps, int32_t flush, const int64_t* t0, const int64_t* gstep0) {
  return policy_rollout_impl<PolicyPlain>(h, n_slices, bounds, streams, ios, arch, obs_dev, reward_dev, done_dev, n_steps, flush, t0, gstep0, "auv_policy_rollout_arch");
}
int auv_policy_act_squash(auv_handle_t* h, int32_t e0, int32_t ne, const auv_policy_io_t* io, void* stream) {
  return policy_act_impl<PolicySquash>(h, e0, ne, io, &POLICY_ARCH_REF, stream, "auv_policy_act_squash");
}
int auv_policy_act_squash_arch(auv_handle_t* h, int32_t e0, int32_t ne, const auv_policy_io_t* io, const auv_policy_arch_t* arch, void* stream) {
  return policy_act_impl<PolicySquash>(h, e0, ne, io, arch, stream, "auv_policy_act_squash_arch");
}
int auv_policy_rollout_squash(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const auv_policy_io_t* ios, float* obs_dev,
    float* reward_dev, uint8_t* done_dev, int32_t n_steps, int32_t flush, const int64_t* t0, const int64_t* gstep0) {
  return policy_rollout_impl<PolicySquash>(h, n_slices, bounds, streams, ios, &POLICY_ARCH_REF, obs_dev, reward_dev, done_dev, n_steps, flush, t0, gstep0, "auv_policy_rollout_squash");
}
int auv_policy_rollout_squash_arch(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const auv_policy_io_t* ios, const auv_policy_arch_t* arch,
    float* obs_dev, float* reward_dev, uint8_t* done_dev, int32_t n_steps, int32_t flush, const int64_t* t0, const int64_t* gstep0) {
  return policy_rollout_impl<PolicySquash>(h, n_slices, bounds, streams, ios, arch, obs_dev, reward_dev, done_dev, n_steps, flush, t0, gstep0, "auv_policy_rollout_squash_arch");
}
int auv_policy_act_stacked(auv_handle_t* h, int32_t e0, int32_t ne, const auv_policy_stack_t* io, void* stream) {
  return policy_act_impl<PolicyStacked>(h, e0, ne, io, &POLICY_ARCH_REF, stream, "auv_policy_act_stacked");
}
int auv_policy_act_stacked_arch(auv_handle_t* h, int32_t e0, int32_t ne, const auv_policy_stack_t* io, const auv_policy_arch_t* arch, void* stream) {
  return policy_act_impl<PolicyStacked>(h, e0, ne, io, arch, stream, "auv_policy_act_stacked_arch");
}
int auv_policy_rollout_stacked(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const auv_policy_stack_t* ios, float* obs_dev,
    float* reward_dev, uint8_t* done_dev, int32_t n_steps, int32_t flush, const int64_t* t0, const int64_t* gstep0) {
  return policy_rollout_impl<PolicyStacked>(h, n_slices, bounds, streams, ios, &POLICY_ARCH_REF, obs_dev, reward_dev, done_dev, n_steps, flush, t0, gstep0, "auv_policy_rollout_stacked");
}
int auv_policy_rollout_stacked_arch(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const auv_policy_stack_t* ios, const auv_policy_arch_t* arch,
    float* obs_dev, float* reward_dev, uint8_t* done_dev, int32_t n_steps, int32_t flush, const int64_t* t0, const int64_t* gstep0) {
  return policy_rollout_impl<PolicyStacked>(h, n_slices, bounds, streams, ios, arch, obs_dev, reward_dev, done_dev, n_steps, flush, t0, gstep0, "auv_policy_rollout_stacked_arch");
}
int auv_policy_act_norm(auv_handle_t* h, int32_t e0, int32_t ne, const auv_policy_norm_t* io, void* stream) {
  return policy_act_impl<PolicyNorm>(h, e0, ne, io, &POLICY_ARCH_REF, stream, "auv_policy_act_norm");
}
int auv_policy_act_norm_arch(auv_handle_t* h, int32_t e0, int32_t ne, const auv_policy_norm_t* io, const auv_policy_arch_t* arch, void* stream) {
  return policy_act_impl<PolicyNorm>(h, e0, ne, io, arch, stream, "auv_policy_act_norm_arch");
}
int auv_policy_rollout_norm(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const auv_policy_norm_t* ios, float* obs_dev,
    float* reward_dev, uint8_t* done_dev, int32_t n_steps, int32_t flush, const int64_t* t0, const int64_t* gstep0) {
  return policy_rollout_impl<PolicyNorm>(h, n_slices, bounds, streams, ios, &POLICY_ARCH_REF, obs_dev, reward_dev, done_dev, n_steps, flush, t0, gstep0, "auv_policy_rollout_norm");
}
int auv_policy_rollout_norm_arch(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const auv_policy_norm_t* ios, const auv_policy_arch_t* arch,
    float* obs_dev, float* reward_dev, uint8_t* done_dev, int32_t n_steps, int32_t flush, const int64_t* t0, const int64_t* gstep0) {
  return policy_rollout_impl<PolicyNorm>(h, n_slices, bounds, streams, ios, arch, obs_dev, reward_dev, done_dev, n_steps, flush, t0, gstep0, "auv_policy_rollout_norm_arch");
}

// ---- the history update alone (include/auv_hip.h, auv_stack_frames; kernel: k12_policy_stacked.hip) ----
int auv_stack_frames(int32_t device, const float* obs, const uint8_t* done, float* hist, int32_t* stk, float* out, int64_t ldx, int32_t e0,
                     int32_t ne, int32_t obs_dim, int32_t frames, int32_t advance, void* stream) {
  if (device < 0) return fail(AUV_EINVAL, "auv_stack_frames: device %d", device);
  if (obs_dim < 1 || obs_dim > 16384) return fail(AUV_EINVAL, "auv_stack_frames: obs_dim %d outside [1, 16384]", obs_dim);
  if (frames < 1 || frames > AUV_MAX_FRAMES) return fail(AUV_EINVAL, "auv_stack_frames: frames = %d outside [1, %d]", frames, AUV_MAX_FRAMES);
  if (e0 < 0 || ne < 0 || (int64_t)e0 + ne > INT32_MAX) return fail(AUV_EINVAL, "auv_stack_frames: rows [%d, %d + %d)", e0, e0, ne);
  if (!obs || !out) return fail(AUV_EINVAL, "auv_stack_frames: null %s", !obs ? "obs" : "out");
  if (ldx < (int64_t)frames * obs_dim) return fail(AUV_EINVAL, "auv_stack_frames: ldx %lld < frames * obs_dim = %d", (long long)ldx, frames * obs_dim);
  if (frames > 1 && (!hist || !stk)) return fail(AUV_EINVAL, "auv_stack_frames: null hist or stk");
  if (((uintptr_t)obs & 3) || ((uintptr_t)out & 3) || ((uintptr_t)hist & 3) || ((uintptr_t)stk & 7))
    return fail(AUV_EINVAL, "auv_stack_frames: obs, out and hist must be 4-byte, stk 8-byte aligned");
  if (ne == 0) return AUV_OK;
  HIP_TRY(hipSetDevice(device));
  auv_launch_stack_frames(obs, done, hist, stk, out, ldx, e0, ne, obs_dim, frames, advance != 0, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

// ---- running normalisation: the same expression on arbitrary rows, the fold and the return pass (kernels: k16_policy_norm.hip) ----
static bool norm_finite(double x) { return x == x && x - x == 0.0; }

int auv_norm_rows(int32_t device, const float* X, const int64_t* idx, int64_t ldx, const float* table, float clip_obs, float* out, int64_t ldo,
                  int32_t M, int32_t obs_dim, void* stream) {
  if (device < 0) return fail(AUV_EINVAL, "auv_norm_rows: device %d", device);
  if (obs_dim < 1 || obs_dim > 16384) return fail(AUV_EINVAL, "auv_norm_rows: obs_dim %d outside [1, 16384]", obs_dim);
  if (M < 0) return fail(AUV_EINVAL, "auv_norm_rows: M = %d < 0", M);
  if (!X || !out || !table) return fail(AUV_EINVAL, "auv_norm_rows: null %s", !X ? "X" : !out ? "out" : "table");
  if (((uintptr_t)table & 7) || ((uintptr_t)idx & 7) || ((uintptr_t)X & 3) || ((uintptr_t)out & 3))
    return fail(AUV_EINVAL, "auv_norm_rows: table and idx must be 8-byte, X and out 4-byte aligned");
  if (ldx < obs_dim || ldo < obs_dim) return fail(AUV_EINVAL, "auv_norm_rows: ldx %lld or ldo %lld < obs_dim %d", (long long)ldx, (long long)ldo, obs_dim);
  if (!(clip_obs > 0.0f)) return fail(AUV_EINVAL, "auv_norm_rows: clip_obs must be > 0");
  if (M == 0) return AUV_OK;
  HIP_TRY(hipSetDevice(device));
  auv_launch_norm_rows(X, idx, ldx, table, clip_obs, out, ldo, M, obs_dim, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

int auv_norm_fold(int32_t device, const float* part, const int32_t* pcnt, int32_t n_slots, int32_t obs_dim, double eps, double* mom, float* table,
                  void* stream) {
  if (device < 0) return fail(AUV_EINVAL, "auv_norm_fold: device %d", device);
  if (obs_dim < 1 || obs_dim > 16384) return fail(AUV_EINVAL, "auv_norm_fold: obs_dim %d outside [1, 16384]", obs_dim);
  if (n_slots < 1) return fail(AUV_EINVAL, "auv_norm_fold: n_slots = %d < 1", n_slots);
  if (!part || !pcnt || !mom || !table) return fail(AUV_EINVAL, "auv_norm_fold: null buffer");
  if (((uintptr_t)part & 3) || ((uintptr_t)pcnt & 3) || ((uintptr_t)mom & 7) || ((uintptr_t)table & 7))
    return fail(AUV_EINVAL, "auv_norm_fold: part and pcnt must be 4-byte, mom and table 8-byte aligned");
  if (!norm_finite(eps) || eps < 0.0) return fail(AUV_EINVAL, "auv_norm_fold: eps must be finite and >= 0");
  HIP_TRY(hipSetDevice(device));
  auv_launch_norm_fold(part, pcnt, n_slots, obs_dim, eps, mom, table, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

int auv_norm_returns(int32_t device, const float* R, const float* Dn, float* R_out, int32_t T, int32_t N, double gamma, float clip_reward,
                     double eps, double* ret, double* rpart, double* rmom, int32_t update, void* stream) {
  if (device < 0) return fail(AUV_EINVAL, "auv_norm_returns: device %d", device);
  if (T < 1 || N < 1) return fail(AUV_EINVAL, "auv_norm_returns: T = %d, N = %d", T, N);
  if (!R || !R_out || !rmom) return fail(AUV_EINVAL, "auv_norm_returns: null %s", !R ? "R" : !R_out ? "R_out" : "rmom");
  if (update && (!Dn || !ret || !rpart)) return fail(AUV_EINVAL, "auv_norm_returns: update needs Dn, ret and rpart");
  if (((uintptr_t)R & 3) || ((uintptr_t)R_out & 3) || ((uintptr_t)Dn & 3) || ((uintptr_t)ret & 7) || ((uintptr_t)rpart & 7) || ((uintptr_t)rmom & 7))
    return fail(AUV_EINVAL, "auv_norm_returns: float buffers must be 4-byte, double buffers 8-byte aligned");
  if (!(clip_reward > 0.0f)) return fail(AUV_EINVAL, "auv_norm_returns: clip_reward must be > 0");
  if (!norm_finite(gamma) || !norm_finite(eps) || eps < 0.0) return fail(AUV_EINVAL, "auv_norm_returns: gamma and eps must be finite, eps >= 0");
  HIP_TRY(hipSetDevice(device));
  auv_launch_norm_returns(R, Dn, R_out, T, N, gamma, clip_reward, eps, ret, rpart, rmom, update != 0, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

// ---- a population of policies (include/auv_hip.h, auv_population_*; kernels: k11_population.hip, k14_population_arch.hip) ----
// The entries without _arch evaluate the reference's net: they are the _arch ones with POLICY_ARCH_REF, under their own names in the
// error strings.  `a` is checked first (check_policy_arch); every check behind it is the plain entries', with the member size and the
// LDS tile of the triple.
size_t auv_population_member_floats(int32_t obs_dim) { return auv_population_member_floats_arch(obs_dim, &POLICY_ARCH_REF); }

size_t auv_population_member_floats_arch(int32_t obs_dim, const auv_policy_arch_t* arch) {
  if (obs_dim <= 0 || !arch) return 0;
  return auv_population_member_floats_impl(*arch, obs_dim);          // (0 for an unlisted triple)
}

static int check_population_obs_dim(const auv_policy_arch_t& a, int32_t obs_dim, const char* who) {
  if (obs_dim < 1) return fail(AUV_EINVAL, "%s: obs_dim %d < 1", who, obs_dim);
  if (obs_dim > 16384 || auv_policy_lds_bytes(a.h1, a.h2, a.h3, obs_dim) > 160 * 1024)
    return fail(AUV_EINVAL, "%s: obs_dim %d is too wide for the policy kernel's LDS tile", who, obs_dim);
  return AUV_OK;
}

// what every population launch needs of `io`, whatever its rows are
static int check_population_io(const auv_policy_arch_t& a, const auv_population_io_t* io, const char* who) {
  if (!io) return fail(AUV_EINVAL, "%s: null io", who);
  int rc = check_population_obs_dim(a, io->obs_dim, who);
  if (rc) return rc;
  if (io->G < 16 || io->G % 16) return fail(AUV_EINVAL, "%s: G = %d rows per member must be a positive multiple of 16", who, io->G);
  if (!io->members || ((uintptr_t)io->members & 15)) return fail(AUV_EINVAL, "%s: members must be a 16-byte aligned device pointer", who);
  if (io->stride < (int64_t)auv_population_member_floats_impl(a, io->obs_dim) || (io->stride & 3))
    return fail(AUV_EINVAL, "%s: stride %lld must be a multiple of 4 and >= auv_population_member_floats(%d) = %zu", who, (long long)io->stride,
                io->obs_dim, auv_population_member_floats_impl(a, io->obs_dim));
  if (io->M < 0) return fail(AUV_EINVAL, "%s: M = %d < 0", who, io->M);
  if (io->action && io->action_ld < 2) return fail(AUV_EINVAL, "%s: action_ld %d < 2", who, io->action_ld);
  if (((uintptr_t)io->mu & 3) || ((uintptr_t)io->action & 3) || ((uintptr_t)io->fit & 3) || ((uintptr_t)io->ends & 3))
    return fail(AUV_EINVAL, "%s: mu, action, fit and ends must be 4-byte aligned", who);
  return AUV_OK;
}

static int population_act_impl(int32_t device, const auv_population_io_t* io, const auv_policy_arch_t* arch, void* stream, const char* who) {
  if (device < 0) return fail(AUV_EINVAL, "%s: device %d", who, device);
  int rc = check_policy_arch(arch, nullptr, who);
  if (rc) return rc;
  const auv_policy_arch_t a = *arch;
  rc = check_population_io(a, io, who);
  if (rc) return rc;
  if (io->accumulate && (!io->reward_in || !io->done_in || !io->fit || !io->ends))
    return fail(AUV_EINVAL, "%s: accumulate needs reward_in, done_in, fit and ends", who);
  if (io->accumulate && ((uintptr_t)io->reward_in & 3)) return fail(AUV_EINVAL, "%s: reward_in must be 4-byte aligned", who);
  if (io->act) {
    if (!io->mu && !io->action && !io->accumulate) return fail(AUV_EINVAL, "%s: no output asked for (mu and action are NULL) and no accumulation", who);
    if (!io->X || ((uintptr_t)io->X & 3)) return fail(AUV_EINVAL, "%s: X must be a 4-byte aligned device pointer", who);
    if (io->ldx < io->obs_dim) return fail(AUV_EINVAL, "%s: ldx %lld < obs_dim %d", who, (long long)io->ldx, io->obs_dim);
  } else if (!io->accumulate) {
    return fail(AUV_EINVAL, "%s: neither act nor accumulate", who);
  }
  if (io->M == 0) return AUV_OK;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(auv_population_prepare(a, io->obs_dim));
  auv_launch_population_act(a, *io, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}
int auv_population_act(int32_t device, const auv_population_io_t* io, void* stream) {
  return population_act_impl(device, io, &POLICY_ARCH_REF, stream, "auv_population_act");
}
int auv_population_act_arch(int32_t device, const auv_population_io_t* io, const auv_policy_arch_t* arch, void* stream) {
  return population_act_impl(device, io, arch, stream, "auv_population_act_arch");
}

static int population_rollout_impl(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const auv_population_io_t* ios,
                                   const auv_policy_arch_t* arch, float* obs_dev, float* reward_dev, uint8_t* done_dev, int32_t n_steps,
                                   int32_t flush, const char* who) {
  REQUIRE_READY(h);
  int rc = check_policy_arch(arch, nullptr, who);
  if (rc) return rc;
  const auv_policy_arch_t a = *arch;
  rc = check_slices(h, n_slices, bounds, streams, who);
  if (rc) return rc;
  if (!ios || n_steps < 0 || !obs_dev || !reward_dev || !done_dev) return fail(AUV_EINVAL, "%s: bad arguments", who);
  const int D = auv_obs_cols(h->d.cfg, h->d.pool_ns);
  auv_population_io_t io[AUV_MAX_CHAINS];                // the slices' own rows of ios[i]
  for (int i = 0; i < n_slices; i++) {
    rc = check_population_io(a, ios + i, who);
    if (rc) return rc;
    const auv_population_io_t& s = ios[i];
    if (s.obs_dim != D) return fail(AUV_EINVAL, "%s: obs_dim %d, the handle's observation has %d columns", who, s.obs_dim, D);
    if (s.M != h->d.n) return fail(AUV_EINVAL, "%s: ios[%d].M = %d, the handle has %d environments (whole-batch rows)", who, i, s.M, h->d.n);
    if (bounds[i] % s.G || (bounds[i + 1] % s.G && bounds[i + 1] != h->d.n))
      return fail(AUV_EINVAL, "%s: slice [%d, %d) does not start and end on a multiple of G = %d", who, bounds[i], bounds[i + 1], s.G);
    if (!s.fit || !s.ends) return fail(AUV_EINVAL, "%s: null fit or ends", who);
    rc = check_actions(s.action, AUV_F32, who);
    if (rc) return rc;
    if (s.action_ld != 2) return fail(AUV_EINVAL, "%s: action_ld %d (the environment reads an [N][2] buffer)", who, s.action_ld);
    const size_t lo = (size_t)bounds[i];
    io[i] = s;
    io[i].members = s.members + (lo / (size_t)s.G) * (size_t)s.stride;
    io[i].X = obs_dev + lo * (size_t)D, io[i].ldx = D;
    io[i].mu = s.mu ? s.mu + 2 * lo : nullptr;
    io[i].action = s.action + 2 * lo;
    io[i].reward_in = reward_dev + lo, io[i].done_in = done_dev + lo;
    io[i].fit = s.fit + lo, io[i].ends = s.ends + lo;
    io[i].M = bounds[i + 1] - bounds[i];
  }
  PAIR_CHECK(h, obs_dev);
  HIP_TRY(auv_population_prepare(a, D));
  return rollout_loop(
      h, n_slices, bounds, streams, obs_dev, reward_dev, done_dev, n_steps, flush, [&](int i) { return ios[i].action; },
      [&](int i, int32_t k, bool flushing) {
        // (the first launch of a call has no completed step of this window behind it; the flush launch only books the last one)
        io[i].accumulate = flushing || k > 0, io[i].act = !flushing;
        auv_launch_population_act(a, io[i], (hipStream_t)streams[i]);
      });
}
int auv_population_rollout(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const auv_population_io_t* ios,
                           float* obs_dev, float* reward_dev, uint8_t* done_dev, int32_t n_steps, int32_t flush) {
  return population_rollout_impl(h, n_slices, bounds, streams, ios, &POLICY_ARCH_REF, obs_dev, reward_dev, done_dev, n_steps, flush,
                                 "auv_population_rollout");
}
int auv_population_rollout_arch(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const auv_population_io_t* ios,
                                const auv_policy_arch_t* arch, float* obs_dev, float* reward_dev, uint8_t* done_dev, int32_t n_steps,
                                int32_t flush) {
  return population_rollout_impl(h, n_slices, bounds, streams, ios, arch, obs_dev, reward_dev, done_dev, n_steps, flush,
                                 "auv_population_rollout_arch");
}

static int check_population_block(const auv_policy_arch_t& a, int32_t obs_dim, int32_t P, float sigma, const char* who) {
  int rc = check_population_obs_dim(a, obs_dim, who);
  if (rc) return rc;
  if (P < 1 || P > 65535) return fail(AUV_EINVAL, "%s: P = %d members outside [1, 65535]", who, P);
  if (!(sigma == sigma) || sigma - sigma != 0.0f) return fail(AUV_EINVAL, "%s: sigma must be finite", who);
  return AUV_OK;
}

static int population_perturb_impl(int32_t device, const float* theta, float* members, int64_t stride, int32_t P, int32_t obs_dim, float sigma,
                                   uint64_t seed, int64_t generation, const auv_policy_arch_t* arch, void* stream, const char* who) {
  if (device < 0) return fail(AUV_EINVAL, "%s: device %d", who, device);
  int rc = check_policy_arch(arch, nullptr, who);
  if (rc) return rc;
  const auv_policy_arch_t a = *arch;
  rc = check_population_block(a, obs_dim, P, sigma, who);
  if (rc) return rc;
  if (!theta || !members || ((uintptr_t)theta & 15) || ((uintptr_t)members & 15))
    return fail(AUV_EINVAL, "%s: theta and members must be 16-byte aligned device pointers", who);
  if (stride < (int64_t)auv_population_member_floats_impl(a, obs_dim) || (stride & 3) || stride > 0x7fffffff)
    return fail(AUV_EINVAL, "%s: stride %lld must be a multiple of 4, >= auv_population_member_floats(%d) = %zu and < 2^31", who,
                (long long)stride, obs_dim, auv_population_member_floats_impl(a, obs_dim));
  HIP_TRY(hipSetDevice(device));
  auv_launch_population_perturb(a, theta, members, (long long)stride, P, obs_dim, sigma, seed, (unsigned long long)generation, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}
int auv_population_perturb(int32_t device, const float* theta, float* members, int64_t stride, int32_t P, int32_t obs_dim, float sigma,
                           uint64_t seed, int64_t generation, void* stream) {
  return population_perturb_impl(device, theta, members, stride, P, obs_dim, sigma, seed, generation, &POLICY_ARCH_REF, stream,
                                 "auv_population_perturb");
}
int auv_population_perturb_arch(int32_t device, const float* theta, float* members, int64_t stride, int32_t P, int32_t obs_dim, float sigma,
                                uint64_t seed, int64_t generation, const auv_policy_arch_t* arch, void* stream) {
  return population_perturb_impl(device, theta, members, stride, P, obs_dim, sigma, seed, generation, arch, stream,
                                 "auv_population_perturb_arch");
}

static int population_update_impl(int32_t device, float* theta, const float* w, float* grad, int32_t P, int32_t obs_dim, float sigma, float lr,
                                  uint64_t seed, int64_t generation, const auv_policy_arch_t* arch, void* stream, const char* who) {
  if (device < 0) return fail(AUV_EINVAL, "%s: device %d", who, device);
  int rc = check_policy_arch(arch, nullptr, who);
  if (rc) return rc;
  const auv_policy_arch_t a = *arch;
  rc = check_population_block(a, obs_dim, P, sigma, who);
  if (rc) return rc;
  if (P < 2 || (P & 1)) return fail(AUV_EINVAL, "%s: P = %d must be even (mirrored pairs)", who, P);
  if (!(sigma > 0.0f)) return fail(AUV_EINVAL, "%s: sigma must be > 0", who);
  if (!(lr == lr) || lr - lr != 0.0f) return fail(AUV_EINVAL, "%s: lr must be finite", who);
  if (!w || !grad || ((uintptr_t)w & 3) || ((uintptr_t)grad & 15) || ((uintptr_t)theta & 15))
    return fail(AUV_EINVAL, "%s: w must be 4-byte, grad and theta 16-byte aligned device pointers", who);
  if (lr != 0.0f && !theta) return fail(AUV_EINVAL, "%s: lr != 0 needs theta", who);
  HIP_TRY(hipSetDevice(device));
  auv_launch_population_update(a, theta, w, grad, P, obs_dim, sigma, lr, seed, (unsigned long long)generation, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}
int auv_population_update(int32_t device, float* theta, const float* w, float* grad, int32_t P, int32_t obs_dim, float sigma, float lr,
                          uint64_t seed, int64_t generation, void* stream) {
  return population_update_impl(device, theta, w, grad, P, obs_dim, sigma, lr, seed, generation, &POLICY_ARCH_REF, stream,
                                "auv_population_update");
}
int auv_population_update_arch(int32_t device, float* theta, const float* w, float* grad, int32_t P, int32_t obs_dim, float sigma, float lr,
                               uint64_t seed, int64_t generation, const auv_policy_arch_t* arch, void* stream) {
  return population_update_impl(device, theta, w, grad, P, obs_dim, sigma, lr, seed, generation, arch, stream, "auv_population_update_arch");
}

// ---- the PPO update (include/auv_hip.h, auv_ppo_*; kernels: k8_ppo_update.hip, k13_ppo_update_arch.hip) ----
struct auv_ppo {
  AuvPpoDev d;
  auv_policy_arch_t arch;          // the hidden widths, a triple of POL_ARCH_LIST: every launch dispatches on them
  int device;
  float* arena;
};

size_t auv_ppo_param_floats(int32_t obs_dim) { return auv_ppo_param_floats_arch(obs_dim, &POLICY_ARCH_REF); }

size_t auv_ppo_param_floats_arch(int32_t obs_dim, const auv_policy_arch_t* arch) {
  if (obs_dim <= 0 || !arch || !pol_arch_listed(arch->h1, arch->h2, arch->h3)) return 0;
  return auv_ppo_param_floats_impl(obs_dim, *arch);
}

int auv_ppo_create(int32_t device, int32_t obs_dim, int32_t max_batch, auv_ppo_t** out) {
  return auv_ppo_create_arch(device, obs_dim, max_batch, &POLICY_ARCH_REF, out);
}

int auv_ppo_create_arch(int32_t device, int32_t obs_dim, int32_t max_batch, const auv_policy_arch_t* arch, auv_ppo_t** out) {
  if (!out) return fail(AUV_EINVAL, "auv_ppo_create: null out");
  *out = nullptr;
  int rca = check_policy_arch(arch, nullptr, "auv_ppo_create");
  if (rca != AUV_OK) return rca;
  const auv_policy_arch_t a = *arch;
  if (obs_dim < 1) return fail(AUV_EINVAL, "auv_ppo_create: obs_dim %d < 1", obs_dim);
  if (obs_dim > 16384 || auv_ppo_lds_bytes(obs_dim, a) > 160 * 1024)
    return fail(AUV_EINVAL, "auv_ppo_create: obs_dim %d is too wide for the row pass' LDS tile", obs_dim);
  if (max_batch < 1 || max_batch > (1 << 24)) return fail(AUV_EINVAL, "auv_ppo_create: max_batch %d outside [1, 2^24]", max_batch);
  if (device < 0) return fail(AUV_EINVAL, "auv_ppo_create: device %d", device);
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device >= ndev) return fail(AUV_EINVAL, "auv_ppo_create: device %d not present (%d visible)", device, ndev);
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(auv_ppo_prepare(obs_dim, a));
  auv_ppo* p = new auv_ppo();
  p->device = device, p->arch = a;
  AuvPpoDev& d = p->d;
  d.obs_dim = obs_dim, d.k0p = (obs_dim + 31) & ~31, d.max_batch = max_batch, d.rt_max = (max_batch + 15) / 16;
  const size_t rows = (size_t)d.rt_max * 16, fwd = auv_ppo_fwd_floats(obs_dim, a), tr = auv_ppo_tr_floats(a);
  // one allocation, carved into parts of a multiple of four floats each (16-byte aligned)
  const size_t n_part = (size_t)AUV_PPO_MAX_SPLIT * (fwd - 4);
  size_t total = fwd + tr + 256 + rows * d.k0p + 2 * rows * (2 * (size_t)(a.h1 + a.h2 + a.h3) + 16) + n_part + (size_t)d.rt_max * 12 + 4 * AUV_PPO_NORM_BLOCKS;
  hipError_t e = hipMalloc((void**)&p->arena, total * sizeof(float));
  if (e != hipSuccess) {
    delete p;
    return fail(AUV_ENOMEM, "auv_ppo_create: %zu bytes of scratch for batches of %d rows: %s", total * sizeof(float), max_batch, hipGetErrorString(e));
  }
  float* q = p->arena;
  auto take = [&q](size_t n) { float* r = q; q += n; return r; };
  d.fwd = take(fwd), d.tr = take(tr), d.zero = take(256);
  d.sqpart = (double*)take(4 * AUV_PPO_NORM_BLOCKS);
  d.X = take(rows * d.k0p);
  for (int net = 0; net < 2; net++) {
    d.Y[net][0] = take(rows * a.h1), d.Y[net][1] = take(rows * a.h2), d.Y[net][2] = take(rows * a.h3);
    d.dZ[net][0] = take(rows * a.h1), d.dZ[net][1] = take(rows * a.h2), d.dZ[net][2] = take(rows * a.h3), d.dZ[net][3] = take(rows * 16);
  }
  d.part = take(n_part), d.tstat = take((size_t)d.rt_max * 12);   // ([rt_max][8], then the squash head's [rt_max]; 12: a multiple of four)
  d.pol = nullptr;
  e = hipMemset(p->arena, 0, total * sizeof(float));
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    (void)hipFree(p->arena);
    delete p;
    return fail(AUV_EHIP, "auv_ppo_create: %s", hipGetErrorString(e));
  }
  *out = p;
  return AUV_OK;
}

void auv_ppo_destroy(auv_ppo_t* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  (void)hipDeviceSynchronize();
  (void)hipFree(p->arena);
  delete p;
}

int auv_ppo_load(auv_ppo_t* p, const float* theta, void* stream) {
  if (!p || !theta) return fail(AUV_EINVAL, "auv_ppo_load: null %s", !p ? "updater" : "theta");
  HIP_TRY(hipSetDevice(p->device));
  auv_launch_ppo_load(p->d, p->arch, theta, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

int auv_ppo_attach_policy(auv_ppo_t* p, float* policy_params) {
  if (!p) return fail(AUV_EINVAL, "auv_ppo_attach_policy: null updater");
  if ((uintptr_t)policy_params & 15) return fail(AUV_EINVAL, "auv_ppo_attach_policy: policy_params must be 16-byte aligned");
  p->d.pol = policy_params;
  return AUV_OK;
}

int auv_ppo_grad(auv_ppo_t* p, const auv_ppo_batch_t* b, float* grad, float* stats, void* stream) {
  if (!p || !b || !grad || !stats) return fail(AUV_EINVAL, "auv_ppo_grad: null argument");
  if (!b->O || !b->A || !b->LP || !b->ADV || !b->RET) return fail(AUV_EINVAL, "auv_ppo_grad: null batch buffer");
  if (b->B < 1 || b->B > p->d.max_batch) return fail(AUV_EINVAL, "auv_ppo_grad: B = %d outside [1, max_batch = %d]", b->B, p->d.max_batch);
  if (b->n_rows < 1 || (!b->idx && b->B > b->n_rows)) return fail(AUV_EINVAL, "auv_ppo_grad: B = %d rows of n_rows = %d", b->B, b->n_rows);
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(auv_ppo_prepare(p->d.obs_dim, p->arch));
  auv_launch_ppo_grad(p->d, p->arch, *b, grad, stats, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

int auv_ppo_grad_clone(auv_ppo_t* p, const auv_ppo_clone_batch_t* b, float* grad, float* stats, void* stream) {
  if (!p || !b || !grad || !stats) return fail(AUV_EINVAL, "auv_ppo_grad_clone: null argument");
  if (!b->O || !b->A || !b->RET) return fail(AUV_EINVAL, "auv_ppo_grad_clone: null batch buffer (O, A and RET are required)");
  if (b->kind != 0 && b->kind != 1) return fail(AUV_EINVAL, "auv_ppo_grad_clone: kind = %d (0: Gaussian NLL, 1: MSE on the mean)", b->kind);
  if (b->B < 1) return fail(AUV_EINVAL, "auv_ppo_grad_clone: B = %d < 1", b->B);
  if (b->n_rows < 1 || (!b->idx && b->B > b->n_rows)) return fail(AUV_EINVAL, "auv_ppo_grad_clone: B = %d rows of n_rows = %d", b->B, b->n_rows);
  if (b->B > p->d.max_batch) return fail(AUV_EINVAL, "auv_ppo_grad_clone: B = %d above max_batch = %d", b->B, p->d.max_batch);
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(auv_ppo_prepare(p->d.obs_dim, p->arch, AUV_PPO_HEAD_CLONE));
  auv_launch_ppo_grad_clone(p->d, p->arch, *b, grad, stats, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

int auv_ppo_grad_squash(auv_ppo_t* p, const auv_ppo_squash_batch_t* b, float* grad, float* stats, void* stream) {
  if (!p || !b || !grad || !stats) return fail(AUV_EINVAL, "auv_ppo_grad_squash: null argument");
  if (!b->O || !b->A || !b->LP || !b->ADV || !b->RET) return fail(AUV_EINVAL, "auv_ppo_grad_squash: null batch buffer");
  if (b->B < 1 || b->B > p->d.max_batch) return fail(AUV_EINVAL, "auv_ppo_grad_squash: B = %d outside [1, max_batch = %d]", b->B, p->d.max_batch);
  if (b->n_rows < 1 || (!b->idx && b->B > b->n_rows)) return fail(AUV_EINVAL, "auv_ppo_grad_squash: B = %d rows of n_rows = %d", b->B, b->n_rows);
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(auv_ppo_prepare(p->d.obs_dim, p->arch, AUV_PPO_HEAD_SQUASH));
  auv_launch_ppo_grad_squash(p->d, p->arch, *b, grad, stats, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

int auv_ppo_adam(auv_ppo_t* p, float* theta, float* m, float* v, const float* grad, const auv_ppo_adam_t* a, float* norms_out, void* stream) {
  if (!p || !theta || !m || !v || !grad || !a || !norms_out) return fail(AUV_EINVAL, "auv_ppo_adam: null argument");
  if (!(a->bc1 > 0.0) || !(a->bc2 > 0.0)) return fail(AUV_EINVAL, "auv_ppo_adam: bias corrections must be > 0 (step >= 1)");
  AuvPpoAdamDev h;
  h.w1 = (float)(1.0 - a->beta1), h.b2 = (float)a->beta2, h.w2 = (float)(1.0 - a->beta2);
  h.step_size = (float)(a->lr / a->bc1), h.bc2_sqrt = (float)std::sqrt(a->bc2), h.eps = (float)a->eps;
  h.max_norm_pi = a->max_norm_pi, h.max_norm_v = a->max_norm_v;
  HIP_TRY(hipSetDevice(p->device));
  auv_launch_ppo_adam(p->d, p->arch, theta, m, v, grad, h, norms_out, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return AUV_OK;
}

}  // extern "C"
