// auv_launch.h — the host-side launchers the kernel files define (k1 .. k7, k9 .. k12, k14 .. k17, k_step_fused.hip) and the C ABI's host
// files (auv_capi*.hip) call: declared once, here, with their default arguments.  Definer and caller both include this header, so
// a definition that drifts from what its caller believes is a compile error.  The launchers of the PPO update, the world
// generator, the renderer and the k11 population pass are declared beside their argument structs (auv_ppo.h, auv_generate.h,
// auv_render.h, auv_population_pass.h).
#ifndef AUV_LAUNCH_H
#define AUV_LAUNCH_H
#include "auv_device.h"
#include "auv_snapshot.h"

void auv_launch_k1(const AuvDev& d, const void* actions, int dtype, hipStream_t st, hipEvent_t ev0 = nullptr,
                   hipEvent_t ev1 = nullptr);
void auv_launch_k2(const AuvDev& d, int advance_movers, hipStream_t st);
void auv_launch_k2_fresh(const AuvDev& d, hipStream_t st);
void auv_launch_k3(const AuvDev& d, int mode, float* obs, float* reward, uint8_t* done, hipStream_t st);
void auv_launch_k3_fresh(const AuvDev& d, float* obs, hipStream_t st);
void auv_launch_k3_nav(const AuvDev& d, float* obs, hipStream_t st);
void auv_launch_k3_reward(const AuvDev& d, float* obs, float* reward, uint8_t* done, int lidar_obs, hipStream_t st,
                          hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
void auv_launch_reset(const AuvDev& d, const uint8_t* mask, const int32_t* world_idx, float* obs, hipStream_t st);
void auv_launch_harvest(const AuvDev& d, int count, hipStream_t st, const int32_t* count_dev = nullptr);
void auv_launch_fw_shadow_reset(const AuvDev& d, const int32_t* count_dev, hipStream_t st);
void auv_launch_refresh_desc(const AuvDev& d, hipStream_t st);
void auv_launch_derive(const AuvDev& d, hipStream_t st);
void auv_launch_ring_advance(const AuvDev& d, hipStream_t st);   // (no caller at present: the ring is advanced inside the step's launches)
size_t auv_k2_lds_bytes(const AuvDev& d);
hipError_t auv_k2_prepare(const AuvDev& d);
bool auv_k23_ok(const AuvDev& d);
void auv_launch_k23(const AuvDev& d, float* obs, hipStream_t st, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
hipError_t auv_step_fused_prepare(const AuvDev& d);
uint32_t auv_step_lds_bytes(const AuvDev& d);
int auv_pick_seg_cap(const AuvDev& d);
bool auv_roles_ok(const AuvDev& d);
void auv_launch_step_roles(const AuvDev& d, const void* actions, int dtype, float* obs, float* reward, uint8_t* done,
                           hipStream_t st, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
void auv_launch_k31(const AuvDev& d, const void* actions, int dtype, float* obs, float* reward, uint8_t* done, hipStream_t st);
void auv_launch_step_multi(const AuvDev& d, const void* actions, int dtype, float* obs, float* reward, uint8_t* done, int n_steps, int first_slot,
                           int n_slots, unsigned long long seq0, int order, int lead, int lag, hipStream_t st, unsigned int fw_call = 0u);
void auv_launch_step_record(const AuvDev& d, const void* actions, int dtype, float* obs, float* reward, uint8_t* done, float* obs_rec, float* reward_rec,
                            uint8_t* done_rec, int n_steps, int first_slot, int n_slots, unsigned long long seq0, int order, int lead, int lag, hipStream_t st,
                            unsigned int fw_call = 0u);
void auv_launch_step_feedback(const AuvDev& d, const double* gains, const void* actions, int dtype, float* obs, float* reward, uint8_t* done, float* obs_rec,
                              float* reward_rec, uint8_t* done_rec, double* act_rec, int n_steps, int first_slot, int n_slots, unsigned long long seq0,
                              int order, int lead, int lag, hipStream_t st, const double* sector_gains, const int32_t* sector_bounds,
                              const double* hidden, int activation, unsigned int fw_call = 0u);
void auv_launch_spin(unsigned long long ticks, hipStream_t st);
void auv_launch_rdv_publish(unsigned long long* word, unsigned long long seq, hipStream_t st);
void auv_launch_rdv_arrive(unsigned long long* word, hipStream_t st);
void auv_launch_rdv_wait(const unsigned long long* word, unsigned long long target, int32_t* err, int code, double limit_s, int32_t* abort_flag,
                         int32_t* report, hipStream_t st);
hipError_t auv_launch_probe(unsigned int* words, int np, int nc, unsigned int tag, unsigned int* failures, uint32_t lds, hipStream_t st);
// the forward launches (k6_policy.hip, k9_policy_eval.hip, k12_policy_stacked.hip) take a hidden-width triple of the closed list
// (auv_policy_mfma.h, POL_ARCH_LIST)
size_t auv_policy_param_floats_impl(int h1, int h2, int h3, int obs_dim);
size_t auv_policy_lds_bytes(int h1, int h2, int h3, int obs_dim);
hipError_t auv_policy_prepare(int h1, int h2, int h3, int obs_dim);
void auv_launch_policy(int h1, int h2, int h3, const auv_policy_io_t& io, int e0, int ne, hipStream_t st, long long t_host = -1,
                       long long gstep_host = -1);
void auv_launch_gae(const float* R, const float* V, const float* Dn, const float* last_v, float gamma, float lam, float* adv, float* ret,
                    int T, int N, hipStream_t st);
void auv_launch_k4(const AuvDev& d, const int32_t* sector_start, int n_sectors, double width, double* out_dist,
                   float* out_closeness, hipStream_t st);
void auv_launch_snapshot(const AuvSnapArgs& a, const int32_t* env_idx, int m, void* rows, hipStream_t st);
void auv_launch_restore(const AuvSnapArgs& a, const AuvDev& d, const void* rows, int n_rows, const int32_t* row_idx, const int32_t* env_idx, int m,
                        float* obs, hipStream_t st);
void auv_launch_plan_score(const float* reward, const uint8_t* done, int T, int n, int group, float gamma, float* score, int32_t* best, hipStream_t st);
hipError_t auv_policy_eval_prepare(int h1, int h2, int h3, int obs_dim);
void auv_launch_policy_eval(int h1, int h2, int h3, const auv_policy_eval_t& ev, bool want_pi, bool want_v, hipStream_t st);
void auv_launch_plan_score_v(const float* reward, const uint8_t* done, const float* terminal, int T, int n, int group, float gamma, float* score,
                             int32_t* best, hipStream_t st);
// k15_plan.hip: the planner's sampler and refit (contracts: include/auv_hip.h, auv_plan_sample / auv_plan_refit).  The host side has
// checked every size (group <= AUV_PLAN_MAX_GROUP, T * n * 2 < 2^31) and every pointer the method reads or writes.
struct AuvPlanSample {
  const float *mean, *sigma;         // [T][B][2]
  const float *mean0, *sigma0;       // [T][B][2]: what a group with reset[b] != 0 reads (with `reset` only)
  const uint8_t* reset;              // [B] or NULL
  float* ring;                       // [T][n][2]
  int32_t T, n, group, shift;
  float lo[2], hi[2];
  unsigned long long seed, draw;
};
struct AuvPlanRefit {
  const float *ring, *score;         // [T][n][2], [n]
  const int32_t* best;               // [B]
  const float *mean_in, *sigma_in;   // [T][B][2] (MPPI)
  float *mean_out, *sigma_out;       // [T][B][2], both or neither
  float *chosen, *predicted;         // [T][B][2], [B]; each nullable
  int32_t T, n, group, method, n_elite;
  float sigma_min, lambda;
};
void auv_launch_plan_sample(const AuvPlanSample& a, hipStream_t st);
void auv_launch_plan_refit(const AuvPlanRefit& a, hipStream_t st);
// k14_population_arch.hip: the population launches at the widths `a` (a listed triple; the reference's lands on k11_population.hip)
size_t auv_population_member_floats_impl(const auv_policy_arch_t& a, int obs_dim);
hipError_t auv_population_prepare(const auv_policy_arch_t& a, int obs_dim);
void auv_launch_population_act(const auv_policy_arch_t& a, const auv_population_io_t& io, hipStream_t st);
// k12_policy_stacked.hip
size_t auv_policy_stacked_lds_bytes(int h1, int h2, int h3, int width);
hipError_t auv_policy_stacked_prepare(int h1, int h2, int h3, int width);
void auv_launch_policy_stacked(int h1, int h2, int h3, const auv_policy_stack_t& s, int e0, int ne, hipStream_t st, long long t_host = -1,
                               long long gstep_host = -1);
void auv_launch_stack_frames(const float* obs, const uint8_t* done, float* hist, int32_t* stk, float* out, long long ldx, int e0, int ne,
                             int obs_dim, int frames, int advance, hipStream_t st);
// k16_policy_norm.hip: the normalising act launch (LDS: auv_policy_lds_bytes), the same expression on arbitrary rows, the fold of the
// observation partials and the return pass (contracts: include/auv_hip.h, auv_policy_norm).  The host side has checked every pointer.
hipError_t auv_policy_norm_prepare(int h1, int h2, int h3, int obs_dim);
void auv_launch_policy_norm(int h1, int h2, int h3, const auv_policy_norm_t& s, int e0, int ne, hipStream_t st, long long t_host = -1,
                            long long gstep_host = -1);
void auv_launch_norm_rows(const float* X, const int64_t* idx, long long ldx, const float* table, float clip_obs, float* out, long long ldo,
                          int M, int obs_dim, hipStream_t st);
void auv_launch_norm_fold(const float* part, const int32_t* pcnt, int n_slots, int obs_dim, double eps, double* mom, float* table,
                          hipStream_t st);
void auv_launch_norm_returns(const float* R, const float* Dn, float* out, int T, int N, double gamma, float clip_reward, double eps, double* ret,
                             double* rpart, double* rmom, bool update, hipStream_t st);
// k17_policy_squash.hip: the act and the eval launch of a tanh-squashed policy (exact f32, LDS: auv_policy_lds_bytes); `eval` names
// the kernel auv_policy_squash_prepare sets up
hipError_t auv_policy_squash_prepare(int h1, int h2, int h3, int obs_dim, bool eval);
void auv_launch_policy_squash(int h1, int h2, int h3, const auv_policy_io_t& io, int e0, int ne, hipStream_t st, long long t_host = -1,
                              long long gstep_host = -1);
void auv_launch_policy_eval_squash(int h1, int h2, int h3, const auv_policy_eval_t& ev, bool want_pi, bool want_v, hipStream_t st);
void auv_launch_population_perturb(const auv_policy_arch_t& a, const float* theta, float* members, long long stride, int P, int obs_dim,
                                   float sigma, unsigned long long seed, unsigned long long generation, hipStream_t st);
void auv_launch_population_update(const auv_policy_arch_t& a, float* theta, const float* w, float* grad, int P, int obs_dim, float sigma,
                                  float lr, unsigned long long seed, unsigned long long generation, hipStream_t st);

#endif  // AUV_LAUNCH_H
