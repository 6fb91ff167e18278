// The PPO update object behind auv_ppo_* (include/auv_hip.h): what auv_capi_learn.hip allocates and k8_ppo_update.hip launches on.
#ifndef AUV_PPO_H
#define AUV_PPO_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/auv_hip.h"

#define AUV_PPO_MAX_SPLIT 16       // split-K factor of the weight-gradient pass (workgroups per output unit), at most
#define AUV_PPO_NORM_BLOCKS 64     // partial sums of squares per gradient-norm launch
// the heads of the row pass (auv_ppo_pass.h, ppo_head): which kernel a launch or auv_ppo_prepare means
#define AUV_PPO_HEAD_PPO 0
#define AUV_PPO_HEAD_CLONE 1
#define AUV_PPO_HEAD_SQUASH 2

// Device memory of one updater of hidden widths (H1, H2, H3), a triple of POL_ARCH_LIST (auv_policy_mfma.h); the widths themselves are
// not stored here: the kernels take them as a template parameter, the host keeps them beside this struct.  Every matrix of the row pass' scratch is stored in 16 x 16 blocks [row tile][column tile][256]:
// element (r, c) of a block at ((r / 4) * 16 + c) * 4 + r % 4 -- the float4 a lane of the weight-gradient pass loads, and the
// four registers a lane of an MFMA result holds.
struct AuvPpoDev {
  int32_t obs_dim, k0p, max_batch, rt_max;
  float* fwd;          // forward copy: the layout of auv_policy_io::params (two nets, log_std[2], two floats of padding)
  float* tr;           // transposed copy, per net: W2^T [H1][H2] | W3^T [H2][H3] | W4^T [H3][32], fragment order
  float* zero;         // [256] zeros: the "bias" of a backward layer (256: the widest listed layer)
  float* X;            // [rt][k0p / 16][256]   the gathered, zero-padded observations (written by the policy net's workgroups)
  float* Y[2][3];      // per net: Y1 [rt][H1 / 16][256], Y2 [rt][H2 / 16][256], Y3 [rt][H3 / 16][256]
  float* dZ[2][4];     // per net: dZ1 [rt][H1 / 16][256], dZ2 [rt][H2 / 16][256], dZ3 [rt][H3 / 16][256], dZ4 [rt][1][256]
  float* part;         // [AUV_PPO_MAX_SPLIT][2][net floats]: split-K partials of dW (row-major, padded like the forward copy) and db
  float* tstat;        // [rt][8]: per row tile sum pg, sum vf, max |adv|, max ratio, non-finite inputs, clipped rows, d log_std[2]
                       // (k8_clone: sum bc, sum vf, max |a - mu|, sum w, non-finite inputs, 0, d log_std[2])
                       // and behind them [rt_max]: the squash head's sum of log(1 - tanh^2 a) per row tile (its reduction alone reads it)
  double* sqpart;      // [AUV_PPO_NORM_BLOCKS][2]: partial sums of squares of the policy and the value group
  float* pol;          // attached auv_policy_io::params buffer (nullable)
};

struct AuvPpoAdamDev {
  float w1, b2, w2;    // 1 - beta1, beta2, 1 - beta2: each rounded once from double
  float step_size, bc2_sqrt, eps, max_norm_pi, max_norm_v;
};

// k13_ppo_update_arch.hip: sizes and launches for the widths `a`, which must be listed (pol_arch_listed: the C entries check it).
// (256, 128, 64) goes to the kernels of k8_ppo_update.hip, every other triple to its own instantiations.
size_t auv_ppo_param_floats_impl(int obs_dim, const auv_policy_arch_t& a);
size_t auv_ppo_fwd_floats(int obs_dim, const auv_policy_arch_t& a);
size_t auv_ppo_tr_floats(const auv_policy_arch_t& a);
size_t auv_ppo_lds_bytes(int obs_dim, const auv_policy_arch_t& a);
hipError_t auv_ppo_prepare(int obs_dim, const auv_policy_arch_t& a, int head = AUV_PPO_HEAD_PPO);    // head: whose row pass (AUV_PPO_HEAD_*)
void auv_launch_ppo_load(const AuvPpoDev& d, const auv_policy_arch_t& a, const float* theta, hipStream_t st);
void auv_launch_ppo_grad(const AuvPpoDev& d, const auv_policy_arch_t& a, const auv_ppo_batch_t& b, float* grad, float* stats, hipStream_t st);
void auv_launch_ppo_grad_clone(const AuvPpoDev& d, const auv_policy_arch_t& a, const auv_ppo_clone_batch_t& b, float* grad, float* stats,
                               hipStream_t st);
void auv_launch_ppo_grad_squash(const AuvPpoDev& d, const auv_policy_arch_t& a, const auv_ppo_squash_batch_t& b, float* grad, float* stats,
                                hipStream_t st);
void auv_launch_ppo_adam(const AuvPpoDev& d, const auv_policy_arch_t& a, float* theta, float* m, float* v, const float* grad,
                         const AuvPpoAdamDev& h, float* norms_out, hipStream_t st);
// k8_ppo_update.hip: the same at the reference's widths
hipError_t auv_k8_ppo_prepare(int obs_dim, int head);
void auv_k8_ppo_load(const AuvPpoDev& d, const float* theta, hipStream_t st);
void auv_k8_ppo_grad(const AuvPpoDev& d, const auv_ppo_batch_t& b, float* grad, float* stats, hipStream_t st);
void auv_k8_ppo_grad_clone(const AuvPpoDev& d, const auv_ppo_clone_batch_t& b, float* grad, float* stats, hipStream_t st);
void auv_k8_ppo_grad_squash(const AuvPpoDev& d, const auv_ppo_squash_batch_t& b, float* grad, float* stats, hipStream_t st);
void auv_k8_ppo_adam(const AuvPpoDev& d, float* theta, float* m, float* v, const float* grad, const AuvPpoAdamDev& h, float* norms_out,
                     hipStream_t st);
#endif /* AUV_PPO_H */
