// K8 -- the PPO minibatch update of examples/ppo.py (minibatch_step) as a few launches: forward and backward of both nets on
// the matrix cores, the clipped-surrogate / value / entropy loss, the two global-norm clips and Adam (include/auv_hip.h, auv_ppo_*).
//
// Reference: scripts/run.py:332-357 -- PPO2(MlpPolicy, net_arch [256, 128, 64] for policy and value function, tanh), a diagonal
// Gaussian over the two actions with a free log_std[2].  The loss and its gradient (derived by hand from minibatch_step):
//   ratio = exp(logp(mu, a) - lp_old);  pg = -mean(min(ratio adv, clamp(ratio, 1 - c, 1 + c) adv));  vf = 0.5 mean((v - ret)^2)
//   loss = pg + vf_coef vf - ent_coef sum_k (0.5 + log sqrt(2 pi) + log_std_k)
//   d pg / d logp_i = -adv_i ratio_i / B, or 0 where the clipped branch is the active minimum (adv > 0 and ratio > 1 + c, or
//   adv < 0 and ratio < 1 - c);  d logp / d mu_k = (a_k - mu_k) / sigma_k^2;  d logp / d log_std_k = z_k^2 - 1;
//   d loss / d v_i = vf_coef (v_i - ret_i) / B;  the entropy adds -ent_coef to each log_std gradient.
//
// Launches of auv_ppo_grad:
//   k8_rows    one workgroup = 16 rows of one net (as k6_policy_act): gathers its rows through idx, runs the forward pass with all
//              activations kept in LDS, forms the head gradient and dZ_l = (dZ_{l+1} W_{l+1}) * (1 - Y_l^2) with W_{l+1} read through
//              the transposed fragment-order copy, and writes Y_{l-1} / dZ_l in 16 x 16 blocks plus per-tile partial statistics.
//   k8_wgrad   dW_l = dZ_l^T Y_{l-1}, db_l = column sums of dZ_l: split-K over the batch, one workgroup = up to four 16 x 16
//              output tiles of one row of tiles, four waves on four row ranges, summed in a fixed order.
//   k8_reduce  sums the split partials in a fixed order into the flat gradient (torch layout), and the tile statistics.
// auv_ppo_grad_clone: the same three with k8_clone in place of k8_rows -- the same row pass with a supervised head (ppo_head).
// auv_ppo_grad_squash: the same three with k8_squash -- PPO's head with the entropy of the tanh-squashed distribution, estimated on the
// stored actions (ppo_head_pg<SQUASH>), and the reduction that also reads its ninth per-tile sum (k8_reduce<A, true>).
// Launches of auv_ppo_adam: k8_norm (partial sums of squares per group), k8_adam (clip, Adam, and the scatter of every updated
// weight into the forward copy, the transposed copy and an attached auv_policy_io::params buffer).
// No floating-point atomics anywhere: every sum crosses workgroups through memory and a kernel boundary, in an order that depends
// on B alone.  No kernel waits for another workgroup.
//
// The bodies are templates on the hidden widths (auv_ppo_pass.h).  This file holds the kernels of the reference's widths [256, 128, 64];
// k13_ppo_update_arch.hip holds those of the other listed triples and the dispatch on an updater's widths.
#include "auv_ppo_pass.h"

namespace {

// grid (ceil(B / 16), 2): blockIdx.y = 0 the policy net, 1 the value net
__global__ void __launch_bounds__(POL_THREADS, 4) k8_rows(RowArgs<auv_ppo_batch_t> ra) { ppo_row_pass<PolArchRef>(ra.d, ra.b, blockIdx.y, blockIdx.x); }

// the same grid with the supervised head: the row pass of auv_ppo_grad_clone
__global__ void __launch_bounds__(POL_THREADS, 4) k8_clone(RowArgs<auv_ppo_clone_batch_t> ra) {
  ppo_row_pass<PolArchRef>(ra.d, ra.b, blockIdx.y, blockIdx.x);
}

// the same grid with the squashed distribution's entropy in PPO's head: the row pass of auv_ppo_grad_squash
__global__ void __launch_bounds__(POL_THREADS, 4) k8_squash(RowArgs<auv_ppo_squash_batch_t> ra) {
  ppo_row_pass<PolArchRef>(ra.d, ra.b, blockIdx.y, blockIdx.x);
}

struct K8 {
  static constexpr auto rows = k8_rows;
  static constexpr auto clone = k8_clone;
  static constexpr auto squash = k8_squash;
};

}  // namespace

hipError_t auv_k8_ppo_prepare(int obs_dim, int head) { return ppo_prepare<PolArchRef, K8>(obs_dim, head); }
void auv_k8_ppo_load(const AuvPpoDev& d, const float* theta, hipStream_t st) { ppo_launch_load<PolArchRef>(d, theta, st); }
void auv_k8_ppo_grad(const AuvPpoDev& d, const auv_ppo_batch_t& b, float* grad, float* stats, hipStream_t st) {
  ppo_launch_grad<PolArchRef, K8>(d, b, grad, stats, st);
}
void auv_k8_ppo_grad_clone(const AuvPpoDev& d, const auv_ppo_clone_batch_t& b, float* grad, float* stats, hipStream_t st) {
  ppo_launch_grad_clone<PolArchRef, K8>(d, b, grad, stats, st);
}
void auv_k8_ppo_grad_squash(const AuvPpoDev& d, const auv_ppo_squash_batch_t& b, float* grad, float* stats, hipStream_t st) {
  ppo_launch_grad_squash<PolArchRef, K8>(d, b, grad, stats, st);
}
void auv_k8_ppo_adam(const AuvPpoDev& d, float* theta, float* m, float* v, const float* grad, const AuvPpoAdamDev& h, float* norms_out,
                     hipStream_t st) {
  ppo_launch_adam<PolArchRef>(d, theta, m, v, grad, h, norms_out, st);
}
