// torch.optim.Adam's arithmetic for one element and the scalars of one step, each written once: adam_range_body (tn_misc.hip) walks optimiser
// ranges with them; the main grid's fold (tn_scatter.hip, k_seg_fold<true>) steps a bucket's slots with them while their gradient is still in LDS.
#pragma once
#include "tn_common.h"

struct AdamCoef {
  float neg_step, bc2_sqrt;  // -lr / (1 - beta1^t), sqrt(1 - beta2^t): adam_step_scalars
  float b1, b2, omb1, omb2, eps;
};
__host__ __device__ __forceinline__ AdamCoef adam_coef(float neg_step, float bc2_sqrt, double beta1, double beta2, float eps) {
  return AdamCoef{neg_step, bc2_sqrt, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps};
}
// g: the gradient as the step uses it (already unscaled)
__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, const AdamCoef& c) {
  const float m_new = m * c.b1 + g * c.omb1;
  const float v_new = v * c.b2 + (c.omb2 * g) * g;
  const float den = sqrtf(v_new) / c.bc2_sqrt + c.eps;
  p = p + c.neg_step * (m_new / den);
  m = m_new;
  v = v_new;
}
// The step's scalars in double: bias corrections at (host step count - steps the group skipped), the reference's ExponentialDecayScheduler
// (engine/schedulers.py:109-141) at (sched_step - lag) when max_steps > 0.  In pieces, so that a launch which computes them ONCE (one lane
// each: fold_adam_scalars_block, tn_scatter.hip) can evaluate the four transcendental terms on four waves side by side; adam_step_scalars is
// their composition.  The library is built with -ffp-contract=off (build.sh), and the pragma below pins it from here to the end of the
// including file whatever the build says: the sum of the two log terms is then the same two roundings whether its operands come from registers or through LDS.
#pragma clang fp contract(off)
__device__ __forceinline__ double adam_bias_correction(double beta, int step, int skipped) {
  const int eff = step - skipped;
  return 1.0 - pow(beta, (double)(eff < 1 ? 1 : eff));
}
__device__ __forceinline__ double adam_sched_t(int max_steps, int sched_step, int lag) {
  const double t = (double)(sched_step - lag) / (double)max_steps;
  return t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
}
__device__ __forceinline__ double adam_log_lr_term(double lr, double weight) { return log(lr) * weight; }  // lr = exp(term(lr_init, 1 - t) + term(lr_final, t))
__device__ __forceinline__ void adam_scalars_finish(double bc1, double bc2, double lr, float& neg_step, float& bc2_sqrt) {
  neg_step = (float)(-(lr / bc1));
  bc2_sqrt = (float)sqrt(bc2);
}
__device__ __forceinline__ void adam_step_scalars(int step, int skipped, double lr, double lr_final, int max_steps, int sched_step, int lag, double beta1,
                                                  double beta2, float& neg_step, float& bc2_sqrt) {
  const double bc1 = adam_bias_correction(beta1, step, skipped), bc2 = adam_bias_correction(beta2, step, skipped);
  if (max_steps > 0) {
    const double t = adam_sched_t(max_steps, sched_step, lag);
    lr = exp(adam_log_lr_term(lr, 1.0 - t) + adam_log_lr_term(lr_final, t));
  }
  adam_scalars_finish(bc1, bc2, lr, neg_step, bc2_sqrt);
}

// The main grid's fold stepping its own table (tn_train_step, TN_FOLD_ADAM): what the launches of one iteration share.
// state: 4 floats on the device, zero when the iteration starts (slots 12..15 of tn_train_step's losses16):
//   [0] max |d enc| over the batch's live samples (per wave by the bin pass, as an integer max of bit patterns: NaN > inf > every finite value;
//       reduced by the launch between bin and fold)
//   [1] the decision word, written by the launch between bin and fold and read by the fold and by the Adam launch
//   [2] neg_step, [3] bc2_sqrt of the table's range for this iteration (one extra block of the bin launch)
#define TN_FOLD_ADAM_STATE_SLOT 12
#define TN_FOLD_ADAM_NONE 0.0f       // not armed: the host's conditions do not hold (see tn_train_step), every launch as without the switch
#define TN_FOLD_ADAM_FUSED 1.0f      // the fold steps the table (or leaves it alone when found_inf of its group is raised); no table gradient is stored
#define TN_FOLD_ADAM_FELL_BACK 2.0f  // max |d enc| > FLT_MAX / (8 P), or not finite: a slot's sum might leave float range -- fold and Adam as unfused
struct FoldAdamHost {
  float *p, *m, *v;  // the table's piece of the parameter arena (p == grid.table) and of both moment arenas
  float* state;
  float* found_inf;  // the whole array
  int flag;          // the table's group
  const int32_t* skipped;
  int lag_index;
  int step, max_steps, sched_step;
  double lr, lr_final, beta1, beta2;
  float eps;
  // the group's small ranges (MLP weights, embedding: final when the bin launch has ended), checked by the launch between bin and fold
  const float* grads;
  int ncheck;
  int64_t check_off[TN_TRAIN_STEP_MAX_RANGES], check_cnt[TN_TRAIN_STEP_MAX_RANGES];
};
