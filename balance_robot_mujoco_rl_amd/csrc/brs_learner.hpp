// brs_learner.hpp -- the PPO learner of include/brs_policy.h and the A2C learner on the same handle (7.9), the part shared by the HIP kernels
// (brs_learner.hip) and the host build the CPU tests hold against fp64 torch autograd (tests/learnerhost): everything that is
// not a matrix product -- the per-sample loss heads, the order in which partial sums are combined, the clip scale and the Adam
// update.  The towers themselves are MFMA code in the kernels (brs_policy_tile.hpp, which takes the layout of the flat parameter
// vector from the constants below, as brs_policy.hip does through it) and plain loops in the host build.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/brs.h"
#include "../../include/brs_policy.h"
#include "brs_nan.hpp"  // the selects that keep a NaN

#ifndef BRS_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BRS_HD __host__ __device__ __forceinline__
#else
#define BRS_HD inline
#endif
#endif

namespace brs {
namespace learner {

constexpr int OBS = BRS_POLICY_OBS, HID = BRS_POLICY_HID, ACT = BRS_POLICY_ACT, NPARAM = BRS_POLICY_NPARAM, NSTAT = BRS_LEARNER_NSTAT;
constexpr int OFF_PI = 0, OFF_VF = BRS_POLICY_NPI, OFF_LOGSTD = BRS_POLICY_NPI + BRS_POLICY_NVF;
// inside a tower: W1[64][6] b1[64] W2[64][64] b2[64] W3[NOUT][64] b3[NOUT]
constexpr int O_W1 = 0, O_B1 = O_W1 + HID * OBS, O_W2 = O_B1 + HID, O_B2 = O_W2 + HID * HID, O_W3 = O_B2 + HID;
constexpr int CHUNK = 256;  // samples a workgroup takes per trip; workgroup g takes chunks g, g + G, ... of G workgroups
// a partial row (one per workgroup): the gradient sums, the NSTAT stat sums, the count of bad indices
constexpr int ROW = NPARAM + NSTAT + 1;
constexpr int APPLY_THREADS = 1024, ADV_THREADS = 1024;
enum { S_PL = 0, S_VL = 1, S_ENT = 2, S_KL = 3, S_CLIPFRAC = 4 };

// ---- per-sample loss heads.  Everything carries the 1 / M of the minibatch mean, so that sums over samples are means.
struct ActorHead {
  float dmean[ACT];     // d loss / d mean
  float dlog_std[ACT];  // this sample's share of d loss / d log_std
  float pl, ent, kl, clipfrac;
};

// what both actor heads start from: the standardised action, log pi(a | s) and the entropy of the diagonal Gaussian
struct GaussianTerms {
  float z[ACT], inv_sigma[ACT], lp, ent;
};
BRS_HD GaussianTerms gaussian_terms(const float mean[ACT], const float log_std[ACT], const float act[ACT]) {
  GaussianTerms t;
  t.lp = 0.0f; t.ent = 0.0f;
  for (int k = 0; k < ACT; k++) {
    t.inv_sigma[k] = expf(-log_std[k]);
    t.z[k] = (act[k] - mean[k]) * t.inv_sigma[k];
    t.lp += -0.5f * t.z[k] * t.z[k] - log_std[k] - 0.9189385332046727f;
    t.ent += 1.4189385332046727f + log_std[k];  // 0.5 + 0.5 log(2 pi) + log sigma
  }
  return t;
}
// z^2 - 1.  The device build has always contracted it to one fma -- but only because the SLP vectoriser happened to keep the square
// and the difference of the two actions in one packed chain; with the accumulators of the gradient kernel paired another way the
// square is rounded first and the log_std gradient moves in its last bit.  Written out so that the kernels do not depend on that.
// The host build is compiled without contraction and rounds the square, as it always has
BRS_HD float square_minus_one(float z) {
#if defined(__HIP_DEVICE_COMPILE__)
  return fmaf(z, z, -1.0f);
#else
  return z * z - 1.0f;
#endif
}
// ... and end with: dmean and dlog_std from g_lp = d loss / d log pi (zero with the actor off)
template <class Config>  // anything with actor_on and ent_coef
BRS_HD void actor_head_gradients(ActorHead& o, const GaussianTerms& t, float g_lp, const Config& c, float inv_m) {
  for (int k = 0; k < ACT; k++) {
    if (c.actor_on) {
      o.dmean[k] = g_lp * t.z[k] * t.inv_sigma[k];
      o.dlog_std[k] = g_lp * square_minus_one(t.z[k]) - c.ent_coef * inv_m;
    } else {
      o.dmean[k] = 0.0f;
      o.dlog_std[k] = 0.0f;
    }
  }
}

// adv_n: the (normalised) advantage.  loss = -min(ratio adv, clamp(ratio) adv) - ent_coef entropy
BRS_HD ActorHead actor_head(const float mean[ACT], const float log_std[ACT], const float act[ACT], float logp_old, float adv_n,
                            const brs_ppo_config& c, float inv_m) {
  ActorHead o;
  const GaussianTerms t = gaussian_terms(mean, log_std, act);
  const float lr = t.lp - logp_old, ratio = expf(lr);
  const float clamped = fminf(fmaxf(ratio, 1.0f - c.clip_range), 1.0f + c.clip_range);  // of a NaN ratio: a number; s1 keeps the NaN
  const float s1 = ratio * adv_n, s2 = clamped * adv_n;
  o.pl = -min_keep_nan(s1, s2) * inv_m;
  o.ent = t.ent * inv_m;
  o.kl = ((ratio - 1.0f) - lr) * inv_m;
  o.clipfrac = fabsf(ratio - 1.0f) > c.clip_range ? inv_m : 0.0f;
  // the clamped branch has no gradient where the clamp is active, and where it is not the two branches are the same function;
  // a NaN on either side leaves the gate open, so that the row's NaN reaches the gradient as it reaches torch.min's
  const float g_lp = (c.actor_on && !(s1 > s2)) ? -adv_n * ratio * inv_m : 0.0f;
  actor_head_gradients(o, t, g_lp, c, inv_m);
  return o;
}

struct CriticHead {
  float dvalue, vl;
};

// loss = vf_coef * 0.5 (v - ret / ret_scale)^2
BRS_HD CriticHead critic_head(float value, float ret, const brs_ppo_config& c, float inv_m) {
  const float d = value - ret / c.ret_scale;
  return CriticHead{c.vf_coef * d * inv_m, 0.5f * d * d * inv_m};
}

// ---- A2C: SB3's A2C.train() on the same towers.  policy loss = -adv_n log pi(a | s), no ratio and no clip, so
// there is no logp_old, and the KL and clip-fraction slots of the stats stay zero.  The value loss is critic_head's, the
// convention PPO uses: vf_coef * 0.5 (v - ret / ret_scale)^2 -- SB3's vf_coef = 0.5 on mse_loss is vf_coef = 1.0 here.
template <class Config>  // brs_a2c_config: anything with actor_on and ent_coef
BRS_HD ActorHead a2c_actor_head(const float mean[ACT], const float log_std[ACT], const float act[ACT], float adv_n, const Config& c,
                                float inv_m) {
  ActorHead o;
  const GaussianTerms t = gaussian_terms(mean, log_std, act);
  o.pl = -adv_n * t.lp * inv_m;
  o.ent = t.ent * inv_m;
  o.kl = 0.0f;
  o.clipfrac = 0.0f;
  const float g_lp = c.actor_on ? -adv_n * inv_m : 0.0f;
  actor_head_gradients(o, t, g_lp, c, inv_m);
  return o;
}
// what critic_head, norms and param_scale read of a config, for brs_a2c_config's callers; a brs_ppo_config is its own
BRS_HD brs_ppo_config shared_fields(const brs_a2c_config& c) {
  brs_ppo_config p = {};
  p.vf_coef = c.vf_coef; p.ent_coef = c.ent_coef; p.max_grad_norm_pi = c.max_grad_norm_pi; p.max_grad_norm_vf = c.max_grad_norm_vf;
  p.ret_scale = c.ret_scale; p.normalize_adv = c.normalize_adv; p.actor_on = c.actor_on; p.joint_norm = c.joint_norm;
  return p;
}
BRS_HD const brs_ppo_config& shared_fields(const brs_ppo_config& c) { return c; }

BRS_HD ActorHead zero_actor_head() { return ActorHead{{0.0f, 0.0f}, {0.0f, 0.0f}, 0.0f, 0.0f, 0.0f, 0.0f}; }

// ---- entry i of a minibatch: row idx[i], or row i of the buffer when the minibatch is the whole buffer in its own order (idx
// null: A2C alone, brs_learner_grad refuses it)
BRS_HD int32_t row_at(const int32_t* idx, int i) { return idx ? idx[i] : (int32_t)i; }

// ---- advantage mean and std of the minibatch: thread t of ADV_THREADS folds entries t, t + ADV_THREADS, ... in ascending
// order into (sum, sum of squares) in fp64, the partials are combined by a tree of fixed pairing (tree_pairs below)
BRS_HD void fold_adv(const float* adv, const int32_t* idx, int m, int n_rows, int t, double& s, double& ss) {
  s = 0.0; ss = 0.0;
  for (int i = t; i < m; i += ADV_THREADS) {
    const int32_t row = row_at(idx, i);
    if (row < 0 || row >= n_rows) continue;
    const double a = (double)adv[row];
    s += a; ss += a * a;
  }
}
// the name the fold through row_at had while there were two; host builds written against that header still compile
BRS_HD void fold_adv_rows(const float* adv, const int32_t* idx, int m, int n_rows, int t, double& s, double& ss) {
  fold_adv(adv, idx, m, n_rows, t, s, ss);
}
// -> out[0] = mean, out[1] = unbiased std + 1e-8: adv_n = (adv - out[0]) / out[1]
BRS_HD void adv_mean_denom(double s, double ss, int m, float* out) {
  const double mean = s / (double)m;
  double var = (ss - (double)m * mean * mean) / (double)(m - 1);
  if (var < 0.0) var = 0.0;
  out[0] = (float)mean;
  out[1] = (float)sqrt(var) + 1e-8f;
}

// ---- column `col` of the G partial rows, summed in ascending order of the workgroup
BRS_HD float combine_rows(const float* partial, int G, int col) {
  double s = 0.0;
  for (int g = 0; g < G; g++) s += (double)partial[(size_t)g * ROW + col];
  return (float)s;
}

// ---- gradient norms: actor + log_std on one side, critic on the other; same fold and tree as the advantage statistics
BRS_HD bool is_critic(int i) { return i >= OFF_VF && i < OFF_LOGSTD; }
BRS_HD void fold_squares(const float* grad, int t, double& pi, double& vf) {
  pi = 0.0; vf = 0.0;
  for (int i = t; i < NPARAM; i += APPLY_THREADS) {
    const double g = (double)grad[i];
    if (is_critic(i)) vf += g * g; else pi += g * g;
  }
}
// what the norms become under the config's clip mode, and torch.nn.utils.clip_grad_norm_'s scale
BRS_HD void norms(double sq_pi, double sq_vf, const brs_ppo_config& c, float& norm_pi, float& norm_vf) {
  if (c.joint_norm) { norm_pi = norm_vf = (float)sqrt(sq_pi + sq_vf); }
  else { norm_pi = (float)sqrt(sq_pi); norm_vf = (float)sqrt(sq_vf); }
}
BRS_HD float clip_scale(float norm, float max_norm) { return fminf(1.0f, max_norm / (norm + 1e-6f)); }
BRS_HD float param_scale(int i, float norm_pi, float norm_vf, const brs_ppo_config& c) {
  return (is_critic(i) && !c.joint_norm) ? clip_scale(norm_vf, c.max_grad_norm_vf) : clip_scale(norm_pi, c.max_grad_norm_pi);
}

// ---- early stop: SB3's target_kl
BRS_HD bool kl_stops(float kl, const brs_ppo_config& c) { return c.target_kl > 0.0f && kl > 1.5f * c.target_kl; }

// ---- torch.optim.Adam (no amsgrad, no weight decay), step counted from 1; the bias corrections are formed in fp64 as torch forms
// them in Python floats
struct AdamScalars {
  float step_size, bc2_sqrt, w1, beta2, w2, eps;
};
template <class Config>  // brs_ppo_config, brs_adam_config: anything with lr, beta1, beta2, eps in fp64
BRS_HD AdamScalars adam_scalars(const Config& c, int64_t step) {
  const double bc1 = 1.0 - pow(c.beta1, (double)step), bc2 = 1.0 - pow(c.beta2, (double)step);
  return AdamScalars{(float)(c.lr / bc1), (float)sqrt(bc2), (float)(1.0 - c.beta1), (float)c.beta2, (float)(1.0 - c.beta2), (float)c.eps};
}
BRS_HD void adam_update(float& p, float& m, float& v, float g, const AdamScalars& a) {
  m = m + (g - m) * a.w1;                           // exp_avg.lerp_(grad, 1 - beta1)
  v = v * a.beta2 + a.w2 * g * g;                   // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
  const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
  p = p - a.step_size * (m / denom);                // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// ---- SB3's RMSpropTFLike (alpha, eps; no momentum, not centered, no weight decay): square_avg starts at ONE and epsilon sits
// INSIDE the root -- the two points where it leaves torch.optim.RMSprop.  lr, alpha and eps are rounded to fp32 once
struct RmspropScalars {
  float lr, alpha, w, eps;
};
template <class Config>  // brs_a2c_config: anything with lr, alpha, eps in fp64
BRS_HD RmspropScalars rmsprop_scalars(const Config& c) {
  return RmspropScalars{(float)c.lr, (float)c.alpha, (float)(1.0 - c.alpha), (float)c.eps};
}
BRS_HD void rmsprop_tf_update(float& p, float& sq, float g, const RmspropScalars& s) {
  sq = sq * s.alpha + s.w * g * g;        // square_avg.mul_(alpha).addcmul_(grad, grad, value=1 - alpha)
  const float avg = sqrtf(sq + s.eps);    // square_avg.add(eps).sqrt_()
  p = p - s.lr * (g / avg);               // param.addcdiv_(grad, avg, value=-lr)
}

// the tree both reductions use: partial t takes partial t + s for s = n / 2, n / 4, ... 1 (n a power of two)
template <class F> BRS_HD void tree_pairs(int n, F&& take) {
  for (int s = n / 2; s >= 1; s >>= 1)
    for (int t = 0; t < s; t++) take(t, t + s);
}

}  // namespace learner
}  // namespace brs
