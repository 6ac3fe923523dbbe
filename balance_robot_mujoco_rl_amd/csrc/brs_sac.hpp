// brs_sac.hpp -- SAC on the DDPG widths and on SB3's default [256, 256] (include/brs_policy.h: brs_sac_*, BRS_ARCH_*; DESIGN.md 7.8,
// 7.12), the part shared by the HIP kernels
// (brs_offpolicy.hip: act and target; brs_ddpg_learner.hip: the actor's chain) and the host build the CPU tests hold against fp64
// torch autograd (tests/sachost): the shape of the squashed-Gaussian actor, the Philox blocks of the three noise streams, and
// everything that is not a matrix product -- the log-std clamp and its gate, the sample, logp, the two dz3 formulas, the
// min-select, the target combine, the statistics' shares -- plus the argument rules that need no device.  Compiles with g++.
#pragma once
#include <math.h>
#include <stdint.h>

#include "brs_ddpg_learner.hpp"  // tanh_with_grad, the row loops; brs_offpolicy.hpp through it

namespace brs {
namespace sac {

using namespace brs::ddpg_learner;

// SB3's SAC Actor with net_arch pi=[300, 200]: latent_pi, then mu and log_std, two Linear(200, 2) stacked into one output layer
struct SacActor { static constexpr int IN = OBS, H1 = 300, H2 = 200, OUT = 2 * ACT; static constexpr bool TANH = false; };
constexpr int SAC_NACTOR = nparam<SacActor>();        // the actor VECTOR has one more element: log_ent_coef
static_assert(SAC_NACTOR == BRS_SAC_NACTOR, "include/brs_policy.h");
constexpr int SAC_NSTAT = BRS_SAC_NSTAT;
// ... and with SB3's default net_arch = [256, 256]
struct SacActor256 { static constexpr int IN = OBS, H1 = 256, H2 = 256, OUT = 2 * ACT; static constexpr bool TANH = false; };
static_assert(nparam<SacActor256>() == BRS_SAC256_NACTOR && SacActor256::OUT == SacActor::OUT, "include/brs_policy.h");
// an architecture: the SAC actor and the critic of a handle.  Kernels and host loops are templates over it; the per-row
// arithmetic below does not depend on the widths.
struct ArchReference { static constexpr int ID = BRS_ARCH_REFERENCE; using Pi = SacActor; using Qf = Critic; };
struct ArchSacDefault { static constexpr int ID = BRS_ARCH_SAC_DEFAULT; using Pi = SacActor256; using Qf = Critic256; };
inline bool known_arch(int32_t arch) { return arch == BRS_ARCH_REFERENCE || arch == BRS_ARCH_SAC_DEFAULT; }
// f(A{}) for the architecture `arch` names (known_arch): how a call dispatches on its handle's
template <class F> auto with_arch(int32_t arch, F&& f) { return arch == BRS_ARCH_SAC_DEFAULT ? f(ArchSacDefault{}) : f(ArchReference{}); }
// the per-sample rows next to the hidden ones: dz3[4], the temperature's gradient share, then the SAC_NSTAT statistics; in the
// gradient buffer the last five follow b3 directly (b3 is the last parameter block)
constexpr int SAC_TAIL = 1 + SAC_NSTAT, SAC_Z3_ROWS = SacActor::OUT + SAC_TAIL, SAC_ROW_LEN = SAC_NACTOR + SAC_TAIL;

// ---- the sizing table of a learner handle (brs_ddpg_learner.hip: create).  What the SAC calls of architecture A keep in the scratch:
// the actor's image with its nine per-sample rows (Z3_ROWS = 4 holds dz3[OUT <= 2] and two statistics only), two images of the
// critic's back to back; and the two rows they write
template <class A> struct ArchDims {
  using Pi = typename A::Pi;
  using Qf = typename A::Qf;
  using PiLay = Layout<Pi, SAC_Z3_ROWS>;
  using QfLay = Layout<Qf>;
  static constexpr int ROW_LEN = nparam<Pi>() + SAC_TAIL, TWIN_ROW_LEN = 2 * nparam<Qf>() + BRS_TD3_NSTAT;
  static_assert(Pi::OUT + SAC_TAIL <= SAC_Z3_ROWS && Qf::OUT + NSTAT <= Z3_ROWS, "rows");
};
// the `sac` row of brs_ddpg_learner.hpp's table, and the table as create() reads it.  At the reference widths a SAC handle also serves
// the DDPG / TD3 calls: their images and rows fit (asserted); at other widths those calls are refused
template <class A> constexpr HandleSize sac_handle_size() {
  using D = ArchDims<A>;
  return HandleSize{std::max(D::PiLay::ROWS, 2 * D::QfLay::ROWS), std::max(D::ROW_LEN, D::TWIN_ROW_LEN)};
}
constexpr HandleSize handle_size(bool twin, bool sac, int32_t arch) {
  if (sac) return arch == BRS_ARCH_SAC_DEFAULT ? sac_handle_size<ArchSacDefault>() : sac_handle_size<ArchReference>();
  return ddpg_handle_size(twin);
}
static_assert(handle_size(true, true, BRS_ARCH_REFERENCE).scratch_rows >= handle_size(true, false, BRS_ARCH_REFERENCE).scratch_rows &&
              handle_size(true, true, BRS_ARCH_REFERENCE).partial_len >= handle_size(true, false, BRS_ARCH_REFERENCE).partial_len,
              "a SAC handle of the reference widths serves the DDPG and TD3 calls");

constexpr float LOG_STD_MIN = -20.0f, LOG_STD_MAX = 2.0f, SQUASH_EPS = 1e-6f, HALF_LOG_2PI = 0.9189385332046727f;

BRS_HD void sac_act_block(uint64_t seed, int64_t gid, uint32_t step, uint32_t* o) {
  philox4x32_10(step, BRS_SAC_TAG_ACT, (uint32_t)((uint64_t)gid & 0xffffffffu), (uint32_t)((uint64_t)gid >> 32), (uint32_t)(seed & 0xffffffffu),
                (uint32_t)(seed >> 32), o);
}
// row j of `draw` of brs_sac_td_target (BRS_SAC_TAG_TARGET) and of brs_sac_actor_grad (BRS_SAC_TAG_PI)
BRS_HD void sac_row_block(uint32_t tag, uint64_t seed, uint32_t draw, uint32_t j, uint32_t* o) {
  philox4x32_10(draw, tag, j, 0u, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), o);
}

// torch.clamp(log_std, -20, 2) and where its backward lets the gradient through (both ends included, as torch)
BRS_HD float clamp_log_std(float raw) { return clip_keep_nan(raw, LOG_STD_MIN, LOG_STD_MAX); }  // a NaN stays, as torch.clamp
BRS_HD bool log_std_gate(float raw) { return raw >= LOG_STD_MIN && raw <= LOG_STD_MAX; }
template <class P> BRS_HD float ent_coef_of(const float* actor) { return expf(actor[nparam<P>()]); }  // log_ent_coef follows actor P's b3
// (the name of it in the header as host mirrors were first written against it; nothing of this tree calls it any more)
BRS_HD float ent_coef(const float* actor) { return ent_coef_of<SacActor>(actor); }

// u = mu + sigma z: a product and a sum, on the device as on the host
BRS_HD float pre_squash(float mu, float sigma, float z) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float p = sigma * z;
  return mu + p;
}

// one row's sample from the actor's four outputs and its two normals.  g = 1 - a^2 comes from the exponential of the tanh
// (tanh_with_grad): logp and the gradient use it where SB3 writes 1 - tanh(u)^2.
struct Sample { float a[ACT], g[ACT], sigma[ACT], log_std[ACT], logp; };
BRS_HD void sample(const float* out, const float* z, Sample& s) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float lp = 0.0f;
  for (int k = 0; k < ACT; k++) {
    s.log_std[k] = clamp_log_std(out[ACT + k]);
    s.sigma[k] = expf(s.log_std[k]);
    tanh_with_grad(pre_squash(out[k], s.sigma[k], z[k]), &s.a[k], &s.g[k]);
    const float zz = 0.5f * z[k];
    const float gauss = -(zz * z[k]) - s.log_std[k] - HALF_LOG_2PI;
    lp += gauss - logf(s.g[k] + SQUASH_EPS);
  }
  s.logp = lp;
}

// the per-row tail of brs_sac_act; out[4] is the actor's output (ignored when random != 0)
BRS_HD void sac_act_tail(uint64_t seed, int64_t gid, uint32_t step, int deterministic, int random, const float* out, float* action, float* mu,
                         float* log_std, float* z) {
  uint32_t o[4];
  sac_act_block(seed, gid, step, o);
  normal_pair(o[0], o[1], z);
  for (int k = 0; k < ACT; k++) {
    if (random) {
      action[k] = mu[k] = uniform_action(o[2 + k]);
      log_std[k] = 0.0f;
    } else {
      mu[k] = out[k];
      log_std[k] = clamp_log_std(out[ACT + k]);
      action[k] = tanh_(deterministic ? mu[k] : pre_squash(mu[k], expf(log_std[k]), z[k]));
    }
  }
}

// which critic's Q is the minimum: critic 0 on a tie, as torch.min over the stacked pair; a NaN is selected, from whichever critic
BRS_HD int min_select(float q0, float q1) { return (q1 < q0 || (q1 != q1 && q0 == q0)) ? 1 : 0; }

// y = r + (1 - done) gamma (min(Q1', Q2') - alpha logp')
BRS_HD float sac_combine(float reward, uint8_t done, float gamma, float q0, float q1, float alpha, float logp) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float t = alpha * logp;
  const float v = (min_select(q0, q1) ? q1 : q0) - t;
  return td_combine(reward, done, gamma, v);
}

// d La / d u_k of a row: da = d (-Qmin / m) / d a_k from the critics, alpha_m = alpha / m;
// d (-log(1 - a^2 + eps)) / d u = 2 a (1 - a^2) / (1 - a^2 + eps)
BRS_HD float sac_du(float da, float a, float g, float alpha_m) { return da * g + alpha_m * (2.0f * a * g / (g + SQUASH_EPS)); }
// d La / d (raw log_std_k): through u (d u / d log_std = sigma z) and through logp's -log_std, behind the clamp's gate
BRS_HD float sac_dlog_std(float du, float sigma, float z, float alpha_m, float raw) {
  return log_std_gate(raw) ? du * sigma * z - alpha_m : 0.0f;
}

// the row's shares of the five sums behind the parameter blocks: the temperature's gradient -(mean logp + target_entropy) (zero
// with a fixed ent_coef), La = mean (alpha logp - Qmin), mean logp, mean Qmin, alpha
BRS_HD void sac_shares(int learn_alpha, float target_entropy, float alpha, float logp, float qmin, float inv_m, float* share) {
  share[0] = learn_alpha ? -(logp + target_entropy) * inv_m : 0.0f;
  share[1] = (alpha * logp - qmin) * inv_m;
  share[2] = logp * inv_m;
  share[3] = qmin * inv_m;
  share[4] = alpha * inv_m;
}

// ---- the argument rules that need no device: 0 or the text after the function's name and ": "
inline const char* sac_act_argument_error(const void* actor, int32_t n, const void* obs, int32_t random, const void* action) {
  if (n < 1) return "n must be at least 1";
  if (!action || (!random && (!actor || !obs))) return "null argument";
  return nullptr;
}
inline const char* sac_target_argument_error(const void* actor, const void* critics_t, int32_t m, const void* next_obs, const void* reward,
                                             const void* done, float gamma, const void* y) {
  if (!actor || !critics_t || !next_obs || !reward || !done || !y) return "null argument";
  if (m < 1) return "m must be at least 1";
  if (isnan(gamma) || isinf(gamma)) return "gamma must be finite";
  return nullptr;
}
inline const char* sac_critic_grad_argument_error(const void* critics, int32_t m, const void* obs, const void* act, const void* y, const void* grad) {
  if (!critics || !obs || !act || !y || !grad) return "null argument";
  if (m < 1) return "m must be at least 1";
  return nullptr;
}
inline const char* sac_actor_grad_argument_error(const void* actor, const void* critics, int32_t m, const void* obs, float target_entropy,
                                                 const void* grad) {
  if (!actor || !critics || !obs || !grad) return "null argument";
  if (m < 1) return "m must be at least 1";
  if (isnan(target_entropy) || isinf(target_entropy)) return "target_entropy must be finite";
  return nullptr;
}

}  // namespace sac
}  // namespace brs
