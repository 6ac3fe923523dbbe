// brs_ddpg_learner.hpp -- the DDPG learner of include/brs_policy.h, the part shared by the HIP kernels
// (brs_ddpg_learner.hip) and the host build the CPU tests hold against fp64 torch autograd (tests/ddpglearnerhost): everything
// that is not a matrix product -- the two loss heads, the tanh' factor, the gate rule, the statistics, the combine of partial
// rows, Adam plus Polyak per element -- and a plain-loop forward/backward of the two networks.  Compiles with g++.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "brs_offpolicy.hpp"  // Actor, Critic, Offsets, nparam
#include "brs_learner.hpp"    // AdamScalars

namespace brs {
namespace ddpg_learner {

using namespace brs::offpolicy;

constexpr int NSTAT = BRS_DDPG_NSTAT;
constexpr int Z3_ROWS = 4;  // per-sample rows next to the hidden ones: dz3[OUT] (OUT <= 2), then the NSTAT statistics
static_assert(Actor::OUT + NSTAT <= Z3_ROWS && Critic::OUT + NSTAT <= Z3_ROWS, "rows");
template <class N> constexpr int row_len() { return nparam<N>() + NSTAT; }  // a gradient buffer / a partial row

// ---- how the weight-gradient kernels of brs_ddpg_learner.hip split the sample axis: at 512 padded rows and more, over up to
// MAX_SPLIT workgroup rows of `span` samples each, every one writing a partial row of the handle.  Host code, here so that the
// CPU tests reach it (tests/ddpglearnerhost: dh_split_sweep).
constexpr int MAX_SPLIT = 8, SPLIT_ROWS = 256;
constexpr int pad128(int x) { return (x + 127) / 128 * 128; }
constexpr int TWIN_LEN = 2 * nparam<Critic>() + BRS_TD3_NSTAT;  // the twin gradient buffer / a twin partial row
static_assert(BRS_TD3_NSTAT == 2 * NSTAT, "two statistics per critic");
static_assert(row_len<Critic>() <= row_len<Actor>(), "the critic's row fits the actor's partial row");
// rows of a scratch image (each `ld` floats, ld = max_batch padded to the workgroup's 128 rows) sized for network N: the two hidden
// layers' activations and their gradients in [unit][sample] layout, then ZR per-sample rows.  The single calls use the actor's, the
// wider net, for both networks; the twin calls keep two images of the critic's back to back.  What a handle allocates of them:
// handle_size of brs_sac.hpp.
template <class N, int ZR = Z3_ROWS> struct Layout {
  static constexpr int H1 = 0, H2 = H1 + Padded<N>::H1P, DZ1 = H2 + Padded<N>::H2P, DZ2 = DZ1 + Padded<N>::H1P, Z3 = DZ2 + Padded<N>::H2P, ROWS = Z3 + ZR;
};
using Wide = Layout<Actor>;
using Narrow = Layout<Critic>;
static_assert(Padded<Critic>::H1P <= Padded<Actor>::H1P && Padded<Critic>::H2P <= Padded<Actor>::H2P, "the critic fits in the actor's scratch");
// ---- the sizing table of a learner handle (brs_ddpg_learner.hip: create): scratch rows (each max_batch padded to 128 floats) and the
// length of each of the MAX_SPLIT partial rows behind them -- the largest image and the longest row of any call the handle serves.
//   single (brs_ddpg_learner_create)  the actor's image serves both networks; the actor's row
//   twin   (..._create_twin)          that, or two critic images back to back; that, or two critics side by side in a row
//   sac    (..._create_sac[_arch])    brs_sac.hpp: handle_size, which is what create() calls
struct HandleSize { int scratch_rows, partial_len; };
constexpr HandleSize ddpg_handle_size(bool twin) {
  return twin ? HandleSize{std::max(Wide::ROWS, 2 * Narrow::ROWS), std::max(row_len<Actor>(), TWIN_LEN)} : HandleSize{Wide::ROWS, row_len<Actor>()};
}
// floats such a handle keeps for partial rows (the host build's sweep of the split holds every m against it)
constexpr size_t partial_floats(bool twin) { return (size_t)MAX_SPLIT * ddpg_handle_size(twin).partial_len; }

struct SampleSplit { int mp, span, nsplit; };  // samples padded to 128; samples per split (a multiple of 128); splits launched
inline SampleSplit sample_split(int m) {
  const int mp = pad128(m);
  int nsplit = mp / SPLIT_ROWS;
  nsplit = nsplit < 1 ? 1 : (nsplit > MAX_SPLIT ? MAX_SPLIT : nsplit);
  const int span = pad128((mp + nsplit - 1) / nsplit);
  nsplit = (mp + span - 1) / span;
  return SampleSplit{mp, span, nsplit};
}

// ReLU's backward gate, as torch's: closed where the pre-activation (equivalently: the ReLU's output) is <= 0, so open for a NaN
BRS_HD bool relu_gate(float pre) { return relu_gate_keep_nan(pre); }

// ---- the loss heads; everything carries the 1 / m of the mean, so that sums over rows are means
struct CriticHead { float dq, loss, q; };
// Lc = mean (q - y)^2
BRS_HD CriticHead critic_head(float q, float y, float inv_m) {
  const float d = q - y;
  return CriticHead{2.0f * d * inv_m, d * d * inv_m, q * inv_m};
}
// La = -mean Q(s, pi(s)): d La / d q of a row, and the row's share of the two statistics
BRS_HD float actor_dq(float inv_m) { return -inv_m; }
BRS_HD float actor_loss_share(float q, float inv_m) { return -q * inv_m; }
BRS_HD float actor_sat_share(const float* a, float inv_m) { return 0.5f * (a[0] * a[0] + a[1] * a[1]) * inv_m; }

// tanh and its derivative from ONE exponential: a = 1 - 2 / (e + 1), 1 - a^2 = 4 e / (e + 1)^2 with e = exp(2 x).  The second
// form has no cancellation where the tanh saturates (1 - a * a would carry a's absolute error of ~1e-7 into a factor of 1e-4).
// a is tanh_ of brs_offpolicy.hpp bit for bit.
BRS_HD void tanh_with_grad(float x, float* a, float* g) {
  const float e = expf(2.0f * x), d = e + 1.0f;
  *a = 1.0f - 2.0f / d;
  *g = e >= 1e18f ? 0.0f : 4.0f * e / (d * d);  // (e + 1)^2 overflows past 1.8e19; the factor is below 4e-18 there.  A NaN stays
}

// ---- column `col` of G partial rows of `len` floats, summed in ascending order of the row (brs_learner.hpp's combine_rows)
BRS_HD float combine_partials(const float* partial, int G, int len, int col) {
  double s = 0.0;
  for (int g = 0; g < G; g++) s += (double)partial[(size_t)g * len + col];
  return (float)s;
}

// ---- Adam, then the Polyak update of the target from the NEW parameter: torch's lerp_ for a weight below 0.5
using learner::adam_scalars;  // the one of brs_learner.hpp, over brs_adam_config
BRS_HD float polyak(float target, float param, float tau) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float d = param - target;
  const float s = tau * d;
  return target + s;
}
// learner::adam_update's arithmetic, operation by operation, with contraction off: the kernel and the host build return the
// same bytes (sqrt and the division are correctly rounded on both sides).  adam_update itself is compiled with the device's
// default contraction, which fuses m + (g - m) w1 on the GPU and not under g++; the PPO learner's results stay as they are.
BRS_HD void apply_element(float& p, float& m, float& v, float g, const learner::AdamScalars& a) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float dm = (g - m) * a.w1;
  m = m + dm;
  const float v1 = v * a.beta2, g2 = a.w2 * g;
  const float v2 = g2 * g;
  v = v1 + v2;
  const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
  const float q = m / denom;
  const float u = a.step_size * q;
  p = p - u;
}

// the argument rules of brs_ddpg_learner_apply that need no device: 0 or the text after "brs_ddpg_learner_apply: "
inline const char* apply_argument_error(int32_t n_param, const void* params, const void* grad, const void* m, const void* v,
                                        const brs_adam_config* cfg, int64_t step, float tau) {
  if (!cfg) return "null config";
  if (!params || !grad || !m || !v) return "null argument";
  if (n_param < 1) return "n_param must be at least 1";
  if (step < 1) return "step must be at least 1";
  if (!(tau >= 0.0f && tau <= 1.0f)) return "tau must be in [0, 1]";
  if (!(cfg->lr >= 0.0) || !(cfg->eps >= 0.0)) return "lr and eps must be >= 0";
  if (!(cfg->beta1 >= 0.0 && cfg->beta1 < 1.0) || !(cfg->beta2 >= 0.0 && cfg->beta2 < 1.0)) return "betas must be in [0, 1)";
  return nullptr;
}

// ---- the host's forward and backward of one row: plain loops in fp32, as forward_row of brs_offpolicy.hpp
template <class N> struct RowTape {
  float x[N::IN], h1[N::H1], h2[N::H2], pre[N::OUT];
};
template <class N> inline void forward_row_keep(const float* w, const float* x, RowTape<N>& t) {
  using O = Offsets<N>;
  for (int k = 0; k < N::IN; k++) t.x[k] = x[k];
  for (int u = 0; u < N::H1; u++) {
    float s = w[O::B1 + u];
    for (int k = 0; k < N::IN; k++) s = fmaf(w[O::W1 + u * N::IN + k], x[k], s);
    t.h1[u] = relu_keep_nan(s);
  }
  for (int u = 0; u < N::H2; u++) {
    float s = w[O::B2 + u];
    for (int k = 0; k < N::H1; k++) s = fmaf(w[O::W2 + u * N::H1 + k], t.h1[k], s);
    t.h2[u] = relu_keep_nan(s);
  }
  for (int u = 0; u < N::OUT; u++) {
    float s = 0.0f;
    for (int k = 0; k < N::H2; k++) s = fmaf(w[O::W3 + u * N::H2 + k], t.h2[k], s);
    t.pre[u] = s + w[O::B3 + u];
  }
}
// dz3[OUT] = d loss / d (output before the tanh) of this row -> its share of the gradient, added to grad[nparam] (fp64: the sums
// over the rows are the host's own; the kernels take them in fp32 on the matrix cores, in their order); dx (may be null)
// receives d loss / d input
template <class N> inline void backward_row(const float* w, const RowTape<N>& t, const float* dz3, double* grad, float* dx) {
  using O = Offsets<N>;
  float dz2[N::H2], dz1[N::H1];
  for (int u = 0; u < N::H2; u++) {
    float s = 0.0f;
    for (int k = 0; k < N::OUT; k++) s = fmaf(w[O::W3 + k * N::H2 + u], dz3[k], s);
    dz2[u] = relu_gate(t.h2[u]) ? s : 0.0f;
  }
  for (int k = 0; k < N::H1; k++) {
    float s = 0.0f;
    for (int u = 0; u < N::H2; u++) s = fmaf(w[O::W2 + u * N::H1 + k], dz2[u], s);
    dz1[k] = relu_gate(t.h1[k]) ? s : 0.0f;
  }
  if (grad) {
    for (int u = 0; u < N::H1; u++) {
      for (int k = 0; k < N::IN; k++) grad[O::W1 + u * N::IN + k] += (double)dz1[u] * (double)t.x[k];
      grad[O::B1 + u] += (double)dz1[u];
    }
    for (int u = 0; u < N::H2; u++) {
      for (int k = 0; k < N::H1; k++) grad[O::W2 + u * N::H1 + k] += (double)dz2[u] * (double)t.h1[k];
      grad[O::B2 + u] += (double)dz2[u];
    }
    for (int u = 0; u < N::OUT; u++) {
      for (int k = 0; k < N::H2; k++) grad[O::W3 + u * N::H2 + k] += (double)dz3[u] * (double)t.h2[k];
      grad[O::B3 + u] += (double)dz3[u];
    }
  }
  if (dx)
    for (int k = 0; k < N::IN; k++) {
      float s = 0.0f;
      for (int u = 0; u < N::H1; u++) s = fmaf(w[O::W1 + u * N::IN + k], dz1[u], s);
      dx[k] = s;
    }
}

// the loss head with a factor in front of the loss (SAC's 0.5, a power of two: exact; the DDPG / TD3 calls pass 1, exact too)
BRS_HD CriticHead scale_head(CriticHead h, float loss_scale) { return CriticHead{h.dq * loss_scale, h.loss * loss_scale, h.q}; }

// the rows of loss_scale mse(Q(s, a), y) for critic Q, summed into g[nparam<Q>() + NSTAT]: the gradient, then the loss and mean Q
template <class Q> inline void critic_grad_rows(const float* critic, int m, const float* obs, const float* act, const float* y, float loss_scale,
                                                double* g) {
  const float inv_m = 1.0f / (float)m;
  RowTape<Q> t;
  for (int i = 0; i < m; i++) {
    float x[Q::IN];
    for (int k = 0; k < OBS; k++) x[k] = obs[(size_t)OBS * i + k];
    for (int k = 0; k < ACT; k++) x[OBS + k] = act[(size_t)ACT * i + k];
    forward_row_keep<Q>(critic, x, t);
    const CriticHead hd = scale_head(critic_head(t.pre[0], y[i], inv_m), loss_scale);
    backward_row<Q>(critic, t, &hd.dq, g, nullptr);
    g[nparam<Q>()] += (double)hd.loss;
    g[nparam<Q>() + 1] += (double)hd.q;
  }
}
// grad[NCRITIC + 2]
inline void critic_grad_host(const float* critic, int m, const float* obs, const float* act, const float* y, float* grad) {
  std::vector<double> g((size_t)row_len<Critic>(), 0.0);
  critic_grad_rows<Critic>(critic, m, obs, act, y, 1.0f, g.data());
  for (int j = 0; j < row_len<Critic>(); j++) grad[j] = (float)g[j];
}
// grad[2 nparam<Q>() + 4]: block 0, block 1, then (loss, mean Q) of critic 0 and of critic 1
template <class Q> inline void twin_critic_grad_host(const float* critics, int m, const float* obs, const float* act, const float* y,
                                                     float loss_scale, float* grad) {
  constexpr int NC = nparam<Q>();
  for (int c = 0; c < 2; c++) {
    std::vector<double> g((size_t)NC + NSTAT, 0.0);
    critic_grad_rows<Q>(critics + (size_t)c * NC, m, obs, act, y, loss_scale, g.data());
    for (int j = 0; j < NC; j++) grad[(size_t)c * NC + j] = (float)g[j];
    for (int j = 0; j < NSTAT; j++) grad[2 * (size_t)NC + (size_t)c * NSTAT + j] = (float)g[NC + j];
  }
}

// grad[NACTOR + 2]
inline void actor_grad_host(const float* actor, const float* critic, int m, const float* obs, float* grad) {
  std::vector<double> g((size_t)row_len<Actor>(), 0.0);
  const float inv_m = 1.0f / (float)m;
  RowTape<Actor> ta;
  RowTape<Critic> tc;
  for (int i = 0; i < m; i++) {
    float x[Critic::IN], a[ACT], ga[ACT], dx[Critic::IN], dz3[ACT];
    for (int k = 0; k < OBS; k++) x[k] = obs[(size_t)OBS * i + k];
    forward_row_keep<Actor>(actor, x, ta);
    for (int k = 0; k < ACT; k++) { tanh_with_grad(ta.pre[k], &a[k], &ga[k]); x[OBS + k] = a[k]; }
    forward_row_keep<Critic>(critic, x, tc);
    const float dq = actor_dq(inv_m);
    backward_row<Critic>(critic, tc, &dq, nullptr, dx);
    for (int k = 0; k < ACT; k++) dz3[k] = dx[OBS + k] * ga[k];
    backward_row<Actor>(actor, ta, dz3, g.data(), nullptr);
    g[nparam<Actor>()] += (double)actor_loss_share(tc.pre[0], inv_m);
    g[nparam<Actor>() + 1] += (double)actor_sat_share(a, inv_m);
  }
  for (int j = 0; j < row_len<Actor>(); j++) grad[j] = (float)g[j];
}

inline void apply_host(int n_param, float* params, const float* grad, float* m, float* v, float* target, const brs_adam_config& cfg,
                       int64_t step, float tau) {
  const learner::AdamScalars a = adam_scalars(cfg, step);
  for (int i = 0; i < n_param; i++) {
    apply_element(params[i], m[i], v[i], grad[i], a);
    if (target) target[i] = polyak(target[i], params[i], tau);
  }
}

}  // namespace ddpg_learner
}  // namespace brs
