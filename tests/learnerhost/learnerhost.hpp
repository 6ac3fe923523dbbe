// Host build of the PPO learner's kernel source (balance_robot_mujoco_rl_amd/csrc/brs_learner.hpp): the loss heads, the
// advantage statistics, the order in which the workgroups' partial rows are combined, the norms, the clip scale and the Adam
// update are the header's; the towers, which the kernels run on the matrix cores, are plain loops here, and so are the sample
// contractions.  The split into workgroups and 256-sample chunks is brs_learner.hip's grad_body, written once over the same two
// families (PPO here, A2C in tests/a2chost/a2chost.hpp).  Shared by learnerhost.cpp (a library for tests/test_learner_cpu.py) and
// learnerhost_main.cpp (a program of its own, for the sanitizers).
#pragma once
#include <math.h>
#include <string.h>

#include <vector>

#include "brs_learner.hpp"

namespace learnerhost {

using namespace brs::learner;

// brs_learner.hip's PpoFamily: the config, the row of entry i, the actor head, whether it feeds the KL and clip-fraction sums
struct PpoFamily {
  using Config = brs_ppo_config;
  static constexpr bool RATIO_STATS = true;
  const float* logp_old;
  int32_t row(const int32_t* idx, int i) const { return idx[i]; }
  ActorHead head(const float* mean, const float* log_std, const float* a, int32_t r, float adv_n, const Config& c, float inv_m) const {
    return actor_head(mean, log_std, a, logp_old[r], adv_n, c, inv_m);
  }
};

struct HostLearner {
  int max_workgroups;
  std::vector<float> partial;
  float adv_stat[2] = {0.0f, 1.0f};
  brs_learner_info info;

  explicit HostLearner(int max_wg) : max_workgroups(max_wg > 0 ? max_wg : 256), partial((size_t)max_workgroups * ROW, 0.0f) {
    memset(&info, 0, sizeof(info));
  }

  void begin_iteration() { info.stopped = 0; }

  // forward, head and backward of one tower for one sample; adds the sample's gradient to `g` (the tower's slice of a partial row)
  template <int NOUT, class Head> static void tower_sample(const float* w, const float* x, float* g, Head&& head) {
    const float *W1 = w + O_W1, *b1 = w + O_B1, *W2 = w + O_W2, *b2 = w + O_B2, *W3 = w + O_W3, *b3 = W3 + NOUT * HID;
    float h1[HID], h2[HID], out[NOUT], dz3[NOUT], dz2[HID], dz1[HID];
    for (int j = 0; j < HID; j++) {
      float s = b1[j];
      for (int k = 0; k < OBS; k++) s += W1[j * OBS + k] * x[k];
      h1[j] = tanhf(s);
    }
    for (int j = 0; j < HID; j++) {
      float s = b2[j];
      for (int k = 0; k < HID; k++) s += W2[j * HID + k] * h1[k];
      h2[j] = tanhf(s);
    }
    for (int o = 0; o < NOUT; o++) {
      float s = b3[o];
      for (int k = 0; k < HID; k++) s += W3[o * HID + k] * h2[k];
      out[o] = s;
    }
    head(out, dz3);
    for (int j = 0; j < HID; j++) {
      float s = 0.0f;
      for (int o = 0; o < NOUT; o++) s += W3[o * HID + j] * dz3[o];
      dz2[j] = s * (1.0f - h2[j] * h2[j]);
    }
    for (int k = 0; k < HID; k++) {
      float s = 0.0f;
      for (int j = 0; j < HID; j++) s += W2[j * HID + k] * dz2[j];
      dz1[k] = s * (1.0f - h1[k] * h1[k]);
    }
    for (int j = 0; j < HID; j++) {
      for (int k = 0; k < OBS; k++) g[O_W1 + j * OBS + k] += dz1[j] * x[k];
      g[O_B1 + j] += dz1[j];
      for (int k = 0; k < HID; k++) g[O_W2 + j * HID + k] += dz2[j] * h1[k];
      g[O_B2 + j] += dz2[j];
    }
    for (int o = 0; o < NOUT; o++) {
      for (int k = 0; k < HID; k++) g[O_W3 + o * HID + k] += dz3[o] * h2[k];
      g[O_W3 + NOUT * HID + o] += dz3[o];
    }
  }

  // what launch_grad enqueues once the arguments are checked: learner_adv_kernel, the family's gradient kernel (grad_body),
  // learner_reduce_kernel
  template <class Family>
  void grad_kernels(const Family& family, const float* params, int n_rows, const float* obs, const float* act, const float* adv, const float* ret,
                    const int32_t* idx, int m, const typename Family::Config& c, float* grad_out) {
    if (c.normalize_adv) {  // learner_adv_kernel
      std::vector<double> S((size_t)ADV_THREADS), SS((size_t)ADV_THREADS);
      for (int t = 0; t < ADV_THREADS; t++) fold_adv(adv, idx, m, n_rows, t, S[(size_t)t], SS[(size_t)t]);
      tree_pairs(ADV_THREADS, [&](int a, int b) { S[(size_t)a] += S[(size_t)b]; SS[(size_t)a] += SS[(size_t)b]; });
      adv_mean_denom(S[0], SS[0], m, adv_stat);
    }
    const float adv_mean = c.normalize_adv ? adv_stat[0] : 0.0f, adv_denom = c.normalize_adv ? adv_stat[1] : 1.0f;
    const float inv_m = 1.0f / (float)m;
    const int nchunks = (m + CHUNK - 1) / CHUNK, G = nchunks < max_workgroups ? nchunks : max_workgroups;
    const float log_std[ACT] = {params[OFF_LOGSTD], params[OFF_LOGSTD + 1]};
    const auto& critic_cfg = shared_fields(c);
    for (int g = 0; g < G; g++) {  // grad_body, workgroup g
      float* row = &partial[(size_t)g * ROW];
      for (int i = 0; i < ROW; i++) row[i] = 0.0f;
      for (int chunk = g; chunk < nchunks; chunk += G)
        for (int i = chunk * CHUNK; i < (chunk + 1) * CHUNK && i < m; i++) {
          const int32_t r = family.row(idx, i);
          if (r < 0 || r >= n_rows) { row[NPARAM + NSTAT] += 1.0f; continue; }
          const float* x = obs + (size_t)OBS * r;
          tower_sample<ACT>(params + OFF_PI, x, row + OFF_PI, [&](const float* mean, float* d3) {
            const ActorHead hd = family.head(mean, log_std, act + (size_t)ACT * r, r, (adv[r] - adv_mean) / adv_denom, c, inv_m);
            d3[0] = hd.dmean[0]; d3[1] = hd.dmean[1];
            row[OFF_LOGSTD] += hd.dlog_std[0]; row[OFF_LOGSTD + 1] += hd.dlog_std[1];
            row[NPARAM + S_PL] += hd.pl; row[NPARAM + S_ENT] += hd.ent;
            if constexpr (Family::RATIO_STATS) { row[NPARAM + S_KL] += hd.kl; row[NPARAM + S_CLIPFRAC] += hd.clipfrac; }
          });
          tower_sample<1>(params + OFF_VF, x, row + OFF_VF, [&](const float* v, float* d3) {
            const CriticHead hd = critic_head(v[0], ret[r], critic_cfg, inv_m);
            d3[0] = hd.dvalue;
            row[NPARAM + S_VL] += hd.vl;
          });
        }
    }
    for (int col = 0; col < NPARAM + NSTAT; col++) grad_out[col] = combine_rows(partial.data(), G, col);  // learner_reduce_kernel
    info.bad_index = (int32_t)combine_rows(partial.data(), G, NPARAM + NSTAT);
  }

  // the opening of both apply kernels (brs_learner.hip's grad_norms)
  static void grad_norms(const float* grad_in, const brs_ppo_config& clip_cfg, float& norm_pi, float& norm_vf) {
    std::vector<double> SP((size_t)APPLY_THREADS), SV((size_t)APPLY_THREADS);
    for (int t = 0; t < APPLY_THREADS; t++) fold_squares(grad_in, t, SP[(size_t)t], SV[(size_t)t]);
    tree_pairs(APPLY_THREADS, [&](int a, int b) { SP[(size_t)a] += SP[(size_t)b]; SV[(size_t)a] += SV[(size_t)b]; });
    norms(SP[0], SV[0], clip_cfg, norm_pi, norm_vf);
  }

  // brs_learner_grad: BRS_OK or BRS_ERR_ARG
  int grad(const float* params, int n_rows, const float* obs, const float* act, const float* logp_old, const float* adv, const float* ret,
           const int32_t* idx, int m, const brs_ppo_config* cfg, float* grad_out) {
    if (!cfg || (m > 0 && !idx) || m < 2 || n_rows <= 0 || !(cfg->ret_scale > 0.0f)) return BRS_ERR_ARG;
    grad_kernels(PpoFamily{logp_old}, params, n_rows, obs, act, adv, ret, idx, m, *cfg, grad_out);
    return BRS_OK;
  }

  // brs_learner_apply / learner_apply_kernel
  int apply(float* params, const float* grad_in, float* m, float* v, const brs_ppo_config* cfg) {
    if (!cfg || !params || !grad_in || !m || !v) return BRS_ERR_ARG;
    const brs_ppo_config& c = *cfg;
    float norm_pi, norm_vf;
    grad_norms(grad_in, c, norm_pi, norm_vf);
    const bool stop = info.stopped || kl_stops(grad_in[NPARAM + S_KL], c);
    info.stopped = stop ? 1 : 0;
    for (int k = 0; k < NSTAT; k++) info.stat[k] = grad_in[NPARAM + k];
    info.grad_norm_pi = norm_pi; info.grad_norm_vf = norm_vf;
    if (stop) return BRS_OK;
    info.steps += 1;
    const AdamScalars a = adam_scalars(c, info.steps);
    for (int i = 0; i < NPARAM; i++) adam_update(params[i], m[i], v[i], grad_in[i] * param_scale(i, norm_pi, norm_vf, c), a);
    return BRS_OK;
  }
};

}  // namespace learnerhost
