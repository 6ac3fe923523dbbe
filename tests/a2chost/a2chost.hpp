// Host build of the A2C learner's kernel source (balance_robot_mujoco_rl_amd/csrc/brs_learner.hpp): the A2C actor
// head, row_at, the null-aware advantage fold, the order in which partial rows are combined, the norms, the clip scale and the
// RMSpropTFLike update are the header's; the towers are learnerhost::HostLearner::tower_sample's plain loops, and the split into
// workgroups and 256-sample chunks is brs_learner.hip's.  Shared by a2chost.cpp (a library for tests/test_a2c_cpu.py) and
// a2chost_main.cpp (a program of its own, for the sanitizers).
#pragma once
#include "../learnerhost/learnerhost.hpp"

namespace a2chost {

using namespace brs::learner;
using learnerhost::HostLearner;

struct HostA2C {
  int max_workgroups;
  std::vector<float> partial;
  float adv_stat[2] = {0.0f, 1.0f};
  brs_learner_info info;

  explicit HostA2C(int max_wg) : max_workgroups(max_wg > 0 ? max_wg : 256), partial((size_t)max_workgroups * ROW, 0.0f) {
    memset(&info, 0, sizeof(info));
  }

  // brs_a2c_grad: BRS_OK or BRS_ERR_ARG
  int grad(const float* params, int n_rows, const float* obs, const float* act, const float* adv, const float* ret, const int32_t* idx, int m,
           const brs_a2c_config* cfg, float* grad_out) {
    if (!cfg || m < 1 || (cfg->normalize_adv && m < 2) || (!idx && m > n_rows) || !(cfg->ret_scale > 0.0f) || n_rows <= 0) return BRS_ERR_ARG;
    const brs_a2c_config& c = *cfg;
    const brs_ppo_config critic_cfg = shared_fields(c);
    if (c.normalize_adv) {  // learner_adv_kernel
      std::vector<double> S((size_t)ADV_THREADS), SS((size_t)ADV_THREADS);
      for (int t = 0; t < ADV_THREADS; t++) fold_adv_rows(adv, idx, m, n_rows, t, S[(size_t)t], SS[(size_t)t]);
      tree_pairs(ADV_THREADS, [&](int a, int b) { S[(size_t)a] += S[(size_t)b]; SS[(size_t)a] += SS[(size_t)b]; });
      adv_mean_denom(S[0], SS[0], m, adv_stat);
    }
    const float adv_mean = c.normalize_adv ? adv_stat[0] : 0.0f, adv_denom = c.normalize_adv ? adv_stat[1] : 1.0f;
    const float inv_m = 1.0f / (float)m;
    const int nchunks = (m + CHUNK - 1) / CHUNK, G = nchunks < max_workgroups ? nchunks : max_workgroups;
    const float log_std[ACT] = {params[OFF_LOGSTD], params[OFF_LOGSTD + 1]};
    for (int g = 0; g < G; g++) {  // learner_a2c_grad_kernel, workgroup g
      float* row = &partial[(size_t)g * ROW];
      for (int i = 0; i < ROW; i++) row[i] = 0.0f;
      for (int chunk = g; chunk < nchunks; chunk += G)
        for (int i = chunk * CHUNK; i < (chunk + 1) * CHUNK && i < m; i++) {
          const int32_t r = row_at(idx, i);
          if (r < 0 || r >= n_rows) { row[NPARAM + NSTAT] += 1.0f; continue; }
          const float* x = obs + (size_t)OBS * r;
          HostLearner::tower_sample<ACT>(params + OFF_PI, x, row + OFF_PI, [&](const float* mean, float* d3) {
            const ActorHead hd = a2c_actor_head(mean, log_std, act + (size_t)ACT * r, (adv[r] - adv_mean) / adv_denom, c, inv_m);
            d3[0] = hd.dmean[0]; d3[1] = hd.dmean[1];
            row[OFF_LOGSTD] += hd.dlog_std[0]; row[OFF_LOGSTD + 1] += hd.dlog_std[1];
            row[NPARAM + S_PL] += hd.pl; row[NPARAM + S_ENT] += hd.ent;
          });
          HostLearner::tower_sample<1>(params + OFF_VF, x, row + OFF_VF, [&](const float* v, float* d3) {
            const CriticHead hd = critic_head(v[0], ret[r], critic_cfg, inv_m);
            d3[0] = hd.dvalue;
            row[NPARAM + S_VL] += hd.vl;
          });
        }
    }
    for (int col = 0; col < NPARAM + NSTAT; col++) grad_out[col] = combine_rows(partial.data(), G, col);  // learner_reduce_kernel
    info.bad_index = (int32_t)combine_rows(partial.data(), G, NPARAM + NSTAT);
    return BRS_OK;
  }

  // brs_a2c_apply / learner_rmsprop_apply_kernel
  int apply(float* params, const float* grad_in, float* sq, const brs_a2c_config* cfg) {
    if (!cfg || !params || !grad_in || !sq) return BRS_ERR_ARG;
    const brs_ppo_config clip_cfg = shared_fields(*cfg);
    std::vector<double> SP((size_t)APPLY_THREADS), SV((size_t)APPLY_THREADS);
    for (int t = 0; t < APPLY_THREADS; t++) fold_squares(grad_in, t, SP[(size_t)t], SV[(size_t)t]);
    tree_pairs(APPLY_THREADS, [&](int a, int b) { SP[(size_t)a] += SP[(size_t)b]; SV[(size_t)a] += SV[(size_t)b]; });
    float norm_pi, norm_vf;
    norms(SP[0], SV[0], clip_cfg, norm_pi, norm_vf);
    info.steps += 1;
    for (int k = 0; k < NSTAT; k++) info.stat[k] = grad_in[NPARAM + k];
    info.grad_norm_pi = norm_pi; info.grad_norm_vf = norm_vf;
    const RmspropScalars r = rmsprop_scalars(*cfg);
    for (int i = 0; i < NPARAM; i++) rmsprop_tf_update(params[i], sq[i], grad_in[i] * param_scale(i, norm_pi, norm_vf, clip_cfg), r);
    return BRS_OK;
  }
};

}  // namespace a2chost
