// Host build of the A2C learner's kernel source (balance_robot_mujoco_rl_amd/csrc/brs_learner.hpp): the A2C actor
// head, row_at, the advantage fold, the order in which partial rows are combined, the norms, the clip scale and the RMSpropTFLike
// update are the header's; the towers, the split into workgroups and 256-sample chunks and the opening of the apply kernel are
// learnerhost::HostLearner's, over the A2C family below -- as brs_learner.hip's grad_body serves both families on one handle.
// Shared by a2chost.cpp (a library for tests/test_a2c_cpu.py) and a2chost_main.cpp (a program of its own, for the sanitizers).
#pragma once
#include "../learnerhost/learnerhost.hpp"

namespace a2chost {

using namespace brs::learner;
using learnerhost::HostLearner;

// brs_learner.hip's A2cFamily
struct A2cFamily {
  using Config = brs_a2c_config;
  static constexpr bool RATIO_STATS = false;  // the KL and clip-fraction sums stay zero
  int32_t row(const int32_t* idx, int i) const { return row_at(idx, i); }
  ActorHead head(const float* mean, const float* log_std, const float* a, int32_t, float adv_n, const Config& c, float inv_m) const {
    return a2c_actor_head(mean, log_std, a, adv_n, c, inv_m);
  }
};

struct HostA2C : HostLearner {
  using HostLearner::HostLearner;

  // brs_a2c_grad: BRS_OK or BRS_ERR_ARG
  int grad(const float* params, int n_rows, const float* obs, const float* act, const float* adv, const float* ret, const int32_t* idx, int m,
           const brs_a2c_config* cfg, float* grad_out) {
    if (!cfg || m < 1 || (cfg->normalize_adv && m < 2) || (!idx && m > n_rows) || !(cfg->ret_scale > 0.0f) || n_rows <= 0) return BRS_ERR_ARG;
    grad_kernels(A2cFamily{}, params, n_rows, obs, act, adv, ret, idx, m, *cfg, grad_out);
    return BRS_OK;
  }

  // brs_a2c_apply / learner_rmsprop_apply_kernel
  int apply(float* params, const float* grad_in, float* sq, const brs_a2c_config* cfg) {
    if (!cfg || !params || !grad_in || !sq) return BRS_ERR_ARG;
    const brs_ppo_config clip_cfg = shared_fields(*cfg);
    float norm_pi, norm_vf;
    grad_norms(grad_in, clip_cfg, norm_pi, norm_vf);
    info.steps += 1;
    for (int k = 0; k < NSTAT; k++) info.stat[k] = grad_in[NPARAM + k];
    info.grad_norm_pi = norm_pi; info.grad_norm_vf = norm_vf;
    const RmspropScalars r = rmsprop_scalars(*cfg);
    for (int i = 0; i < NPARAM; i++) rmsprop_tf_update(params[i], sq[i], grad_in[i] * param_scale(i, norm_pi, norm_vf, clip_cfg), r);
    return BRS_OK;
  }
};

}  // namespace a2chost
