// Host build of the DDPG learner's kernel source (balance_robot_mujoco_rl_amd/csrc/brs_ddpg_learner.hpp): the loss heads, the
// tanh' factor, the gate rule, the statistics, Adam plus Polyak and the plain-loop forward/backward on host arrays, behind the
// argument rules of the C ABI (include/brs_policy.h: brs_ddpg_learner_*).  Shared by ddpglearnerhost.cpp (a library for
// tests/test_ddpg_learner_cpu.py) and ddpglearnerhost_main.cpp (a program of its own, for the sanitizers).
#pragma once
#include <stddef.h>

#include "brs_ddpg_learner.hpp"

namespace ddpglearnerhost {

using namespace brs::ddpg_learner;

inline int critic_grad(const float* critic, int m, const float* obs, const float* act, const float* y, float* grad) {
  if (!critic || !obs || !act || !y || !grad || m < 1) return BRS_ERR_ARG;
  critic_grad_host(critic, m, obs, act, y, grad);
  return BRS_OK;
}

inline int actor_grad(const float* actor, const float* critic, int m, const float* obs, float* grad) {
  if (!actor || !critic || !obs || !grad || m < 1) return BRS_ERR_ARG;
  actor_grad_host(actor, critic, m, obs, grad);
  return BRS_OK;
}

inline int apply(int n_param, float* params, const float* grad, float* m, float* v, float* target, const brs_adam_config* cfg, int64_t step,
                 float tau) {
  if (apply_argument_error(n_param, params, grad, m, v, cfg, step, tau)) return BRS_ERR_ARG;
  apply_host(n_param, params, grad, m, v, target, *cfg, step, tau);
  return BRS_OK;
}

}  // namespace ddpglearnerhost
