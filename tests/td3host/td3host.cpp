// The host build of td3host.hpp behind a C interface, for ctypes (tests/td3_cases.py builds this with g++).
#include "td3host.hpp"

extern "C" {

int th_td3_target(const float* actor_t, const float* critics_t, int m, const float* next_obs, const float* reward, const uint8_t* done, float gamma,
                  float policy_noise, float noise_clip, uint64_t seed, uint32_t draw, float* y, float* next_action, float* noise) {
  return td3host::td3_target(actor_t, critics_t, m, next_obs, reward, done, gamma, policy_noise, noise_clip, seed, draw, y, next_action, noise);
}
int th_twin_critic_grad(const float* critics, int m, const float* obs, const float* act, const float* y, float* grad) {
  return td3host::twin_critic_grad(critics, m, obs, act, y, grad);
}
// the single-network entry points of the two host builds this one stands on, so that one library serves a whole TD3 chain
int th_td_target(const float* actor_t, const float* critic_t, int m, const float* next_obs, const float* reward, const uint8_t* done, float gamma,
                 float* y) {
  return offpolicyhost::td_target(actor_t, critic_t, m, next_obs, reward, done, gamma, y);
}
int th_critic_grad(const float* critic, int m, const float* obs, const float* act, const float* y, float* grad) {
  return ddpglearnerhost::critic_grad(critic, m, obs, act, y, grad);
}
int th_actor_grad(const float* actor, const float* critic, int m, const float* obs, float* grad) {
  return ddpglearnerhost::actor_grad(actor, critic, m, obs, grad);
}
int th_apply(int n_param, float* params, const float* grad, float* m, float* v, float* target, const brs_adam_config* cfg, int64_t step, float tau) {
  return ddpglearnerhost::apply(n_param, params, grad, m, v, target, cfg, step, tau);
}

}  // extern "C"
