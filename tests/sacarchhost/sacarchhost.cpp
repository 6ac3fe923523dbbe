// The host build of sacarchhost.hpp behind tests/sachost/sachost.cpp's C interface (the same names and signatures, so that the helpers
// of tests/sac_cases.py drive either), for ctypes (tests/sac_arch_cases.py builds this with g++).
#include "sacarchhost.hpp"

using sacarchhost::H;

extern "C" {

int sh_arch(void) { return H::Arch::ID; }
int sh_sizes(int* nactor, int* ncritic) { *nactor = H::NA; *ncritic = H::NC; return 0; }
int sh_act(const float* actor, int n, const float* obs, uint64_t seed, int64_t base, uint32_t step, int deterministic, int random, float* action,
           float* mu, float* log_std, float* z) {
  return H::act(actor, n, obs, seed, base, step, deterministic, random, action, mu, log_std, z);
}
int sh_target(const float* actor, const float* critics_t, int m, const float* next_obs, const float* reward, const uint8_t* done, float gamma,
              uint64_t seed, uint32_t draw, float* y, float* next_action, float* logp, float* z) {
  return H::target(actor, critics_t, m, next_obs, reward, done, gamma, seed, draw, y, next_action, logp, z);
}
int sh_twin_critic_grad(const float* critics, int m, const float* obs, const float* act, const float* y, float loss_scale, float* grad) {
  return H::twin_critic_grad(critics, m, obs, act, y, loss_scale, grad);
}
int sh_actor_grad(const float* actor, const float* critics, int m, const float* obs, uint64_t seed, uint32_t draw, int learn_alpha,
                  float target_entropy, float* grad, float* dz3) {
  return H::actor_grad(actor, critics, m, obs, seed, draw, learn_alpha, target_entropy, grad, dz3);
}
int sh_apply(int n_param, float* params, const float* grad, float* m, float* v, float* target, const brs_adam_config* cfg, int64_t step, float tau) {
  return ddpglearnerhost::apply(n_param, params, grad, m, v, target, cfg, step, tau);
}
int sh_td3_combine(int m, const float* reward, const uint8_t* done, float gamma, const float* q0, const float* q1, float* y) {
  for (int i = 0; i < m; i++) y[i] = brs::offpolicy::td3_combine(reward[i], done[i], gamma, q0[i], q1[i]);
  return 0;
}
int sh_q(const float* critic, int n, const float* obs, const float* act, float* q) { return H::q(critic, n, obs, act, q); }
// the argument texts of the C ABI (0: accepted); which: 0 act, 1 target, 2 critic gradient, 3 actor gradient
const char* sh_argument_error(int which, const void* a, const void* b, int n, const void* c, const void* d, const void* e, float f, const void* g,
                              int flag) {
  switch (which) {
    case 0: return brs::sac::sac_act_argument_error(a, n, c, flag, g);
    case 1: return brs::sac::sac_target_argument_error(a, b, n, c, d, e, f, g);
    case 2: return brs::sac::sac_critic_grad_argument_error(a, n, c, d, e, g);
    default: return brs::sac::sac_actor_grad_argument_error(a, b, n, c, f, g);
  }
}
int sh_known_arch(int arch) { return brs::sac::known_arch(arch) ? 1 : 0; }

}  // extern "C"
