// The host build of ddpglearnerhost.hpp behind a C interface, for ctypes (tests/ddpg_learner_cases.py builds this with g++).
#include "ddpglearnerhost.hpp"

extern "C" {

int dh_critic_grad(const float* critic, int m, const float* obs, const float* act, const float* y, float* grad) {
  return ddpglearnerhost::critic_grad(critic, m, obs, act, y, grad);
}
int dh_actor_grad(const float* actor, const float* critic, int m, const float* obs, float* grad) {
  return ddpglearnerhost::actor_grad(actor, critic, m, obs, grad);
}
int dh_apply(int n_param, float* params, const float* grad, float* m, float* v, float* target, const brs_adam_config* cfg, int64_t step, float tau) {
  return ddpglearnerhost::apply(n_param, params, grad, m, v, target, cfg, step, tau);
}

void dh_sample_split(int m, int* out) { ddpglearnerhost::split_of(m, out); }
long long dh_split_sweep(int m_lo, int m_hi, int* first_bad, unsigned* first_mask) {
  return ddpglearnerhost::split_sweep(m_lo, m_hi, first_bad, first_mask);
}

// the two statements of Adam's element update side by side: brs_learner.hpp's adam_update (the PPO learner's) and apply_element
// (this learner's, contraction off).  Under g++ neither fuses, so the test holds them to the same bytes: the copies cannot drift.
void dh_adam_pair(int n, const float* grad, const brs_adam_config* cfg, int64_t step, float* p_a, float* m_a, float* v_a, float* p_b, float* m_b,
                  float* v_b) {
  const brs::learner::AdamScalars a = brs::ddpg_learner::adam_scalars(*cfg, step);
  for (int i = 0; i < n; i++) {
    brs::learner::adam_update(p_a[i], m_a[i], v_a[i], grad[i], a);
    brs::ddpg_learner::apply_element(p_b[i], m_b[i], v_b[i], grad[i], a);
  }
}

}  // extern "C"
