// The host build of offpolicyhost.hpp behind a C interface, for ctypes (tests/offpolicy_cases.py builds this with g++).
#include "offpolicyhost.hpp"

extern "C" {

int oh_act(const float* actor, int n, const float* obs, uint64_t seed, int64_t base, uint32_t step, float sigma, int random, float* action,
           float* mean, float* noise) {
  return offpolicyhost::act(actor, n, obs, seed, base, step, sigma, random, action, mean, noise);
}
int oh_q(const float* critic, int n, const float* obs, const float* action, float* out) { return offpolicyhost::q(critic, n, obs, action, out); }
int oh_td_target(const float* actor_t, const float* critic_t, int m, const float* next_obs, const float* reward, const uint8_t* done, float gamma,
                 float* y) {
  return offpolicyhost::td_target(actor_t, critic_t, m, next_obs, reward, done, gamma, y);
}
int oh_replay_add(const brs_replay_storage* s, int n, int cap, int pos, const float* last_obs, const float* action, const float* obs,
                  const float* reward, const uint8_t* term, const uint8_t* trunc, const float* tobs) {
  return offpolicyhost::replay_add(s, n, cap, pos, last_obs, action, obs, reward, term, trunc, tobs);
}
int oh_replay_sample(const brs_replay_storage* s, int n, int cap, int size, int m, uint64_t seed, uint32_t draw, const brs_replay_storage* out,
                     int32_t* idx) {
  return offpolicyhost::replay_sample(s, n, cap, size, m, seed, draw, out, idx);
}

}  // extern "C"
