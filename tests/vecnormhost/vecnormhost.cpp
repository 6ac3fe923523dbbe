// The host VecNormalize of vecnormhost.hpp behind a C interface, for ctypes (tests/vecnorm_cases.py builds this with g++).
#include "vecnormhost.hpp"

using vecnormhost::HostVecNorm;

extern "C" {

void* vh_create(int n, const brs_vecnorm_config* cfg) { return new HostVecNorm(n, *cfg); }
void vh_destroy(void* h) { delete (HostVecNorm*)h; }
void vh_reset(void* h, const float* obs, int training, float* obs_out) { ((HostVecNorm*)h)->reset(obs, training != 0, obs_out); }
void vh_step(void* h, const float* obs, const float* reward, const uint8_t* terminated, const uint8_t* truncated, const float* terminal_obs,
             int training, float* obs_out, float* reward_out, float* terminal_obs_out) {
  ((HostVecNorm*)h)->step(obs, reward, terminated, truncated, terminal_obs, training != 0, obs_out, reward_out, terminal_obs_out);
}
void vh_normalize_obs(void* h, int m, const float* in, float* out) { ((HostVecNorm*)h)->normalize_obs(m, in, out); }
void vh_normalize_reward(void* h, int m, const float* in, float* out) { ((HostVecNorm*)h)->normalize_reward(m, in, out); }
void vh_get_stats(void* h, double* out) { memcpy(out, ((HostVecNorm*)h)->stats, sizeof(double) * brs::vecnorm::NSTAT); }
void vh_set_stats(void* h, const double* in) { memcpy(((HostVecNorm*)h)->stats, in, sizeof(double) * brs::vecnorm::NSTAT); }
void vh_get_returns(void* h, double* out) {
  HostVecNorm* v = (HostVecNorm*)h;
  memcpy(out, v->returns.data(), sizeof(double) * (size_t)v->n);
}

}  // extern "C"
