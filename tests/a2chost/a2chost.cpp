// The host A2C learner of a2chost.hpp behind a C interface, for ctypes (tests/a2c_cases.py builds this with g++).
#include "a2chost.hpp"

using a2chost::HostA2C;

extern "C" {

void* ah_create(int max_workgroups) { return new HostA2C(max_workgroups); }
void ah_destroy(void* h) { delete (HostA2C*)h; }
int ah_grad(void* h, const float* params, int n_rows, const float* obs, const float* act, const float* adv, const float* ret,
            const int32_t* idx, int m, const brs_a2c_config* cfg, float* grad) {
  return ((HostA2C*)h)->grad(params, n_rows, obs, act, adv, ret, idx, m, cfg, grad);
}
int ah_apply(void* h, float* params, const float* grad, float* sq, const brs_a2c_config* cfg) {
  return ((HostA2C*)h)->apply(params, grad, sq, cfg);
}
void ah_stats(void* h, brs_learner_info* out) { *out = ((HostA2C*)h)->info; }
// the optimiser's update alone, on n elements
void ah_rmsprop(float* p, float* sq, const float* g, int n, const brs_a2c_config* cfg) {
  const brs::learner::RmspropScalars r = brs::learner::rmsprop_scalars(*cfg);
  for (int i = 0; i < n; i++) brs::learner::rmsprop_tf_update(p[i], sq[i], g[i], r);
}

}  // extern "C"
