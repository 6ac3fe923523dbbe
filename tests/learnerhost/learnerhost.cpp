// The host learner of learnerhost.hpp behind a C interface, for ctypes (tests/test_learner_cpu.py builds this with g++).
#include "learnerhost.hpp"

using learnerhost::HostLearner;

extern "C" {

void* lh_create(int max_workgroups) { return new HostLearner(max_workgroups); }
void lh_destroy(void* h) { delete (HostLearner*)h; }
void lh_begin_iteration(void* h) { ((HostLearner*)h)->begin_iteration(); }
int lh_grad(void* h, const float* params, int n_rows, const float* obs, const float* act, const float* logp_old, const float* adv,
            const float* ret, const int32_t* idx, int m, const brs_ppo_config* cfg, float* grad) {
  return ((HostLearner*)h)->grad(params, n_rows, obs, act, logp_old, adv, ret, idx, m, cfg, grad);
}
int lh_apply(void* h, float* params, const float* grad, float* m, float* v, const brs_ppo_config* cfg) {
  return ((HostLearner*)h)->apply(params, grad, m, v, cfg);
}
void lh_stats(void* h, brs_learner_info* out) { *out = ((HostLearner*)h)->info; }

}  // extern "C"
