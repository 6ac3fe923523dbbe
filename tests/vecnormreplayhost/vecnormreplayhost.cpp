// The host build of the normalising replay sample behind a C interface, for ctypes (tests/vecnorm_replay_cases.py builds this
// with g++).  The handle is a HostVecNorm of tests/vecnormhost: vh_create / vh_set_stats / vh_destroy are restated here so that
// one library serves a test.
#include "vecnormreplayhost.hpp"

using vecnormhost::HostVecNorm;

extern "C" {

void* vrh_create(int n, const brs_vecnorm_config* cfg) { return new HostVecNorm(n, *cfg); }
void vrh_destroy(void* h) { delete (HostVecNorm*)h; }
void vrh_set_stats(void* h, const double* in) { memcpy(((HostVecNorm*)h)->stats, in, sizeof(double) * brs::vecnorm::NSTAT); }
int vrh_replay_sample(void* h, const brs_replay_storage* s, int n, int cap, int size, int m, uint64_t seed, uint32_t draw,
                      const brs_replay_storage* out, int32_t* idx) {
  return vecnormreplayhost::replay_sample(*(HostVecNorm*)h, *s, n, cap, size, m, seed, draw, *out, idx, nullptr);
}

}  // extern "C"
