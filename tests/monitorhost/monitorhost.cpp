// The host monitor of monitorhost.hpp behind a C interface, for ctypes (tests/test_monitor_cpu.py builds this with g++).
#include "monitorhost.hpp"

using monitorhost::HostMonitor;

extern "C" {

void* mh_create(int n, int max_len, int log_capacity) { return new HostMonitor(n, max_len, log_capacity); }
void mh_destroy(void* h) { delete (HostMonitor*)h; }
int mh_reset(void* h, const int32_t* targets) { return ((HostMonitor*)h)->reset(targets); }
void mh_update(void* h, const float* reward, const uint8_t* terminated, const uint8_t* truncated) {
  ((HostMonitor*)h)->update(reward, terminated, truncated);
}
void mh_stats(void* h, brs_episode_stats* out) { ((HostMonitor*)h)->stats(out); }
void mh_histogram(void* h, int64_t* hist) {
  HostMonitor* m = (HostMonitor*)h;
  memcpy(hist, m->hist.data(), m->hist.size() * sizeof(int64_t));
}
void mh_episodes(void* h, int32_t* env, double* ret, int32_t* len, uint8_t* time_limit) {
  HostMonitor* m = (HostMonitor*)h;
  const size_t R = (size_t)m->rows;
  if (R == 0) return;
  memcpy(env, m->log_env.data(), R * sizeof(int32_t)); memcpy(ret, m->log_ret.data(), R * sizeof(double));
  memcpy(len, m->log_len.data(), R * sizeof(int32_t)); memcpy(time_limit, m->log_time_limit.data(), R);
}

}  // extern "C"
