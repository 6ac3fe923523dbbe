// Host build of the episode monitor's kernel source (balance_robot_mujoco_rl_amd/csrc/brs_monitor.hpp): the per-env
// transition and the reduction of brs_monitor_stats on host arrays, with the host side of brs_monitor.hip (reset, the
// histogram and `pending`) restated in the plainest form.  Shared by monitorhost.cpp (a library for tests/test_monitor_cpu.py)
// and monitorhost_main.cpp (a program of its own, for the sanitizers).
#pragma once
#include <string.h>

#include <vector>

#include "brs_monitor.hpp"

namespace monitorhost {

struct HostMonitor {
  int n, max_len, log_capacity;
  std::vector<double> ep_ret, sum_ret, sum_ret2, min_ret, max_ret, log_ret;
  std::vector<int32_t> ep_len, ended, counted, target, base, min_len, longest, n_terminated, n_time_limit, log_env, log_len;
  std::vector<int64_t> sum_len, sum_len2, hist;
  std::vector<uint8_t> log_time_limit;
  int32_t pending = 0;
  int64_t steps = 0, rows = 0;

  HostMonitor(int n_, int max_len_, int cap) : n(n_), max_len(max_len_), log_capacity(cap) { reset(nullptr); }

  brs::monitor::Columns columns() {
    brs::monitor::Columns c;
    c.ep_ret = ep_ret.data(); c.ep_len = ep_len.data(); c.ended = ended.data(); c.counted = counted.data(); c.target = target.data();
    c.base = base.data(); c.sum_ret = sum_ret.data(); c.sum_ret2 = sum_ret2.data(); c.min_ret = min_ret.data(); c.max_ret = max_ret.data();
    c.sum_len = sum_len.data(); c.sum_len2 = sum_len2.data(); c.min_len = min_len.data(); c.max_len = longest.data();
    c.n_terminated = n_terminated.data(); c.n_time_limit = n_time_limit.data(); c.log_env = log_env.data(); c.log_ret = log_ret.data();
    c.log_len = log_len.data(); c.log_time_limit = log_time_limit.data();
    return c;
  }

  // brs_monitor_reset: 0, or -1 for a negative target or a sum above the capacity
  int reset(const int32_t* targets) {
    int64_t sum = 0;
    if (targets)
      for (int i = 0; i < n; i++) {
        if (targets[i] < 0) return -1;
        sum += targets[i];
      }
    if (sum > log_capacity) return -1;
    const size_t N = (size_t)n, R = (size_t)log_capacity;
    for (auto* v : {&ep_ret, &sum_ret, &sum_ret2, &min_ret, &max_ret}) v->assign(N, 0.0);
    for (auto* v : {&ep_len, &ended, &counted, &base, &min_len, &longest, &n_terminated, &n_time_limit}) v->assign(N, 0);
    for (auto* v : {&sum_len, &sum_len2}) v->assign(N, 0);
    target.assign(N, -1);
    hist.assign((size_t)max_len + 1, 0);
    log_ret.assign(R, 0.0); log_env.assign(R, 0); log_len.assign(R, 0); log_time_limit.assign(R, 0);
    pending = n; steps = 0; rows = sum;
    if (targets) {
      pending = 0;
      int32_t b = 0;
      for (int i = 0; i < n; i++) { target[i] = targets[i]; base[i] = b; b += targets[i]; pending += targets[i] > 0; }
    }
    return 0;
  }

  void update(const float* reward, const uint8_t* terminated, const uint8_t* truncated) {
    const brs::monitor::Columns c = columns();
    for (int i = 0; i < n; i++) {
      const brs::monitor::Outcome o = brs::monitor::transition(c, i, reward[i], terminated[i], truncated[i], max_len);
      if (o.bin >= 0) hist[(size_t)o.bin] += 1;
      if (o.reached) pending -= 1;
    }
    steps += 1;
  }

  // monitor_reduce_kernel: the same partials and the same pairing
  void stats(brs_episode_stats* out) {
    const brs::monitor::Columns c = columns();
    std::vector<brs::monitor::Partial> p((size_t)brs::monitor::REDUCE_THREADS);
    for (int t = 0; t < brs::monitor::REDUCE_THREADS; t++) p[(size_t)t] = brs::monitor::fold_envs(c, n, t);
    for (int s = brs::monitor::REDUCE_THREADS / 2; s >= 1; s >>= 1)
      for (int t = 0; t < s; t++) brs::monitor::combine(p[(size_t)t], p[(size_t)(t + s)]);
    memset(out, 0, sizeof(*out));
    brs::monitor::to_stats(p[0], pending, steps, out);
  }
};

}  // namespace monitorhost
