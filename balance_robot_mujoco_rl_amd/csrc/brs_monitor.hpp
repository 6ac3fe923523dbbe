// brs_monitor.hpp -- the episode monitor of include/brs_policy.h, the part shared by the HIP kernels
// (brs_monitor.hip) and the host build the CPU tests compare with the numpy restatement (tests/monitorhost): the columns a
// monitor owns, the per-env transition of one env step, and the partial sums and the combine step of the reduction.
#pragma once
#include <stdint.h>

#include "../../include/brs.h"
#include "../../include/brs_policy.h"

#ifndef BRS_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BRS_HD __host__ __device__ __forceinline__
#else
#define BRS_HD inline
#endif
#endif

namespace brs {
namespace monitor {

constexpr int REDUCE_THREADS = 1024;  // partial p folds envs p, p + 1024, ... in ascending order; then a tree of fixed pairing

// Struct of arrays, one entry per env unless noted.  All of it is zero after a reset except target (-1 without targets).
struct Columns {
  // running episode
  double* ep_ret;
  int32_t* ep_len;
  // episodes that ended
  int32_t* ended;    // all of them
  int32_t* counted;  // those that count
  int32_t* target;   // < 0: every episode counts
  int32_t* base;     // first log row of the env: exclusive prefix sum of the targets
  double *sum_ret, *sum_ret2, *min_ret, *max_ret;
  int64_t *sum_len, *sum_len2;
  int32_t *min_len, *max_len;
  int32_t *n_terminated, *n_time_limit;
  // episode log, one entry per row (log_capacity rows)
  int32_t* log_env;
  double* log_ret;
  int32_t* log_len;
  uint8_t* log_time_limit;
};

// what the caller still has to do for the env after transition(): the histogram bin and `pending`
struct Outcome {
  int32_t bin;   // > 0 or 0 ("longer than max_len"): add one to this bin; -1: nothing to add
  bool reached;  // this episode brought counted[i] up to target[i]
};

// One env step of env i (section 7.3, "per env i, on every update" and "on done").  The common path touches ep_ret and
// ep_len only.
BRS_HD Outcome transition(const Columns& c, int i, float reward, uint8_t terminated, uint8_t truncated, int32_t hist_max_len) {
#if defined(__clang__)
#pragma clang fp contract(off)  // sum_ret2 += ret * ret is a product and a sum, on the device as on the host
#endif
  Outcome out = {-1, false};
  const double ret = c.ep_ret[i] + (double)reward;
  const int32_t len = c.ep_len[i] + 1;
  if (!(terminated | truncated)) {
    c.ep_ret[i] = ret;
    c.ep_len[i] = len;
    return out;
  }
  c.ep_ret[i] = 0.0;
  c.ep_len[i] = 0;
  c.ended[i] += 1;
  const int32_t target = c.target[i], k = c.counted[i];
  if (target >= 0 && k >= target) return out;
  c.counted[i] = k + 1;
  const double sq = ret * ret;
  c.sum_ret[i] += ret;
  c.sum_ret2[i] += sq;
  c.sum_len[i] += (int64_t)len;
  c.sum_len2[i] += (int64_t)len * (int64_t)len;
  if (k == 0) {
    c.min_ret[i] = ret; c.max_ret[i] = ret;
    c.min_len[i] = len; c.max_len[i] = len;
  } else {
    if (ret < c.min_ret[i]) c.min_ret[i] = ret;
    if (ret > c.max_ret[i]) c.max_ret[i] = ret;
    if (len < c.min_len[i]) c.min_len[i] = len;
    if (len > c.max_len[i]) c.max_len[i] = len;
  }
  const bool time_limit = truncated != 0 && terminated == 0;
  if (terminated != 0) c.n_terminated[i] += 1;
  if (time_limit) c.n_time_limit[i] += 1;
  if (target >= 0) {  // k < target: row base + k lies inside this env's share of the log
    const int64_t row = (int64_t)c.base[i] + k;
    c.log_env[row] = i;
    c.log_ret[row] = ret;
    c.log_len[row] = len;
    c.log_time_limit[row] = time_limit ? 1 : 0;
    out.reached = k + 1 == target;
  }
  out.bin = len <= hist_max_len ? len : 0;
  return out;
}

// The reduction of brs_monitor_stats: the sums of a set of envs.  `pending` and `steps` are not per env and are filled in
// by the caller.
struct Partial {
  int64_t episodes, ended, terminated, time_limit, sum_len, sum_len2;
  double sum_ret, sum_ret2, min_ret, max_ret, running_ret;
  int32_t min_len, max_len, first_running, pad;
};

BRS_HD Partial empty_partial() { return Partial{0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0}; }

// a += b; the order of the operands matters for the floating-point sums, so the callers fix it
BRS_HD void combine(Partial& a, const Partial& b) {
  if (b.episodes > 0) {
    if (a.episodes == 0) {
      a.min_ret = b.min_ret; a.max_ret = b.max_ret; a.min_len = b.min_len; a.max_len = b.max_len;
    } else {
      if (b.min_ret < a.min_ret) a.min_ret = b.min_ret;
      if (b.max_ret > a.max_ret) a.max_ret = b.max_ret;
      if (b.min_len < a.min_len) a.min_len = b.min_len;
      if (b.max_len > a.max_len) a.max_len = b.max_len;
    }
  }
  a.episodes += b.episodes; a.ended += b.ended; a.terminated += b.terminated; a.time_limit += b.time_limit;
  a.sum_len += b.sum_len; a.sum_len2 += b.sum_len2;
  a.sum_ret += b.sum_ret; a.sum_ret2 += b.sum_ret2; a.running_ret += b.running_ret;
  a.first_running += b.first_running;
}

BRS_HD Partial env_partial(const Columns& c, int i) {
  Partial p = empty_partial();
  p.episodes = c.counted[i]; p.ended = c.ended[i]; p.terminated = c.n_terminated[i]; p.time_limit = c.n_time_limit[i];
  p.sum_len = c.sum_len[i]; p.sum_len2 = c.sum_len2[i];
  p.sum_ret = c.sum_ret[i]; p.sum_ret2 = c.sum_ret2[i]; p.min_ret = c.min_ret[i]; p.max_ret = c.max_ret[i];
  p.running_ret = c.ep_ret[i];
  p.min_len = c.min_len[i]; p.max_len = c.max_len[i];
  p.first_running = c.ended[i] == 0 ? 1 : 0;
  return p;
}

// partial t of REDUCE_THREADS: envs t, t + REDUCE_THREADS, ... in ascending order
BRS_HD Partial fold_envs(const Columns& c, int n, int t) {
  Partial p = empty_partial();
  for (int i = t; i < n; i += REDUCE_THREADS) combine(p, env_partial(c, i));
  return p;
}

BRS_HD void to_stats(const Partial& p, int32_t pending, int64_t steps, brs_episode_stats* s) {
  s->episodes = p.episodes; s->ended = p.ended; s->terminated = p.terminated; s->time_limit = p.time_limit;
  s->sum_len = p.sum_len; s->sum_len2 = p.sum_len2; s->steps = steps;
  s->sum_ret = p.sum_ret; s->sum_ret2 = p.sum_ret2; s->min_ret = p.min_ret; s->max_ret = p.max_ret; s->running_ret = p.running_ret;
  s->min_len = p.min_len; s->max_len = p.max_len; s->first_running = p.first_running; s->pending = pending;
}

}  // namespace monitor
}  // namespace brs
