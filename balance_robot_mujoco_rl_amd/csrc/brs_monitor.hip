// brs_monitor.hip -- the episode monitor of include/brs_policy.h as HIP kernels for gfx950: what the reference
// gets from SB3's Monitor wrapper and evaluate_policy (src/sb_rl.py:501, :536-543), for all envs next to brs_step.
//
//   monitor_update_kernel  one lane per env.  A lane whose env goes on reads 6 bytes and read-modify-writes ep_ret and ep_len;
//                          everything else is touched by the lanes whose episode ended (brs_monitor.hpp: transition).  The
//                          histogram takes one integer atomic per DISTINCT length among a wave's finished episodes (with a
//                          time limit most of them end on the same step with the same length), `pending` at most one per wave.
//                          No LDS, no barrier, no floating-point atomic.
//   monitor_reduce_kernel  one workgroup of 1,024: thread t folds envs t, t + 1024, ... in ascending order, then a tree over LDS
//                          with fixed pairing (t takes t + s for s = 512, 256, ... 1), so that the fp64 sums come out the same
//                          bytes on every run.
#include <hip/hip_runtime.h>

#include <string>

#include "brs_host.hpp"
#include "brs_monitor.hpp"

namespace {

using namespace brs::monitor;

constexpr int UPDATE_THREADS = 256;

__global__ void __launch_bounds__(UPDATE_THREADS) monitor_update_kernel(const Columns c, const int n, const int hist_max_len,
                                                                        const float* __restrict__ reward, const uint8_t* __restrict__ terminated,
                                                                        const uint8_t* __restrict__ truncated,
                                                                        unsigned long long* __restrict__ hist, int32_t* __restrict__ pending) {
  const int i = blockIdx.x * UPDATE_THREADS + threadIdx.x;
  Outcome o = {-1, false};
  if (i < n) o = transition(c, i, reward[i], terminated[i], truncated[i], hist_max_len);

  // histogram: group the wave's counted episodes by bin, one atomic per group
  const int lane = threadIdx.x & 63;
  bool todo = o.bin >= 0;
  unsigned long long rest = __ballot(todo);
  while (rest) {  // wave-uniform: `rest` is a ballot
    const int leader = __ffsll(rest) - 1;
    const int bin = __builtin_amdgcn_readlane(o.bin, leader);
    const unsigned long long same = __ballot(todo && o.bin == bin);
    if (lane == leader) atomicAdd(&hist[bin], (unsigned long long)__popcll(same));
    todo = todo && o.bin != bin;
    rest &= ~same;
  }
  const unsigned long long reached = __ballot(o.reached);
  if (reached && lane == __ffsll(reached) - 1) atomicSub(pending, __popcll(reached));
}

__global__ void __launch_bounds__(REDUCE_THREADS) monitor_reduce_kernel(const Columns c, const int n, const int32_t* __restrict__ pending,
                                                                        brs_episode_stats* __restrict__ out) {
  __shared__ Partial lds[REDUCE_THREADS / 2];
  const int t = threadIdx.x;
  Partial p = fold_envs(c, n, t);
  for (int s = REDUCE_THREADS / 2; s >= 1; s >>= 1) {  // p[t] += p[t + s], the upper half handing over through LDS
    if (t >= s && t < 2 * s) lds[t - s] = p;
    __syncthreads();
    if (t < s) combine(p, lds[t]);
    __syncthreads();
  }
  if (t == 0) to_stats(p, *pending, 0, out);  // steps: the host counts the update calls
}

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

struct brs_monitor {
  int device = 0, n = 0, max_len = 0, log_capacity = 0;
  char* block = nullptr;       // every column, the histogram, pending and the stats slot: one allocation, one memset at reset
  size_t block_bytes = 0;
  brs::monitor::Columns cols{};
  unsigned long long* hist = nullptr;
  int32_t* pending = nullptr;
  brs_episode_stats* stats_dev = nullptr;
  int32_t* staging = nullptr;  // pinned: targets[n], base[n], pending
  int64_t steps = 0, log_rows = 0;
  std::string err;
};

using brs::host::DeviceGuard, brs::host::fail;

extern "C" {

int brs_monitor_create(int32_t device, int32_t n, int32_t max_len, int32_t log_capacity, brs_monitor** out) {
  if (!out) return fail<brs_monitor>(nullptr, BRS_ERR_ARG, "brs_monitor_create: null argument");
  *out = nullptr;
  if (n <= 0) return fail<brs_monitor>(nullptr, BRS_ERR_ARG, "brs_monitor_create: n must be positive");
  if (max_len <= 0) return fail<brs_monitor>(nullptr, BRS_ERR_ARG, "brs_monitor_create: max_len must be positive");
  if (log_capacity < 0) return fail<brs_monitor>(nullptr, BRS_ERR_ARG, "brs_monitor_create: log_capacity must not be negative");
  std::string why;
  if (const int rc = brs::host::check_device(device, "brs_monitor_create", &why)) return fail<brs_monitor>(nullptr, rc, why);
  brs_monitor* m = new brs_monitor();
  m->device = device; m->n = n; m->max_len = max_len; m->log_capacity = log_capacity;
  // carve the block: every piece starts on a 256-byte boundary
  size_t off = 0;
  auto take = [&off](size_t bytes) { const size_t at = off; off += align_up(bytes); return at; };
  const size_t N = (size_t)n, R = (size_t)log_capacity;
  const size_t o_ep_ret = take(8 * N), o_ep_len = take(4 * N), o_ended = take(4 * N), o_counted = take(4 * N), o_target = take(4 * N),
               o_base = take(4 * N), o_sum_ret = take(8 * N), o_sum_ret2 = take(8 * N), o_min_ret = take(8 * N), o_max_ret = take(8 * N),
               o_sum_len = take(8 * N), o_sum_len2 = take(8 * N), o_min_len = take(4 * N), o_max_len = take(4 * N), o_nterm = take(4 * N),
               o_ntl = take(4 * N), o_log_env = take(4 * R), o_log_ret = take(8 * R), o_log_len = take(4 * R), o_log_tl = take(R),
               o_hist = take(8 * ((size_t)max_len + 1)), o_pending = take(4), o_stats = take(sizeof(brs_episode_stats));
  m->block_bytes = off;
  DeviceGuard g(device);
  if (!g.ok || hipMalloc((void**)&m->block, m->block_bytes) != hipSuccess ||
      hipHostMalloc((void**)&m->staging, (2 * N + 1) * sizeof(int32_t)) != hipSuccess) {
    if (m->block) (void)hipFree(m->block);
    delete m;
    return fail<brs_monitor>(nullptr, BRS_ERR_HIP, "brs_monitor_create: device allocation failed");
  }
  char* b = m->block;
  brs::monitor::Columns& c = m->cols;
  c.ep_ret = (double*)(b + o_ep_ret); c.ep_len = (int32_t*)(b + o_ep_len); c.ended = (int32_t*)(b + o_ended);
  c.counted = (int32_t*)(b + o_counted); c.target = (int32_t*)(b + o_target); c.base = (int32_t*)(b + o_base);
  c.sum_ret = (double*)(b + o_sum_ret); c.sum_ret2 = (double*)(b + o_sum_ret2); c.min_ret = (double*)(b + o_min_ret);
  c.max_ret = (double*)(b + o_max_ret); c.sum_len = (int64_t*)(b + o_sum_len); c.sum_len2 = (int64_t*)(b + o_sum_len2);
  c.min_len = (int32_t*)(b + o_min_len); c.max_len = (int32_t*)(b + o_max_len); c.n_terminated = (int32_t*)(b + o_nterm);
  c.n_time_limit = (int32_t*)(b + o_ntl); c.log_env = (int32_t*)(b + o_log_env); c.log_ret = (double*)(b + o_log_ret);
  c.log_len = (int32_t*)(b + o_log_len); c.log_time_limit = (uint8_t*)(b + o_log_tl);
  m->hist = (unsigned long long*)(b + o_hist); m->pending = (int32_t*)(b + o_pending); m->stats_dev = (brs_episode_stats*)(b + o_stats);
  *out = m;
  const int rc = brs_monitor_reset(m, nullptr, nullptr);  // a new monitor is a reset one, without targets
  if (rc != BRS_OK) {
    const std::string msg = m->err;
    *out = nullptr;
    (void)brs_monitor_destroy(m);
    return fail<brs_monitor>(nullptr, rc, msg);
  }
  return BRS_OK;
}

int brs_monitor_destroy(brs_monitor* m) {
  if (!m) return BRS_ERR_STATE;
  {
    DeviceGuard g(m->device);
    if (m->block) (void)hipFree(m->block);
    if (m->staging) (void)hipHostFree(m->staging);
  }
  delete m;
  return BRS_OK;
}

const char* brs_monitor_last_error(const brs_monitor* m) { return brs::host::last_error(m); }

int brs_monitor_reset(brs_monitor* m, const int32_t* targets_host, void* stream) {
  if (!m) return BRS_ERR_STATE;
  const size_t N = (size_t)m->n;
  int64_t rows = 0;
  int32_t waiting = m->n;
  if (targets_host) {
    waiting = 0;
    for (size_t i = 0; i < N; i++) {
      if (targets_host[i] < 0) return fail(m, BRS_ERR_ARG, "brs_monitor_reset: negative target");
      rows += targets_host[i];
      waiting += targets_host[i] > 0;
    }
    if (rows > m->log_capacity) return fail(m, BRS_ERR_ARG, "brs_monitor_reset: the targets add up to more than log_capacity");
  }
  DeviceGuard g(m->device);
  if (!g.ok) return fail(m, BRS_ERR_HIP, "brs_monitor_reset: hipSetDevice failed");
  hipStream_t s = (hipStream_t)stream;
  BRS_HIP_TRY(m, hipStreamSynchronize(s));  // an earlier reset's copy may still read the staging buffer
  BRS_HIP_TRY(m, hipMemsetAsync(m->block, 0, m->block_bytes, s));
  if (targets_host) {
    int32_t base = 0;
    for (size_t i = 0; i < N; i++) { m->staging[i] = targets_host[i]; m->staging[N + i] = base; base += targets_host[i]; }
    BRS_HIP_TRY(m, hipMemcpyAsync(m->cols.target, m->staging, N * sizeof(int32_t), hipMemcpyHostToDevice, s));
    BRS_HIP_TRY(m, hipMemcpyAsync(m->cols.base, m->staging + N, N * sizeof(int32_t), hipMemcpyHostToDevice, s));
  } else {
    BRS_HIP_TRY(m, hipMemsetAsync(m->cols.target, 0xff, N * sizeof(int32_t), s));  // -1: every episode counts
  }
  m->staging[2 * N] = waiting;
  BRS_HIP_TRY(m, hipMemcpyAsync(m->pending, m->staging + 2 * N, sizeof(int32_t), hipMemcpyHostToDevice, s));
  BRS_HIP_TRY(m, hipStreamSynchronize(s));
  m->steps = 0;
  m->log_rows = rows;
  return BRS_OK;
}

int brs_monitor_update(brs_monitor* m, const float* reward_dev, const uint8_t* terminated_dev, const uint8_t* truncated_dev, void* stream) {
  if (!m) return BRS_ERR_STATE;
  if (!reward_dev || !terminated_dev || !truncated_dev) return fail(m, BRS_ERR_ARG, "brs_monitor_update: null argument");
  DeviceGuard g(m->device);
  if (!g.ok) return fail(m, BRS_ERR_HIP, "brs_monitor_update: hipSetDevice failed");
  hipLaunchKernelGGL(monitor_update_kernel, dim3((m->n + UPDATE_THREADS - 1) / UPDATE_THREADS), dim3(UPDATE_THREADS), 0, (hipStream_t)stream,
                     m->cols, m->n, m->max_len, reward_dev, terminated_dev, truncated_dev, m->hist, m->pending);
  if (hipGetLastError() != hipSuccess) return fail(m, BRS_ERR_HIP, "brs_monitor_update: kernel launch failed");
  m->steps += 1;
  return BRS_OK;
}

int brs_monitor_stats(brs_monitor* m, brs_episode_stats* out_host, void* stream) {
  if (!m) return BRS_ERR_STATE;
  if (!out_host) return fail(m, BRS_ERR_ARG, "brs_monitor_stats: null argument");
  DeviceGuard g(m->device);
  if (!g.ok) return fail(m, BRS_ERR_HIP, "brs_monitor_stats: hipSetDevice failed");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(monitor_reduce_kernel, dim3(1), dim3(brs::monitor::REDUCE_THREADS), 0, s, m->cols, m->n, m->pending, m->stats_dev);
  if (hipGetLastError() != hipSuccess) return fail(m, BRS_ERR_HIP, "brs_monitor_stats: kernel launch failed");
  BRS_HIP_TRY(m, hipMemcpyAsync(out_host, m->stats_dev, sizeof(brs_episode_stats), hipMemcpyDeviceToHost, s));
  BRS_HIP_TRY(m, hipStreamSynchronize(s));
  out_host->steps = m->steps;
  return BRS_OK;
}

int brs_monitor_histogram(brs_monitor* m, int64_t* hist_host, void* stream) {
  if (!m) return BRS_ERR_STATE;
  if (!hist_host) return fail(m, BRS_ERR_ARG, "brs_monitor_histogram: null argument");
  DeviceGuard g(m->device);
  if (!g.ok) return fail(m, BRS_ERR_HIP, "brs_monitor_histogram: hipSetDevice failed");
  hipStream_t s = (hipStream_t)stream;
  BRS_HIP_TRY(m, hipMemcpyAsync(hist_host, m->hist, ((size_t)m->max_len + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  BRS_HIP_TRY(m, hipStreamSynchronize(s));
  return BRS_OK;
}

int brs_monitor_episodes(brs_monitor* m, int32_t* env_host, double* ret_host, int32_t* len_host, uint8_t* time_limit_host, void* stream) {
  if (!m) return BRS_ERR_STATE;
  if (!env_host || !ret_host || !len_host || !time_limit_host) return fail(m, BRS_ERR_ARG, "brs_monitor_episodes: null argument");
  DeviceGuard g(m->device);
  if (!g.ok) return fail(m, BRS_ERR_HIP, "brs_monitor_episodes: hipSetDevice failed");
  hipStream_t s = (hipStream_t)stream;
  const size_t R = (size_t)m->log_rows;
  if (R > 0) {
    BRS_HIP_TRY(m, hipMemcpyAsync(env_host, m->cols.log_env, R * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    BRS_HIP_TRY(m, hipMemcpyAsync(ret_host, m->cols.log_ret, R * sizeof(double), hipMemcpyDeviceToHost, s));
    BRS_HIP_TRY(m, hipMemcpyAsync(len_host, m->cols.log_len, R * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    BRS_HIP_TRY(m, hipMemcpyAsync(time_limit_host, m->cols.log_time_limit, R, hipMemcpyDeviceToHost, s));
  }
  BRS_HIP_TRY(m, hipStreamSynchronize(s));
  return BRS_OK;
}

}  // extern "C"
