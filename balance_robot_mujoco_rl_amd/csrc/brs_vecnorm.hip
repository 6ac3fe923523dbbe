// brs_vecnorm.hip -- VecNormalize of include/brs_policy.h as HIP kernels for gfx950: the running mean and
// variance of the observations and of the discounted return that SB3's VecNormalize keeps between the env and the algorithm,
// for all envs next to brs_step.  A training step is three launches, no atomics, no synchronisation:
//
//   vecnorm_moments_kernel  256 threads, workgroup g owns the envs [1024 g, 1024 g + 1024): a thread folds its four envs
//                           (coalesced reads) into seven (count, mean, M2) triples, advancing the discounted return on the
//                           way; a butterfly over the 64 lanes of each wave (fp64 cross-lane moves, two 32-bit moves each); the
//                           four wave results meet in LDS and merge in ascending order: one row of seven triples per workgroup.
//   vecnorm_fold_kernel     one workgroup of seven waves, a column each: lane l folds rows l, l + 64, ..., the same butterfly,
//                           lane 0 applies update_from_moments to the running statistics.
//   vecnorm_apply_kernel    one lane per env: reads the 21 doubles, writes the three outputs, clears `returns` where done.
//
// The shape of the tree is a function of n alone (brs_vecnorm.hpp), so the statistics come out the same bytes on every run and
// in the host build.  When not training only the apply kernel is launched.
//
//   vecnorm_replay_sample_kernel  brs_replay_sample's index and gather with the minibatch normalised on the way out:
//                           eight lanes per sample, one launch, the statistics read and nothing of the handle written.
#include <hip/hip_runtime.h>
#include <string.h>

#include <string>

#include "brs_host.hpp"
#include "brs_vecnorm.hpp"

namespace {

using namespace brs::vecnorm;

constexpr int APPLY_THREADS = 256;

struct Config {
  double gamma, epsilon, clip_obs, clip_reward;
  int norm_obs, norm_reward;
};

__device__ __forceinline__ Triple shfl_xor(const Triple& v, int s) {
  return Triple{__shfl_xor(v.n, s, WAVE), __shfl_xor(v.mean, s, WAVE), __shfl_xor(v.m2, s, WAVE)};
}

// steps s = 1, 2, ... 32 over the wave: the pair (l, l ^ s) merges lower lane first, and both lanes keep the result
__device__ __forceinline__ Triple wave_tree(Triple v, int lane) {
#pragma unroll
  for (int s = 1; s < WAVE; s <<= 1) {
    const Triple o = shfl_xor(v, s);
    const bool lower = (lane & s) == 0;
    v = merge(lower ? v : o, lower ? o : v);
  }
  return v;
}

__global__ void __launch_bounds__(MOMENT_THREADS) vecnorm_moments_kernel(const int n, const float* __restrict__ obs,
                                                                         const float* __restrict__ reward, double* __restrict__ returns,
                                                                         const double gamma, const int with_ret,
                                                                         Triple* __restrict__ partials) {
  __shared__ Triple lds[MOMENT_WAVES][NCOL];
  const int t = threadIdx.x, lane = t & (WAVE - 1), wave = t / WAVE;
  Triple acc[NCOL];
  fold_thread(n, blockIdx.x, t, obs, reward, returns, gamma, with_ret != 0, acc);
#pragma unroll
  for (int c = 0; c < NCOL; c++) acc[c] = wave_tree(acc[c], lane);
  if (lane < NCOL) {  // every lane holds every column's result: lane c hands over column c
    Triple mine = acc[0];
#pragma unroll
    for (int c = 1; c < NCOL; c++)
      if (lane == c) mine = acc[c];
    lds[wave][lane] = mine;
  }
  __syncthreads();
  if (t < NCOL) {
    Triple a = lds[0][t];
#pragma unroll
    for (int w = 1; w < MOMENT_WAVES; w++) a = merge(a, lds[w][t]);
    partials[(int64_t)blockIdx.x * NCOL + t] = a;
  }
}

__global__ void __launch_bounds__(NCOL* WAVE) vecnorm_fold_kernel(const Triple* __restrict__ partials, const int num, const int do_obs,
                                                                  const int do_ret, double* __restrict__ stats) {
  const int lane = threadIdx.x & (WAVE - 1), c = threadIdx.x / WAVE;  // wave-uniform
  if (c < NOBS ? !do_obs : !do_ret) return;
  const Triple a = wave_tree(fold_partials(partials, num, c, lane), lane);
  if (lane == 0) update_from_moments(stats, c, a);
}

__global__ void __launch_bounds__(APPLY_THREADS) vecnorm_apply_kernel(const int n, const Config cfg, const double* __restrict__ stats,
                                                                      const float* __restrict__ obs, const float* __restrict__ reward,
                                                                      const uint8_t* __restrict__ terminated,
                                                                      const uint8_t* __restrict__ truncated,
                                                                      const float* __restrict__ terminal_obs, double* __restrict__ returns,
                                                                      float* __restrict__ obs_out, float* __restrict__ reward_out,
                                                                      float* __restrict__ terminal_obs_out) {
  const int64_t i = (int64_t)blockIdx.x * APPLY_THREADS + threadIdx.x;
  if (i >= n) return;
#pragma unroll
  for (int c = 0; c < NOBS; c++) {
    const float x = obs[i * NOBS + c], y = terminal_obs[i * NOBS + c];
    const double mean = stats[mean_at(c)], var = stats[var_at(c)];
    obs_out[i * NOBS + c] = cfg.norm_obs ? normalize_obs(x, mean, var, cfg.epsilon, cfg.clip_obs) : x;
    terminal_obs_out[i * NOBS + c] = cfg.norm_obs ? normalize_obs(y, mean, var, cfg.epsilon, cfg.clip_obs) : y;
  }
  const float r = reward[i];
  reward_out[i] = cfg.norm_reward ? normalize_reward(r, stats[var_at(RET)], cfg.epsilon, cfg.clip_reward) : r;
  if (terminated[i] | truncated[i]) returns[i] = 0.0;
}

// one lane per element of [m][6]
__global__ void __launch_bounds__(APPLY_THREADS) vecnorm_obs_kernel(const int64_t total, const Config cfg, const double* __restrict__ stats,
                                                                    const float* __restrict__ in, float* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * APPLY_THREADS + threadIdx.x;
  if (k >= total) return;
  const int c = (int)(k % NOBS);
  const float x = in[k];
  out[k] = cfg.norm_obs ? normalize_obs(x, stats[mean_at(c)], stats[var_at(c)], cfg.epsilon, cfg.clip_obs) : x;
}

__global__ void __launch_bounds__(APPLY_THREADS) vecnorm_reward_kernel(const int m, const Config cfg, const double* __restrict__ stats,
                                                                       const float* __restrict__ in, float* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * APPLY_THREADS + threadIdx.x;
  if (k >= m) return;
  const float r = in[k];
  out[k] = cfg.norm_reward ? normalize_reward(r, stats[var_at(RET)], cfg.epsilon, cfg.clip_reward) : r;
}

// ReplayBuffer.sample(batch_size, env=vec_normalize) in one launch: replay_sample_kernel's geometry (brs_offpolicy.hip), 256
// threads, eight lanes per sample, each lane one 8-byte piece or the tail, every lane of a sample computing the same Philox block.
// The elements pass through normalize_obs / normalize_reward of the handle's statistics as they stand when the kernel runs.  V2:
// every pointer of the 8-byte pieces is 8-byte aligned (the host side decides).
template <bool V2> __global__ void __launch_bounds__(SAMPLE_THREADS) vecnorm_replay_sample_kernel(
    const brs_replay_storage s, const int n, const int size, const int m, const uint64_t seed, const uint32_t draw, const SampleNorm cfg,
    const double* __restrict__ stats, const brs_replay_storage out, int32_t* __restrict__ idx) {
  const int64_t t = (int64_t)blockIdx.x * SAMPLE_THREADS + threadIdx.x;
  const int64_t j = t / SAMPLE_PARTS;
  const int part = (int)(t % SAMPLE_PARTS);
  if (j >= m) return;
  int32_t row, env;
  const int64_t cell = sample_cell_of(seed, draw, j, size, n, &row, &env);
  if (part == SAMPLE_PARTS - 1) {
    sample_tail(s, out, idx, cell, j, row, env, cfg, stats);
    return;
  }
  const SamplePiece p = sample_piece(s, out, cell, j, part);
  float v[2];
  if (V2) { const float2 x = *reinterpret_cast<const float2*>(p.src); v[0] = x.x; v[1] = x.y; }
  else { v[0] = p.src[0]; v[1] = p.src[1]; }
  normalize_piece(v, p.col, cfg, stats);
  if (V2) *reinterpret_cast<float2*>(p.dst) = make_float2(v[0], v[1]);
  else { p.dst[0] = v[0]; p.dst[1] = v[1]; }
}

struct StatsArg {
  double v[NSTAT];
};
static_assert(sizeof(brs_vecnorm_stats) == sizeof(StatsArg), "brs_vecnorm_stats is the 21 doubles");

// the statistics travel as a kernel argument: nothing of the caller's is read after the call returns
__global__ void vecnorm_set_stats_kernel(const StatsArg s, double* __restrict__ stats) {
  if (threadIdx.x < NSTAT) stats[threadIdx.x] = s.v[threadIdx.x];
}

unsigned blocks_for(int64_t items) { return (unsigned)((items + APPLY_THREADS - 1) / APPLY_THREADS); }

}  // namespace

struct brs_vecnorm {
  int device = 0, n = 0;
  Config cfg{};
  char* block = nullptr;  // stats [21], returns [n], partials [slabs][7]: one allocation
  double* stats = nullptr;
  double* returns = nullptr;
  brs::vecnorm::Triple* partials = nullptr;
  std::string err;
};

using brs::host::DeviceGuard, brs::host::fail;

namespace {

StatsArg initial_stats() {
  StatsArg s;
  for (int c = 0; c < NCOL; c++) { s.v[mean_at(c)] = 0.0; s.v[var_at(c)] = 1.0; s.v[count_at(c)] = 1e-4; }
  return s;
}

// moments + fold of one batch on the handle's stream; do_ret: the return column is advanced and takes part
int enqueue_update(brs_vecnorm* v, const char* who, const float* obs, const float* reward, bool do_obs, bool do_ret, hipStream_t s) {
  const int slabs = num_slabs(v->n);
  hipLaunchKernelGGL(vecnorm_moments_kernel, dim3(slabs), dim3(MOMENT_THREADS), 0, s, v->n, obs, reward, v->returns, v->cfg.gamma,
                     do_ret ? 1 : 0, v->partials);
  hipLaunchKernelGGL(vecnorm_fold_kernel, dim3(1), dim3(NCOL * WAVE), 0, s, v->partials, slabs, do_obs ? 1 : 0, do_ret ? 1 : 0, v->stats);
  if (hipGetLastError() != hipSuccess) return fail(v, BRS_ERR_HIP, std::string(who) + ": kernel launch failed");
  return BRS_OK;
}

}  // namespace

extern "C" {

int brs_vecnorm_create(int32_t device, int32_t n, const brs_vecnorm_config* config, brs_vecnorm** out) {
  if (!out) return fail<brs_vecnorm>(nullptr, BRS_ERR_ARG, "brs_vecnorm_create: null argument");
  *out = nullptr;
  if (!config) return fail<brs_vecnorm>(nullptr, BRS_ERR_ARG, "brs_vecnorm_create: null argument");
  if (n <= 0) return fail<brs_vecnorm>(nullptr, BRS_ERR_ARG, "brs_vecnorm_create: n must be positive");
  if (!(config->clip_obs >= 0.0)) return fail<brs_vecnorm>(nullptr, BRS_ERR_ARG, "brs_vecnorm_create: clip_obs must not be negative");
  if (!(config->clip_reward >= 0.0)) return fail<brs_vecnorm>(nullptr, BRS_ERR_ARG, "brs_vecnorm_create: clip_reward must not be negative");
  std::string why;
  if (const int rc = brs::host::check_device(device, "brs_vecnorm_create", &why)) return fail<brs_vecnorm>(nullptr, rc, why);
  brs_vecnorm* v = new brs_vecnorm();
  v->device = device; v->n = n;
  v->cfg = Config{config->gamma, config->epsilon, config->clip_obs, config->clip_reward, config->norm_obs != 0, config->norm_reward != 0};
  const size_t o_stats = 0, o_returns = 256, o_partials = o_returns + ((8 * (size_t)n + 255) & ~(size_t)255);
  const size_t bytes = o_partials + (size_t)num_slabs(n) * NCOL * sizeof(Triple);
  DeviceGuard g(device);
  if (!g.ok || hipMalloc((void**)&v->block, bytes) != hipSuccess) {
    delete v;
    return fail<brs_vecnorm>(nullptr, BRS_ERR_HIP, "brs_vecnorm_create: device allocation failed");
  }
  v->stats = (double*)(v->block + o_stats); v->returns = (double*)(v->block + o_returns); v->partials = (Triple*)(v->block + o_partials);
  // a new handle: statistics 0, 1, 1e-4, returns 0 (all-zero bytes), on the null stream, finished before create returns
  hipError_t e = hipMemset(v->block, 0, bytes);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(vecnorm_set_stats_kernel, dim3(1), dim3(WAVE), 0, 0, initial_stats(), v->stats);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(0);
  if (e != hipSuccess) {
    (void)hipFree(v->block);
    delete v;
    return fail<brs_vecnorm>(nullptr, BRS_ERR_HIP, std::string("brs_vecnorm_create: ") + hipGetErrorString(e));
  }
  *out = v;
  return BRS_OK;
}

int brs_vecnorm_destroy(brs_vecnorm* v) {
  if (!v) return BRS_ERR_STATE;
  {
    DeviceGuard g(v->device);
    if (v->block) (void)hipFree(v->block);
  }
  delete v;
  return BRS_OK;
}

const char* brs_vecnorm_last_error(const brs_vecnorm* v) { return brs::host::last_error(v); }

int brs_vecnorm_reset(brs_vecnorm* v, const float* obs_dev, int32_t training, float* obs_out_dev, void* stream) {
  if (!v) return BRS_ERR_STATE;
  if (!obs_dev || !obs_out_dev) return fail(v, BRS_ERR_ARG, "brs_vecnorm_reset: null argument");
  DeviceGuard g(v->device);
  if (!g.ok) return fail(v, BRS_ERR_HIP, "brs_vecnorm_reset: hipSetDevice failed");
  hipStream_t s = (hipStream_t)stream;
  BRS_HIP_TRY(v, hipMemsetAsync(v->returns, 0, sizeof(double) * (size_t)v->n, s));
  if (training && v->cfg.norm_obs)
    if (const int rc = enqueue_update(v, "brs_vecnorm_reset", obs_dev, nullptr, true, false, s)) return rc;
  const int64_t total = (int64_t)v->n * NOBS;
  hipLaunchKernelGGL(vecnorm_obs_kernel, dim3(blocks_for(total)), dim3(APPLY_THREADS), 0, s, total, v->cfg, v->stats, obs_dev, obs_out_dev);
  if (hipGetLastError() != hipSuccess) return fail(v, BRS_ERR_HIP, "brs_vecnorm_reset: kernel launch failed");
  return BRS_OK;
}

int brs_vecnorm_step(brs_vecnorm* v, const float* obs_dev, const float* reward_dev, const uint8_t* terminated_dev,
                     const uint8_t* truncated_dev, const float* terminal_obs_dev, int32_t training, float* obs_out_dev,
                     float* reward_out_dev, float* terminal_obs_out_dev, void* stream) {
  if (!v) return BRS_ERR_STATE;
  if (!obs_dev || !reward_dev || !terminated_dev || !truncated_dev || !terminal_obs_dev || !obs_out_dev || !reward_out_dev ||
      !terminal_obs_out_dev)
    return fail(v, BRS_ERR_ARG, "brs_vecnorm_step: null argument");
  DeviceGuard g(v->device);
  if (!g.ok) return fail(v, BRS_ERR_HIP, "brs_vecnorm_step: hipSetDevice failed");
  hipStream_t s = (hipStream_t)stream;
  if (training)
    if (const int rc = enqueue_update(v, "brs_vecnorm_step", obs_dev, reward_dev, v->cfg.norm_obs != 0, true, s)) return rc;
  hipLaunchKernelGGL(vecnorm_apply_kernel, dim3(blocks_for(v->n)), dim3(APPLY_THREADS), 0, s, v->n, v->cfg, v->stats, obs_dev, reward_dev,
                     terminated_dev, truncated_dev, terminal_obs_dev, v->returns, obs_out_dev, reward_out_dev, terminal_obs_out_dev);
  if (hipGetLastError() != hipSuccess) return fail(v, BRS_ERR_HIP, "brs_vecnorm_step: kernel launch failed");
  return BRS_OK;
}

int brs_vecnorm_normalize_obs(brs_vecnorm* v, int32_t m, const float* in_dev, float* out_dev, void* stream) {
  if (!v) return BRS_ERR_STATE;
  if (!in_dev || !out_dev) return fail(v, BRS_ERR_ARG, "brs_vecnorm_normalize_obs: null argument");
  if (m <= 0) return fail(v, BRS_ERR_ARG, "brs_vecnorm_normalize_obs: m must be positive");
  DeviceGuard g(v->device);
  if (!g.ok) return fail(v, BRS_ERR_HIP, "brs_vecnorm_normalize_obs: hipSetDevice failed");
  const int64_t total = (int64_t)m * NOBS;
  hipLaunchKernelGGL(vecnorm_obs_kernel, dim3(blocks_for(total)), dim3(APPLY_THREADS), 0, (hipStream_t)stream, total, v->cfg, v->stats,
                     in_dev, out_dev);
  if (hipGetLastError() != hipSuccess) return fail(v, BRS_ERR_HIP, "brs_vecnorm_normalize_obs: kernel launch failed");
  return BRS_OK;
}

int brs_vecnorm_normalize_reward(brs_vecnorm* v, int32_t m, const float* in_dev, float* out_dev, void* stream) {
  if (!v) return BRS_ERR_STATE;
  if (!in_dev || !out_dev) return fail(v, BRS_ERR_ARG, "brs_vecnorm_normalize_reward: null argument");
  if (m <= 0) return fail(v, BRS_ERR_ARG, "brs_vecnorm_normalize_reward: m must be positive");
  DeviceGuard g(v->device);
  if (!g.ok) return fail(v, BRS_ERR_HIP, "brs_vecnorm_normalize_reward: hipSetDevice failed");
  hipLaunchKernelGGL(vecnorm_reward_kernel, dim3(blocks_for(m)), dim3(APPLY_THREADS), 0, (hipStream_t)stream, m, v->cfg, v->stats, in_dev,
                     out_dev);
  if (hipGetLastError() != hipSuccess) return fail(v, BRS_ERR_HIP, "brs_vecnorm_normalize_reward: kernel launch failed");
  return BRS_OK;
}

int brs_replay_sample_vecnorm(brs_vecnorm* v, const brs_replay_storage* storage, int32_t n, int32_t cap, int32_t size, int32_t m,
                              uint64_t seed, uint32_t draw, const brs_replay_storage* out, int32_t* idx_dev, void* stream) {
  if (!v) return BRS_ERR_STATE;
  if (const char* why = replay_sample_argument_error(storage, n, cap, size, m, out))
    return fail(v, BRS_ERR_ARG, std::string("brs_replay_sample_vecnorm: ") + why);
  DeviceGuard g(v->device);
  if (!g.ok) return fail(v, BRS_ERR_HIP, "brs_replay_sample_vecnorm: hipSetDevice failed");
  bool v2 = true;
  for (const void* p : {(const void*)storage->obs, (const void*)storage->next_obs, (const void*)storage->action, (const void*)out->obs,
                        (const void*)out->next_obs, (const void*)out->action})
    v2 = v2 && ((uintptr_t)p & 7) == 0;
  const SampleNorm cfg{v->cfg.epsilon, v->cfg.clip_obs, v->cfg.clip_reward, v->cfg.norm_obs, v->cfg.norm_reward};
  const dim3 grid((unsigned)(((int64_t)m * SAMPLE_PARTS + SAMPLE_THREADS - 1) / SAMPLE_THREADS));
  if (v2)
    hipLaunchKernelGGL(vecnorm_replay_sample_kernel<true>, grid, dim3(SAMPLE_THREADS), 0, (hipStream_t)stream, *storage, n, size, m, seed, draw,
                       cfg, v->stats, *out, idx_dev);
  else
    hipLaunchKernelGGL(vecnorm_replay_sample_kernel<false>, grid, dim3(SAMPLE_THREADS), 0, (hipStream_t)stream, *storage, n, size, m, seed, draw,
                       cfg, v->stats, *out, idx_dev);
  if (hipGetLastError() != hipSuccess) return fail(v, BRS_ERR_HIP, "brs_replay_sample_vecnorm: kernel launch failed");
  return BRS_OK;
}

int brs_vecnorm_get_stats(brs_vecnorm* v, brs_vecnorm_stats* out_host, void* stream) {
  if (!v) return BRS_ERR_STATE;
  if (!out_host) return fail(v, BRS_ERR_ARG, "brs_vecnorm_get_stats: null argument");
  DeviceGuard g(v->device);
  if (!g.ok) return fail(v, BRS_ERR_HIP, "brs_vecnorm_get_stats: hipSetDevice failed");
  hipStream_t s = (hipStream_t)stream;
  BRS_HIP_TRY(v, hipMemcpyAsync(out_host, v->stats, sizeof(brs_vecnorm_stats), hipMemcpyDeviceToHost, s));
  BRS_HIP_TRY(v, hipStreamSynchronize(s));
  return BRS_OK;
}

int brs_vecnorm_set_stats(brs_vecnorm* v, const brs_vecnorm_stats* in_host, void* stream) {
  if (!v) return BRS_ERR_STATE;
  if (!in_host) return fail(v, BRS_ERR_ARG, "brs_vecnorm_set_stats: null argument");
  DeviceGuard g(v->device);
  if (!g.ok) return fail(v, BRS_ERR_HIP, "brs_vecnorm_set_stats: hipSetDevice failed");
  StatsArg a;
  memcpy(&a, in_host, sizeof(a));
  hipLaunchKernelGGL(vecnorm_set_stats_kernel, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, a, v->stats);
  if (hipGetLastError() != hipSuccess) return fail(v, BRS_ERR_HIP, "brs_vecnorm_set_stats: kernel launch failed");
  return BRS_OK;
}

int brs_vecnorm_get_returns(brs_vecnorm* v, double* returns_host, void* stream) {
  if (!v) return BRS_ERR_STATE;
  if (!returns_host) return fail(v, BRS_ERR_ARG, "brs_vecnorm_get_returns: null argument");
  DeviceGuard g(v->device);
  if (!g.ok) return fail(v, BRS_ERR_HIP, "brs_vecnorm_get_returns: hipSetDevice failed");
  hipStream_t s = (hipStream_t)stream;
  BRS_HIP_TRY(v, hipMemcpyAsync(returns_host, v->returns, sizeof(double) * (size_t)v->n, hipMemcpyDeviceToHost, s));
  BRS_HIP_TRY(v, hipStreamSynchronize(s));
  return BRS_OK;
}

}  // extern "C"
