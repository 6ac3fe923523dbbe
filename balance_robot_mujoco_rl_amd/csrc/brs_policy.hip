// brs_policy.hip -- on-device rollout side of the path (include/brs_policy.h): SB3 MlpPolicy
// actor/critic forward + diagonal-Gaussian sample, time-limit bootstrap, GAE(lambda), as HIP kernels for gfx950.
//
// The 6-64-64 towers run on the matrix cores in fp32 (v_mfma_f32_32x32x2_f32; the parity test compares with fp32 torch at rtol
// 1e-5): the tiling -- a wave owns 64 envs, the product is computed transposed, the weights sit in a padded LDS image staged once
// per 256-env workgroup, activations stay in accumulator layout from one layer to the next -- is brs_policy_tile.hpp's, shared
// with the learners of brs_learner.hip; this file holds the kernels around it.  Round 2's kernel walked the towers lane by lane
// with the weights as scalar operands (2,097 s_load per wave, latency-bound): 115 us per policy step at 65,536 envs = 2.5 % of the
// env step it feeds (profiles/r03_rollout_kernel_stats_before_mfma.json); this one: profiles/r03_rollout_kernel_stats.json.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/brs.h"
#include "../../include/brs_policy.h"
#include "brs_host.hpp"
#include "brs_core.hpp"         // philox4x32_10 (same generator as the simulator)
#include "brs_nan.hpp"          // clip_keep_nan
#include "brs_policy_tile.hpp"  // stage_tower, tower_forward, the LDS image of a tower

namespace {

using namespace brs::policy_tile;
constexpr int POLICY_THREADS = 256;  // 4 waves x 64 envs share one staged copy of the weights

// observations of the two envs (32 nt + lane % 32) this lane feeds into the matrix cores; rows beyond n read as zero
__device__ __forceinline__ void load_obs_tiles(const float* __restrict__ obs, int n, int wave_base, float (&x)[2][OBS]) {
  const int c = threadIdx.x & 31;
#pragma unroll
  for (int nt = 0; nt < 2; nt++) {
    const int e = wave_base + 32 * nt + c;
#pragma unroll
    for (int k = 0; k < OBS; k++) x[nt][k] = e < n ? obs[(size_t)OBS * e + k] : 0.0f;
  }
}

__global__ void __launch_bounds__(POLICY_THREADS) policy_act_kernel(const float* __restrict__ w, const int n, const float* __restrict__ obs,
                                                                    const uint64_t seed, const int64_t gid_base, const uint32_t step,
                                                                    const int deterministic, float* __restrict__ action,
                                                                    float* __restrict__ action_clipped, float* __restrict__ logp,
                                                                    float* __restrict__ value, float* __restrict__ noise) {
  __shared__ float Lpi[T_SIZE], Lvf[T_SIZE];
  stage_tower<ACT>(w + OFF_PI, Lpi, blockDim.x);
  stage_tower<1>(w + OFF_VF, Lvf, blockDim.x);
  __syncthreads();
  const int wave_base = blockIdx.x * blockDim.x + (threadIdx.x & ~63), h = (threadIdx.x >> 5) & 1;
  float x[2][OBS], m2[2][ACT], v2[2][1];
  load_obs_tiles(obs, n, wave_base, x);
  tower_forward<ACT>(Lpi, x, m2);   // (no lane leaves before the matrix instructions: they need the whole wave)
  tower_forward<1>(Lvf, x, v2);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // lane l finishes env l of the wave: N-tile h, column l % 32
  if (i >= n) return;
  const float mean[ACT] = {h ? m2[1][0] : m2[0][0], h ? m2[1][1] : m2[0][1]};
  const float v = h ? v2[1][0] : v2[0][0];
  float z[ACT] = {0.0f, 0.0f};
  if (!deterministic) {
    const int64_t gid = gid_base + (int64_t)i;
    uint32_t o[4];
    brs::philox4x32_10(step, 0x504f4c49u, (uint32_t)((uint64_t)gid & 0xffffffffu), (uint32_t)((uint64_t)gid >> 32),
                       (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), o);
    // Box-Muller on two 24-bit uniforms in (0, 1)
    const float u1 = ((float)(o[0] >> 8) + 0.5f) * (1.0f / 16777216.0f), u2 = ((float)(o[1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float r = sqrtf(-2.0f * logf(u1)), th = 6.283185307179586f * u2;
    z[0] = r * cosf(th); z[1] = r * sinf(th);
  }
  float lp = 0.0f;
#pragma unroll
  for (int k = 0; k < ACT; k++) {
    const float ls = w[OFF_LOGSTD + k];
    const float a = fmaf(expf(ls), z[k], mean[k]);
    action[(size_t)ACT * i + k] = a;
    // fminf / fmaxf drop a NaN operand: a NaN action would leave here as -1 and the simulator's bad-state guard, which resets
    // a lane that is handed a NaN action, would never see it.  np.clip (what SB3 applies) keeps the NaN; this unit is IEEE
    action_clipped[(size_t)ACT * i + k] = brs::clip_keep_nan(a, -1.0f, 1.0f);
    lp += -0.5f * z[k] * z[k] - ls - 0.9189385332046727f;  // log N(a; mean, exp(ls)) with (a - mean) / sigma = z
    if (noise) noise[(size_t)ACT * i + k] = z[k];
  }
  logp[i] = lp;
  value[i] = v;
}

__global__ void __launch_bounds__(POLICY_THREADS) policy_value_kernel(const float* __restrict__ w, const int n, const float* __restrict__ obs,
                                                                      float* __restrict__ value) {
  __shared__ float Lvf[T_SIZE];
  stage_tower<1>(w + OFF_VF, Lvf, blockDim.x);
  __syncthreads();
  const int wave_base = blockIdx.x * blockDim.x + (threadIdx.x & ~63), h = (threadIdx.x >> 5) & 1;
  float x[2][OBS], v2[2][1];
  load_obs_tiles(obs, n, wave_base, x);
  tower_forward<1>(Lvf, x, v2);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) value[i] = h ? v2[1][0] : v2[0][0];
}

__global__ void __launch_bounds__(POLICY_THREADS) bootstrap_kernel(const float* __restrict__ w, const int n, const float* __restrict__ tobs,
                                                                   const uint8_t* __restrict__ term, const uint8_t* __restrict__ trunc,
                                                                   const float gamma, float* __restrict__ reward) {
  __shared__ float Lvf[T_SIZE];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool need = i < n && trunc[i] && !term[i];
  if (!__syncthreads_or(need)) return;  // a workgroup without a truncated episode leaves at once (the common case)
  stage_tower<1>(w + OFF_VF, Lvf, blockDim.x);
  __syncthreads();
  const int wave_base = blockIdx.x * blockDim.x + (threadIdx.x & ~63), h = (threadIdx.x >> 5) & 1;
  float x[2][OBS], v2[2][1];
  load_obs_tiles(tobs, n, wave_base, x);
  tower_forward<1>(Lvf, x, v2);
  if (need) reward[i] = fmaf(gamma, h ? v2[1][0] : v2[0][0], reward[i]);
}

// GAE(lambda): one lane per env walks its column of the [T][N] buffers backwards; every access is coalesced over envs
__global__ void __launch_bounds__(256) gae_kernel(const int T, const int N, const float* __restrict__ reward,
                                                  const float* __restrict__ value, const uint8_t* __restrict__ episode_start,
                                                  const float* __restrict__ last_value, const uint8_t* __restrict__ last_done,
                                                  const float gamma, const float lam, float* __restrict__ adv, float* __restrict__ ret) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  float next_value = last_value[i], next_nonterminal = last_done[i] ? 0.0f : 1.0f, gae = 0.0f;
  for (int t = T - 1; t >= 0; t--) {
    const size_t k = (size_t)t * N + i;
    const float v = value[k];
    const float delta = reward[k] + gamma * next_value * next_nonterminal - v;
    gae = delta + gamma * lam * next_nonterminal * gae;
    adv[k] = gae;
    ret[k] = gae + v;
    next_value = v;
    next_nonterminal = episode_start[k] ? 0.0f : 1.0f;
  }
}

}  // namespace

struct brs_policy {
  int device = 0;
  float* w_own = nullptr;  // BRS_POLICY_NPARAM floats owned by the handle
  const float* w = nullptr;
  std::string err;
};

using brs::host::DeviceGuard, brs::host::fail;  // fail<brs_policy>(nullptr, ...): the error of a failed brs_policy_create

extern "C" {

int brs_policy_create(int32_t device, brs_policy** out) {
  if (!out) return fail<brs_policy>(nullptr, BRS_ERR_ARG, "brs_policy_create: null argument");
  *out = nullptr;
  std::string why;
  if (const int rc = brs::host::check_device(device, "brs_policy_create", &why)) return fail<brs_policy>(nullptr, rc, why);
  brs_policy* p = new brs_policy();
  p->device = device;
  DeviceGuard g(device);
  if (!g.ok || hipMalloc(&p->w_own, BRS_POLICY_NPARAM * sizeof(float)) != hipSuccess ||
      hipMemset(p->w_own, 0, BRS_POLICY_NPARAM * sizeof(float)) != hipSuccess) {
    delete p;
    return fail<brs_policy>(nullptr, BRS_ERR_HIP, "brs_policy_create: device allocation failed");
  }
  p->w = p->w_own;
  *out = p;
  return BRS_OK;
}

int brs_policy_destroy(brs_policy* p) {
  if (!p) return BRS_ERR_STATE;
  {
    DeviceGuard g(p->device);
    if (p->w_own) (void)hipFree(p->w_own);
  }
  delete p;
  return BRS_OK;
}

const char* brs_policy_last_error(const brs_policy* p) { return brs::host::last_error(p); }

int brs_policy_set_weights(brs_policy* p, const float* params_host) {
  if (!p) return BRS_ERR_STATE;
  if (!params_host) return fail(p, BRS_ERR_ARG, "brs_policy_set_weights: null pointer");
  DeviceGuard g(p->device);
  if (!g.ok) return fail(p, BRS_ERR_HIP, "brs_policy_set_weights: hipSetDevice failed");
  // kernels enqueued earlier on ANY stream (PyTorch's side streams do not synchronise with the null stream) may still be
  // reading w_own: drain the device before overwriting it.  Not on the rollout path (weights change once per update).
  BRS_HIP_TRY(p, hipDeviceSynchronize());
  BRS_HIP_TRY(p, hipMemcpy(p->w_own, params_host, BRS_POLICY_NPARAM * sizeof(float), hipMemcpyHostToDevice));
  p->w = p->w_own;
  return BRS_OK;
}

int brs_policy_use_device_weights(brs_policy* p, const float* params_dev) {
  if (!p) return BRS_ERR_STATE;
  if (!params_dev) return fail(p, BRS_ERR_ARG, "brs_policy_use_device_weights: null pointer");
  p->w = params_dev;
  return BRS_OK;
}

int brs_policy_act(brs_policy* p, int32_t n, const float* obs_dev, uint64_t seed, int64_t env_index_base, uint32_t step,
                   int32_t deterministic, float* action_dev, float* action_clipped_dev, float* logp_dev, float* value_dev,
                   float* noise_dev, void* stream) {
  if (!p) return BRS_ERR_STATE;
  if (n <= 0 || !obs_dev || !action_dev || !action_clipped_dev || !logp_dev || !value_dev)
    return fail(p, BRS_ERR_ARG, "brs_policy_act: bad argument");
  DeviceGuard g(p->device);
  if (!g.ok) return fail(p, BRS_ERR_HIP, "brs_policy_act: hipSetDevice failed");
  hipLaunchKernelGGL(policy_act_kernel, dim3((n + POLICY_THREADS - 1) / POLICY_THREADS), dim3(POLICY_THREADS), 0, (hipStream_t)stream, p->w, n, obs_dev, seed, env_index_base,
                     step, deterministic, action_dev, action_clipped_dev, logp_dev, value_dev, noise_dev);
  BRS_HIP_TRY(p, hipGetLastError());
  return BRS_OK;
}

int brs_policy_value(brs_policy* p, int32_t n, const float* obs_dev, float* value_dev, void* stream) {
  if (!p) return BRS_ERR_STATE;
  if (n <= 0 || !obs_dev || !value_dev) return fail(p, BRS_ERR_ARG, "brs_policy_value: bad argument");
  DeviceGuard g(p->device);
  if (!g.ok) return fail(p, BRS_ERR_HIP, "brs_policy_value: hipSetDevice failed");
  hipLaunchKernelGGL(policy_value_kernel, dim3((n + POLICY_THREADS - 1) / POLICY_THREADS), dim3(POLICY_THREADS), 0, (hipStream_t)stream, p->w, n, obs_dev, value_dev);
  BRS_HIP_TRY(p, hipGetLastError());
  return BRS_OK;
}

int brs_rollout_bootstrap(brs_policy* p, int32_t n, const float* terminal_obs_dev, const uint8_t* terminated_dev,
                          const uint8_t* truncated_dev, float gamma, float* reward_dev, void* stream) {
  if (!p) return BRS_ERR_STATE;
  if (n <= 0 || !terminal_obs_dev || !terminated_dev || !truncated_dev || !reward_dev)
    return fail(p, BRS_ERR_ARG, "brs_rollout_bootstrap: bad argument");
  DeviceGuard g(p->device);
  if (!g.ok) return fail(p, BRS_ERR_HIP, "brs_rollout_bootstrap: hipSetDevice failed");
  hipLaunchKernelGGL(bootstrap_kernel, dim3((n + POLICY_THREADS - 1) / POLICY_THREADS), dim3(POLICY_THREADS), 0, (hipStream_t)stream, p->w, n, terminal_obs_dev, terminated_dev,
                     truncated_dev, gamma, reward_dev);
  BRS_HIP_TRY(p, hipGetLastError());
  return BRS_OK;
}

int brs_gae(int32_t device, int32_t T, int32_t N, const float* reward_dev, const float* value_dev, const uint8_t* episode_start_dev,
            const float* last_value_dev, const uint8_t* last_done_dev, float gamma, float lam, float* adv_dev, float* ret_dev,
            void* stream) {
  if (T <= 0 || N <= 0 || !reward_dev || !value_dev || !episode_start_dev || !last_value_dev || !last_done_dev || !adv_dev || !ret_dev)
    return BRS_ERR_ARG;
  DeviceGuard g(device);
  if (!g.ok) return BRS_ERR_HIP;
  hipLaunchKernelGGL(gae_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, T, N, reward_dev, value_dev, episode_start_dev,
                     last_value_dev, last_done_dev, gamma, lam, adv_dev, ret_dev);
  return hipGetLastError() == hipSuccess ? BRS_OK : BRS_ERR_HIP;
}

}  // extern "C"
