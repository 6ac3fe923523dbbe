// brs_kernels.hip -- HIP kernels (gfx950 / CDNA4) and the C ABI of include/brs.h.
//
// Host side: device guard, error slots and device check are brs_host.hpp's, shared with the library's other three units; every
// entry point that touches the device constructs the guard and returns BRS_ERR_HIP if it is not `ok`.  What differs between
// the two model families is one row of FamilyOps, which the handle points to.
//
// Kernel design:
//   * one wavefront LANE per environment instance; a 64-thread workgroup is one wave.  At the benchmark size
//     (65,536 envs) the grid is 1,024 waves = one wave per SIMD of the 256 CUs, so the register budget is the
//     full 512 VGPRs and nothing is gained by trading registers for occupancy.
//   * the whole env step (reward, control law, 250 substeps, block state machine, termination, observation,
//     time limit, auto-reset with in-kernel Philox) is ONE launch; state is read once from HBM (field-major
//     SoA: every wave-level load is one contiguous segment) and written once.
//   * the per-lane contact list lives in LDS as lane-strided columns (word w of slot s at (s*8+w)*64 + lane):
//     ds_read_b32/ds_write_b32 with consecutive lanes on consecutive banks, conflict-free by construction.
//   * the tiny dense solves (8x8 / 6x6 / 14x14 Cholesky of M + J^T D J) are fully unrolled on statically
//     indexed register arrays -- no MFMA (a 2-wheel rigid body is not a dense contraction), no scratch.
//   * no inter-lane communication, no barriers, no atomics: lanes are independent envs.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/brs.h"
#include "brs_host.hpp"
#if defined(BRS_TIMING)
__device__ unsigned long long brs_dbg[16];
// per-wave record of the last launch, 16 words per wave (waves 0-1023): phase slots 0-11 (brs_core.hpp: BRS_TIC ids), HW_ID,
// XCC_ID, lanes per cost-class key (8 x u8) and lanes per bucket (8 x u8) of the keys the lane map was built from
__device__ unsigned long long brs_dbg_wave[16 * 1024];
#define BRS_TIMING_LANE_WORDS 153
#endif
#include "brs_state.hpp"

using namespace brs;

namespace {

template <bool BLK> constexpr int lane_words() { return BLK ? LDS_WORDS_ENV03 : LDS_WORDS_ENV01; }

template <bool BLK> __device__ __forceinline__ Store<float> lane_store(float* lds) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  return Store<float>{lds + wave * (64 * lane_words<BLK>()) + lane, 64};
}

// VARIANT >= 0: the model constants of that registered id are folded at COMPILE time (constexpr make_params, default
// timestep / substeps): ~100 values become instruction literals instead of SGPRs.  The kernel is SGPR-bound as well as
// VGPR-bound -- with the constants in kernel arguments 5-15 % of its loop instructions were v_readlane reloads of spilled
// SGPRs, each a VALU issue slot.  Only the per-handle fields stay runtime.  VARIANT = -1: everything runtime (non-default
// timestep).
template <int VARIANT> __device__ __forceinline__ Params<float> fold_params(const Params<float>& rt) {
  if constexpr (VARIANT < 0) return rt;
  else {
    constexpr Params<float> c = make_params<float>(VARIANT, 0u, -1, 0, 0, 0.0, 0, 0);
    Params<float> p = c;
    p.seed = rt.seed; p.gid_base = rt.gid_base; p.auto_reset = rt.auto_reset; p.noise = rt.noise;
    p.max_episode_steps = rt.max_episode_steps; p.nsub = rt.nsub;
    return p;
  }
}

// Lane grouping (Env03): after every step the envs are regrouped along the lanes by the cost class of their NEXT step
// (brs_state.hpp: cost_class).  The bucket of an env is its cost-class key; brs_state.hpp: lane_slot lays the buckets out
// along the lanes, every expensive bucket from a wave boundary with far lanes filling its last wave.  The step kernel
// counts its lanes per bucket as it retires (wave-aggregated atomics into 8 counters behind the lane map), brs_group_kernel
// ranks the envs inside their buckets with wave-aggregated cursors and turns (bucket, rank, counts) into a slot: a few
// microseconds over 256 workgroups.  (Round 2a: a stable counting sort in ONE workgroup, 95 us = 2 % of the step.)  The order
// inside a bucket depends on the order the atomics arrive in -- an env's arithmetic does not depend on its lane, so results
// stay bit-identical (tests/test_lane_map_gpu.py).
constexpr int NBUCKET = LM_NBUCKET;
// counters behind the lane map and the keys: cnt[NBUCKET] (lanes per bucket, filled by the step kernel), cursor[NBUCKET], ticket
constexpr int GROUP_WORDS = 32;
static_assert(2 * NBUCKET + 1 <= GROUP_WORDS, "bucket counters do not fit");
template <bool BLK> __device__ __forceinline__ unsigned* group_counters(int* ii, int N) {
  return (unsigned*)(ii + ((size_t)Layout<BLK>::NI + 2) * N);
}

template <bool BLK, int VARIANT>
__device__ __forceinline__ void step_body(const Params<float>& Prt, const int N, double* __restrict__ d, float* __restrict__ f,
                                          int* __restrict__ ii, const float* __restrict__ actions, float* __restrict__ obs,
                                          float* __restrict__ reward, uint8_t* __restrict__ terminated,
                                          uint8_t* __restrict__ truncated, float* __restrict__ terminal_obs) {
  extern __shared__ float brs_lds_dyn[];
  float* lds = brs_lds_dyn;
  const int lane_slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (lane_slot >= N) return;  // no barriers anywhere: a partial last wave just masks lanes
  const Params<float> P = fold_params<VARIANT>(Prt);
  // lane <-> env: identity, or the cost-class grouping computed after the previous step (brs_state.hpp: cost_class).  The
  // gather makes the state accesses of a wave non-contiguous; at < 0.2 % of the HBM roofline that costs nothing.  The env
  // index is re-read wherever it is needed instead of being held across the loop (brs_state.hpp: LaneIndex).
  // The map and the cost classes live behind the int state in the SAME allocation (ii + NI * N: perm[N], then keys[N] bytes):
  // no extra kernel arguments -- the kernel is SGPR-bound too (its Params live in SGPRs), and two more pointers held across
  // the loop cost ~10 % in spill traffic (measured).  Env01 has no rare collision paths: identity, decided at compile time.
  const LaneIndex idx{BLK ? ii + (size_t)Layout<BLK>::NI * N : nullptr, lane_slot};
  Store<float> st = lane_store<BLK>(lds);
#if defined(BRS_TIMING) && defined(__HIP_DEVICE_COMPILE__)
  if ((threadIdx.x & 63) == 0) for (int k = 0; k < 16; k++) brs_tim_slots()[k] = 0;
  if constexpr (BLK) {  // the wave's composition at launch: the keys are read before this step overwrites them
    const int key = ((const uint8_t*)(ii + ((size_t)Layout<BLK>::NI + 1) * N))[idx.get()];
    unsigned long long ck = 0ull;
    for (int k = 0; k < 8; k++) ck |= (unsigned long long)__popcll(__ballot(key == k)) << (8 * k);
    if ((threadIdx.x & 63) == 0) { brs_tim_slots()[14] = ck; brs_tim_slots()[15] = ck; }  // (the buckets are the keys)
  }
#endif
  Stream<float> rng;
  float a0, a1;
  {
    const size_t i = idx.get();
    rng.open(P.seed, P.gid_base + (int64_t)i, 0u);
    a0 = actions[2 * i]; a1 = actions[2 * i + 1];
    if (isnan_(a0) | isnan_(a1)) ii[(size_t)Layout<BLK>::I_BAD * N + i] |= BAD_START_BIT;
  }
  float o[6], to[6], rew;
  int te, tr, cls = 0;
  env_step_idx<float, BLK, float, LaneIndex>(P, st, rng, d, f, ii, (size_t)N, idx, a0, a1, o, to, rew, te, tr, BLK ? &cls : nullptr);
  const size_t i = idx.get();
  if constexpr (BLK) {
    ((uint8_t*)(ii + ((size_t)Layout<BLK>::NI + 1) * N))[i] = (uint8_t)cls;
    const int b = cls;
    unsigned* cnt = group_counters<BLK>(ii, N);
#pragma unroll
    for (int k = 0; k < NBUCKET; k++) {
      const unsigned long long m = __ballot(b == k);
      if (m != 0ull && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(&cnt[k], (unsigned)__popcll(m));
    }
  }
#if defined(BRS_TIMING) && defined(__HIP_DEVICE_COMPILE__)
  if ((threadIdx.x & 63) == 0) {
    for (int k = 0; k < 12; k++) atomicAdd(&brs_dbg[k], brs_tim_slots()[k]);
    atomicMax(&brs_dbg[12], brs_tim_slots()[8]);  // slowest wave of the launch: cycles, trips (load imbalance, 1 wave per SIMD)
    atomicMax(&brs_dbg[13], brs_tim_slots()[9]);
    // per-wave record of the LAST launch: phase cycles, where the wave ran, what it carried (which lanes made it slow?)
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    const unsigned w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (w < 1024) {
      for (int k = 0; k < 12; k++) brs_dbg_wave[16 * w + k] = brs_tim_slots()[k];
      brs_dbg_wave[16 * w + 12] = hw; brs_dbg_wave[16 * w + 13] = xcc;
      brs_dbg_wave[16 * w + 14] = BLK ? brs_tim_slots()[14] : 0ull; brs_dbg_wave[16 * w + 15] = BLK ? brs_tim_slots()[15] : 0ull;
    }
  }
#endif
#pragma unroll
  for (int k = 0; k < 6; k++) obs[6 * (size_t)i + k] = o[k];
  if (terminal_obs) {
#pragma unroll
    for (int k = 0; k < 6; k++) terminal_obs[6 * (size_t)i + k] = to[k];
  }
  reward[i] = rew;
  terminated[i] = (uint8_t)te;
  truncated[i] = (uint8_t)tr;
}

#define BRS_STEP_ARGS                                                                                                      \
  const Params<float> Prt, const int N, double *__restrict__ d, float *__restrict__ f, int *__restrict__ ii,              \
      const float *__restrict__ actions, float *__restrict__ obs, float *__restrict__ reward, uint8_t *__restrict__ terminated, \
      uint8_t *__restrict__ truncated, float *__restrict__ terminal_obs
template <bool BLK, int VARIANT> __global__ void __launch_bounds__(256) brs_step_kernel(BRS_STEP_ARGS) {
  step_body<BLK, VARIANT>(Prt, N, d, f, ii, actions, obs, reward, terminated, truncated, terminal_obs);
}
// The Env01-family body (8 dofs, 336 registers when left alone) capped at 256 registers so that TWO waves fit a SIMD
// (LDS: 14 KB per wave, no limit).  Measured, Env01-v2: 65,536 envs (1,024 waves = one per SIMD either way)
// 49.0 vs 48.0 M env-steps/s -- the 109 spilled VGPRs cost nothing visible; 131,072 / 262,144 / 524,288 envs: 70.9 / 75.5 /
// 79.1 M vs 49.8 / 50.9 / 51.5 M: the second resident wave is worth x1.42 - 1.54 as soon as a launch has more waves than the
// chip has SIMDs.  Default for 64-thread workgroups; BRS_ENV01_OCC1=1 selects the uncapped build (A/B).
template <int VARIANT> __global__ void __launch_bounds__(64, 2) brs_step_kernel_occ2(BRS_STEP_ARGS) {
  step_body<false, VARIANT>(Prt, N, d, f, ii, actions, obs, reward, terminated, truncated, terminal_obs);
}

template <bool BLK>
__global__ void __launch_bounds__(256) brs_reset_kernel(const Params<float> P, const int N, double* __restrict__ d,
                                                        float* __restrict__ f, int* __restrict__ ii,
                                                        const uint8_t* __restrict__ mask, float* __restrict__ obs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  if (mask && !mask[i]) return;
  EnvState<float, BLK> S;
  load_state<float, BLK>(S, d, f, ii, (size_t)N, (size_t)i);
  Stream<float> rng;
  rng.open(P.seed, P.gid_base + (int64_t)i, S.rng_ctr);
  float o[6];
  Sim<float, BLK>::env_reset(P, S, rng, o);
  S.rng_ctr = rng.ctr;
  store_state<float, BLK>(S, d, f, ii, (size_t)N, (size_t)i);
#pragma unroll
  for (int k = 0; k < 6; k++) obs[6 * (size_t)i + k] = o[k];
}

template <bool BLK>
__global__ void __launch_bounds__(256) brs_physics_kernel(const Params<float> P, const int N, double* __restrict__ d,
                                                          float* __restrict__ f, int* __restrict__ ii,
                                                          const float* __restrict__ ctrl, const int nsub) {
  extern __shared__ float brs_lds_dyn[];
  float* lds = brs_lds_dyn;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  Store<float> st = lane_store<BLK>(lds);
  physics_mem<float, BLK, float>(P, st, d, f, ii, (size_t)N, (size_t)i, ctrl[2 * (size_t)i], ctrl[2 * (size_t)i + 1], nsub);
}

constexpr int GROUP_THREADS = 256, GROUP_ENVS = 1024;  // small workgroups (they have to find room between step-kernel waves
                                                       // when several handles share a GPU), 4 envs per thread
__global__ void __launch_bounds__(GROUP_THREADS) brs_group_kernel(const int N, const uint8_t* __restrict__ keys, int* __restrict__ perm,
                                                                  unsigned* __restrict__ ctr, const unsigned cap) {
  // ONE slot request per workgroup and bucket: same-address device atomics are the cost of this kernel (one request per
  // wave: 61 us for 65,536 envs; per 1,024 envs: 7 us).  Wave counts -> LDS -> exclusive offsets inside the workgroup
  constexpr int NV = GROUP_ENVS / 64;  // 64-env groups of the workgroup ("virtual waves": 4 passes x 4 waves)
  __shared__ unsigned wcnt[NV][NBUCKET], woff[NBUCKET], cnt[NBUCKET];
  __shared__ LanePlan plan;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int b[GROUP_ENVS / GROUP_THREADS];
  unsigned long long mine[GROUP_ENVS / GROUP_THREADS];
#pragma unroll
  for (int j = 0; j < GROUP_ENVS / GROUP_THREADS; j++) {
    const int e = blockIdx.x * GROUP_ENVS + j * GROUP_THREADS + threadIdx.x;
    b[j] = e < N ? (int)keys[e] : -1;
    mine[j] = 0ull;
#pragma unroll
    for (int k = 0; k < NBUCKET; k++) {
      const unsigned long long m = __ballot(b[j] == k);
      if (lane == 0) wcnt[j * (GROUP_THREADS / 64) + w][k] = (unsigned)__popcll(m);
      mine[j] = b[j] == k ? m : mine[j];
    }
  }
  __syncthreads();
  if (threadIdx.x < NBUCKET) {  // thread k: the step kernel's count of bucket k, this workgroup's share of the bucket's cursor
    const int k = threadIdx.x;
    unsigned tot = 0;
    cnt[k] = ctr[k];
    for (int v = 0; v < NV; v++) { const unsigned c = wcnt[v][k]; wcnt[v][k] = tot; tot += c; }  // exclusive over the 64-env groups
    woff[k] = tot ? atomicAdd(&ctr[NBUCKET + k], tot) : 0u;
  }
  __syncthreads();
  if (threadIdx.x == 0) plan = lane_plan(cnt, cap);  // where the buckets go: once per workgroup
  __syncthreads();
#pragma unroll
  for (int j = 0; j < GROUP_ENVS / GROUP_THREADS; j++) {
    const int e = blockIdx.x * GROUP_ENVS + j * GROUP_THREADS + threadIdx.x;
    if (b[j] >= 0) {
      const unsigned r = woff[b[j]] + wcnt[j * (GROUP_THREADS / 64) + w][b[j]] + (unsigned)__popcll(mine[j] & ((1ull << lane) - 1ull));
      perm[lane_slot(plan, cnt, b[j], r)] = e;
    }
  }
  // the last workgroup to finish clears the counters for the next step (every other one has read them by then)
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    if (atomicAdd(&ctr[2 * NBUCKET], 1u) == gridDim.x - 1) {
#pragma unroll
      for (int k = 0; k <= 2 * NBUCKET; k++) ctr[k] = 0u;
    }
  }
}

// What the host side has to know about a model family (Env01: robot alone; Env03: robot and block), filled once per family
// (make_family_ops below): the entry points read the handle's row instead of branching on the family.
struct FamilyOps {
  int nq, nv, lds_words;                 // row widths of brs_get_state / brs_set_state; LDS words per lane (step, physics)
  size_t ND, NF, NI, bytes_per_env;      // state fields per env (fp64, fp32, int32) and their size
  const void *reset_kernel, *physics_kernel;
  // brs_state.hpp: the conversions between MuJoCo-style rows and the device layout (same signatures in both families)
  decltype(&hostconv::init_state<true, float>) init_state;
  decltype(&hostconv::mark_bad_start<true, float>) mark_bad_start;
  decltype(&hostconv::get_state<true, float>) get_state;   decltype(&hostconv::set_state<true, float>) set_state;
  decltype(&hostconv::get_aux<true, float>) get_aux;       decltype(&hostconv::set_aux<true, float>) set_aux;
  decltype(&hostconv::get_xpose<true>) get_xpose;          decltype(&hostconv::set_xpose<true>) set_xpose;
};

}  // namespace

struct brs_handle {
  Params<float> P;
  int N = 0, device = 0, bt = 64;
  const FamilyOps* ops = nullptr;
  bool blk = false;          // Env03 family: the step kernel maintains the lane map and the bucket counters
  double* d = nullptr;
  float* f = nullptr;
  int* ii = nullptr;
  size_t nd = 0, nf = 0, ni = 0;
  bool folded = false;       // model constants folded at compile time (default timestep): variant-specific step kernel
  bool occ2 = false;         // Env01 family: body capped at 256 registers, two waves per SIMD (default; BRS_ENV01_OCC1=1: off)
  bool grouping = false;     // Env03: regroup lanes by cost class after every step (perm / keys live behind the int state)
  unsigned wheel_cap = LM_WAVE;  // wheel lanes per wave in the lane map: diluted only if the launch fits one wave per SIMD
  int* perm() const { return ii + ni; }                            // [N] lane slot -> env
  uint8_t* keys() const { return (uint8_t*)(ii + ni + (size_t)N); }  // [N] cost class of every env for its next step
  unsigned* counters() const { return (unsigned*)(ii + ni + 2 * (size_t)N); }  // [GROUP_WORDS] bucket counts, cursors, ticket
  std::string err;
};

namespace {

using host::DeviceGuard, host::fail;  // fail<brs_handle>(nullptr, ...): the error of a failed brs_create
#if defined(BRS_TIMING)
size_t lds_bytes(const brs_handle* h) { return (size_t)h->bt * BRS_TIMING_LANE_WORDS * sizeof(float) + (size_t)(h->bt / 64) * 128; }
#else
size_t lds_bytes(const brs_handle* h) { return (size_t)h->bt * h->ops->lds_words * sizeof(float); }
#endif
// one lane per env, workgroups of the handle's size; the launch's status is what hipGetLastError returns
int launch_per_env(brs_handle* h, const void* kernel, void** args, size_t lds, void* stream) {
  (void)hipLaunchKernel(kernel, dim3((h->N + h->bt - 1) / h->bt), dim3(h->bt), args, lds, (hipStream_t)stream);
  BRS_HIP_TRY(h, hipGetLastError());
  return BRS_OK;
}

// every step-kernel instantiation there is: brs_create prepares a handle's rows, brs_step launches the one step_kernel_of selects
struct StepKernel { bool blk, occ2; int variant; const void* fn; };
const StepKernel STEP_KERNELS[] = {
    {true, false, -1, (const void*)brs_step_kernel<true, -1>},
    {true, false, ENV03_V1, (const void*)brs_step_kernel<true, ENV03_V1>},
    {true, false, ENV03_V2, (const void*)brs_step_kernel<true, ENV03_V2>},
    {false, false, -1, (const void*)brs_step_kernel<false, -1>},
    {false, false, ENV01_V1, (const void*)brs_step_kernel<false, ENV01_V1>},
    {false, false, ENV01_V2, (const void*)brs_step_kernel<false, ENV01_V2>},
    {false, false, ENV01_V3, (const void*)brs_step_kernel<false, ENV01_V3>},
    {false, false, ENV02_V1, (const void*)brs_step_kernel<false, ENV02_V1>},
    {false, true, -1, (const void*)brs_step_kernel_occ2<-1>},
    {false, true, ENV01_V1, (const void*)brs_step_kernel_occ2<ENV01_V1>},
    {false, true, ENV01_V2, (const void*)brs_step_kernel_occ2<ENV01_V2>},
    {false, true, ENV01_V3, (const void*)brs_step_kernel_occ2<ENV01_V3>},
    {false, true, ENV02_V1, (const void*)brs_step_kernel_occ2<ENV02_V1>},
};
// the kernel brs_step launches for this handle: the capped build only for the Env01 family at one wave per workgroup, model
// constants folded only at the default timestep (every handle brs_create returns has one: it checks)
const StepKernel* step_kernel_of(const brs_handle* h) {
  const bool occ2 = !h->blk && h->occ2 && h->bt == 64;
  const int variant = h->folded ? h->P.variant : -1;
  for (const StepKernel& k : STEP_KERNELS)
    if (k.blk == h->blk && k.occ2 == occ2 && k.variant == variant) return &k;
  return nullptr;
}

// The reset and physics kernels, Env03 family first.  Like STEP_KERNELS this names its kernels for the first time, and the order
// of first mention is the order the device code is emitted in: keep it, and a build's device code can be compared with its parent's.
const void* const PHYSICS_KERNELS[] = {(const void*)brs_physics_kernel<true>, (const void*)brs_physics_kernel<false>};
const void* const RESET_KERNELS[] = {(const void*)brs_reset_kernel<true>, (const void*)brs_reset_kernel<false>};

template <bool BLK> FamilyOps make_family_ops() {
  using L = Layout<BLK>;
  return {L::NQ, L::NV, lane_words<BLK>(), L::ND, L::NF, L::NI, L::bytes_per_env, RESET_KERNELS[BLK ? 0 : 1], PHYSICS_KERNELS[BLK ? 0 : 1],
          hostconv::init_state<BLK, float>, hostconv::mark_bad_start<BLK, float>, hostconv::get_state<BLK, float>, hostconv::set_state<BLK, float>,
          hostconv::get_aux<BLK, float>, hostconv::set_aux<BLK, float>, hostconv::get_xpose<BLK>, hostconv::set_xpose<BLK>};
}
const FamilyOps FAMILY_OPS[] = {make_family_ops<false>(), make_family_ops<true>()};  // [has_block]

int upload_state(brs_handle* h, const std::vector<double>& d, const std::vector<float>& f, const std::vector<int>& ii) {
  BRS_HIP_TRY(h, hipMemcpy(h->d, d.data(), d.size() * sizeof(double), hipMemcpyHostToDevice));
  BRS_HIP_TRY(h, hipMemcpy(h->f, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice));
  BRS_HIP_TRY(h, hipMemcpy(h->ii, ii.data(), ii.size() * sizeof(int), hipMemcpyHostToDevice));
  return BRS_OK;
}
// the state accessors: copy the state to the host, let `edit(d, f, ii, N)` read or change the copy, copy it back if `write`
template <class Edit> int state_roundtrip(brs_handle* h, const char* who, bool write, Edit edit) {
  if (!h) return BRS_ERR_STATE;
  DeviceGuard g(h->device);
  if (!g.ok) return fail(h, BRS_ERR_HIP, std::string(who) + ": hipSetDevice failed");
  std::vector<double> d(h->nd); std::vector<float> f(h->nf); std::vector<int> ii(h->ni);
  BRS_HIP_TRY(h, hipDeviceSynchronize());
  BRS_HIP_TRY(h, hipMemcpy(d.data(), h->d, h->nd * sizeof(double), hipMemcpyDeviceToHost));
  BRS_HIP_TRY(h, hipMemcpy(f.data(), h->f, h->nf * sizeof(float), hipMemcpyDeviceToHost));
  BRS_HIP_TRY(h, hipMemcpy(ii.data(), h->ii, h->ni * sizeof(int), hipMemcpyDeviceToHost));
  edit(d.data(), f.data(), ii.data(), (size_t)h->N);
  return write ? upload_state(h, d, f, ii) : BRS_OK;
}

}  // namespace

extern "C" {

int brs_sizes(int32_t variant, int32_t* nq, int32_t* nv, int32_t* nobs, int32_t* nact) {
  if (!host::known_variant(variant)) return BRS_ERR_ARG;
  const FamilyOps* ops = &FAMILY_OPS[host::has_block(variant)];
  if (nq) *nq = ops->nq;
  if (nv) *nv = ops->nv;
  if (nobs) *nobs = 6;
  if (nact) *nact = 2;
  return BRS_OK;
}

int brs_create(const brs_config* cfg, brs_handle** out) {
  if (!cfg || !out) return fail<brs_handle>(nullptr, BRS_ERR_ARG, "brs_create: null argument");
  *out = nullptr;
  if (!host::known_variant(cfg->variant)) return fail<brs_handle>(nullptr, BRS_ERR_ARG, "brs_create: unknown variant");
  if (cfg->num_envs <= 0) return fail<brs_handle>(nullptr, BRS_ERR_ARG, "brs_create: num_envs must be > 0");
  if ((cfg->flags & BRS_FLAG_NOISE_ON) && (cfg->flags & BRS_FLAG_NOISE_OFF))
    return fail<brs_handle>(nullptr, BRS_ERR_ARG, "brs_create: NOISE_ON and NOISE_OFF are exclusive");
  int bt = cfg->block_threads > 0 ? cfg->block_threads : 64;
  if (bt % 64 != 0 || bt > 256) return fail<brs_handle>(nullptr, BRS_ERR_ARG, "brs_create: block_threads must be 64, 128, 192 or 256");
  std::string why;
  if (const int rc = host::check_device(cfg->device, "brs_create", &why)) return fail<brs_handle>(nullptr, rc, why);
  brs_handle* h = new brs_handle();
  h->N = cfg->num_envs; h->device = cfg->device; h->bt = bt;
  h->ops = &FAMILY_OPS[host::has_block(cfg->variant)]; h->blk = host::has_block(cfg->variant);
  int noise = (cfg->flags & BRS_FLAG_NOISE_ON) ? 1 : ((cfg->flags & BRS_FLAG_NOISE_OFF) ? 0 : -1);
  h->P = make_params<float>(cfg->variant, cfg->flags & BRS_FLAG_AUTO_RESET, noise, cfg->max_episode_steps, cfg->substeps,
                            cfg->timestep, cfg->seed, cfg->env_index_base);
  DeviceGuard g(h->device);
  size_t N = (size_t)h->N;
  h->nd = h->ops->ND * N; h->nf = h->ops->NF * N; h->ni = h->ops->NI * N;
  auto bail = [&](const std::string& m) { std::string mm = m; brs_destroy(h); return fail<brs_handle>(nullptr, BRS_ERR_HIP, mm); };
  if (!g.ok) return bail("brs_create: hipSetDevice failed");
  // + 7 fp64 scratch columns addressed by lane slot (accessor pose parked during the last substep, brs_state.hpp: LaneIndex)
  if (hipMalloc(&h->d, (h->nd + 7 * N) * sizeof(double)) != hipSuccess) return bail("brs_create: hipMalloc(fp64 state) failed");
  if (hipMalloc(&h->f, h->nf * sizeof(float)) != hipSuccess) return bail("brs_create: hipMalloc(fp32 state) failed");
  if (hipMalloc(&h->ii, (h->ni + 2 * N + GROUP_WORDS) * sizeof(int)) != hipSuccess) return bail("brs_create: hipMalloc(int state) failed");
  std::vector<double> d(h->nd); std::vector<float> f(h->nf); std::vector<int> ii(h->ni);
  h->ops->init_state(d.data(), f.data(), ii.data(), N, cfg->seed, cfg->env_index_base);
  if (upload_state(h, d, f, ii) != BRS_OK) return bail("brs_create: initial upload failed: " + h->err);
  {  // lane map = identity until the first regrouping (always read by the Env03 step kernel)
    std::vector<int> id(2 * N, 0);
    for (size_t k = 0; k < N; k++) id[k] = (int)k;
    if (hipMemcpy(h->perm(), id.data(), 2 * N * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return bail("brs_create: lane map init failed");
    if (hipMemset(h->counters(), 0, GROUP_WORDS * sizeof(int)) != hipSuccess) return bail("brs_create: counter init failed");
    h->grouping = h->blk && !(cfg->flags & BRS_FLAG_NO_LANE_GROUPING);
    int cus = 0;  // CDNA: 4 SIMDs per CU.  More waves than SIMDs are back-filled: diluting would only add work
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess) return bail("brs_create: CU count query failed");
    h->wheel_cap = (N + LM_WAVE - 1) / LM_WAVE <= 4 * (size_t)cus ? (unsigned)LM_RARE_CAP : (unsigned)LM_WAVE;
    h->folded = !(cfg->timestep > 0 && cfg->timestep != 2e-5) && !std::getenv("BRS_NO_FOLD");
    h->occ2 = !h->blk && std::getenv("BRS_ENV01_OCC1") == nullptr;
  }
  // dynamic LDS above the 64 KiB default needs the attribute (Env03, 256-thread blocks: 256 x 160 words = 160 KiB, all of a CU's LDS)
  size_t lb = lds_bytes(h);
  hipError_t ea = hipSuccess;
  auto want = [&](const void* fn) { if (ea == hipSuccess) ea = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lb); };
  if (!step_kernel_of(h)) return bail("brs_create: no step kernel for this variant");
  for (const StepKernel& k : STEP_KERNELS)
    if (k.blk == h->blk) want(k.fn);
  want(h->ops->physics_kernel);
  if (ea != hipSuccess) return bail(std::string("brs_create: hipFuncSetAttribute: ") + hipGetErrorString(ea));
  *out = h;
  return BRS_OK;
}

int brs_destroy(brs_handle* h) {
  if (!h) return BRS_ERR_STATE;
  {
    DeviceGuard g(h->device);
    if (h->d) (void)hipFree(h->d);
    if (h->f) (void)hipFree(h->f);
    if (h->ii) (void)hipFree(h->ii);
  }
  delete h;
  return BRS_OK;
}

const char* brs_last_error(const brs_handle* h) { return host::last_error(h); }

int brs_reset(brs_handle* h, const uint8_t* mask_dev, float* obs_dev, void* stream) {
  if (!h) return BRS_ERR_STATE;
  if (!obs_dev) return fail(h, BRS_ERR_ARG, "brs_reset: obs_dev is null");
  DeviceGuard g(h->device);
  if (!g.ok) return fail(h, BRS_ERR_HIP, "brs_reset: hipSetDevice failed");
  void* args[] = {&h->P, &h->N, &h->d, &h->f, &h->ii, &mask_dev, &obs_dev};
  return launch_per_env(h, h->ops->reset_kernel, args, 0, stream);
}

int brs_step(brs_handle* h, const float* actions_dev, float* obs_dev, float* reward_dev, uint8_t* terminated_dev,
             uint8_t* truncated_dev, float* terminal_obs_dev, void* stream) {
  if (!h) return BRS_ERR_STATE;
  if (!actions_dev || !obs_dev || !reward_dev || !terminated_dev || !truncated_dev)
    return fail(h, BRS_ERR_ARG, "brs_step: null buffer");
  DeviceGuard g(h->device);
  if (!g.ok) return fail(h, BRS_ERR_HIP, "brs_step: hipSetDevice failed");
  void* args[] = {&h->P, &h->N, &h->d, &h->f, &h->ii, &actions_dev, &obs_dev, &reward_dev, &terminated_dev, &truncated_dev, &terminal_obs_dev};
  // a step launch that failed left no bucket counts: the grouping kernel must not run on them (its output would not be a
  // permutation, and later steps would skip or double envs)
  if (const int rc = launch_per_env(h, step_kernel_of(h)->fn, args, lds_bytes(h), stream)) return rc;
  if (h->blk) {  // lanes of the NEXT step; without grouping the counts the step kernel left are just cleared
    if (h->grouping) {
      hipLaunchKernelGGL(brs_group_kernel, dim3((h->N + GROUP_ENVS - 1) / GROUP_ENVS), dim3(GROUP_THREADS), 0, (hipStream_t)stream, h->N, h->keys(), h->perm(), h->counters(), h->wheel_cap);
      BRS_HIP_TRY(h, hipGetLastError());
    } else
      BRS_HIP_TRY(h, hipMemsetAsync(h->counters(), 0, GROUP_WORDS * sizeof(int), (hipStream_t)stream));
  }
  return BRS_OK;
}

int brs_physics(brs_handle* h, const float* ctrl_dev, int32_t nsub, void* stream) {
  if (!h) return BRS_ERR_STATE;
  if (!ctrl_dev || nsub < 0) return fail(h, BRS_ERR_ARG, "brs_physics: bad argument");
  DeviceGuard g(h->device);
  if (!g.ok) return fail(h, BRS_ERR_HIP, "brs_physics: hipSetDevice failed");
  void* args[] = {&h->P, &h->N, &h->d, &h->f, &h->ii, &ctrl_dev, &nsub};
  return launch_per_env(h, h->ops->physics_kernel, args, lds_bytes(h), stream);
}

int brs_get_state(brs_handle* h, double* qpos, double* qvel, double* warm, double* time) {
  return state_roundtrip(h, "brs_get_state", false, [&](double* d, float* f, int*, size_t N) { h->ops->get_state(d, f, N, qpos, qvel, warm, time); });
}
int brs_set_state(brs_handle* h, const double* qpos, const double* qvel, const double* warm, const double* time) {
  return state_roundtrip(h, "brs_set_state", true, [&](double* d, float* f, int* ii, size_t N) {
    h->ops->set_state(d, f, N, qpos, qvel, warm, time);
    h->ops->mark_bad_start(d, f, ii, N);
  });
}
int brs_get_aux(brs_handle* h, double* aux) {
  if (!aux) return BRS_ERR_ARG;
  return state_roundtrip(h, "brs_get_aux", false, [&](double* d, float* f, int* ii, size_t N) { h->ops->get_aux(d, f, ii, N, aux); });
}
int brs_set_aux(brs_handle* h, const double* aux) {
  if (!aux) return BRS_ERR_ARG;
  return state_roundtrip(h, "brs_set_aux", true, [&](double* d, float* f, int* ii, size_t N) { h->ops->set_aux(d, f, ii, N, aux); });
}
int brs_get_xpose(brs_handle* h, double* xquat, double* xpos) {
  return state_roundtrip(h, "brs_get_xpose", false, [&](double* d, float*, int*, size_t N) { h->ops->get_xpose(d, N, xquat, xpos); });
}
int brs_set_xpose(brs_handle* h, const double* xquat, const double* xpos) {
  return state_roundtrip(h, "brs_set_xpose", true, [&](double* d, float*, int*, size_t N) { h->ops->set_xpose(d, N, xquat, xpos); });
}

int brs_get_lane_map(brs_handle* h, int32_t* perm, uint8_t* keys, uint32_t* counters, uint32_t* wheel_cap) {
  if (!h) return BRS_ERR_STATE;
  if (!h->blk) return fail(h, BRS_ERR_ARG, "brs_get_lane_map: the Env01 family has no lane map");
  DeviceGuard g(h->device);
  if (!g.ok) return fail(h, BRS_ERR_HIP, "brs_get_lane_map: hipSetDevice failed");
  BRS_HIP_TRY(h, hipDeviceSynchronize());
  const size_t N = (size_t)h->N;
  if (perm) BRS_HIP_TRY(h, hipMemcpy(perm, h->perm(), N * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (keys) BRS_HIP_TRY(h, hipMemcpy(keys, h->keys(), N * sizeof(uint8_t), hipMemcpyDeviceToHost));
  if (counters) BRS_HIP_TRY(h, hipMemcpy(counters, h->counters(), (2 * NBUCKET + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (wheel_cap) *wheel_cap = h->wheel_cap;  // the value brs_step passes to brs_group_kernel
  return BRS_OK;
}

int64_t brs_step_bytes_per_env(const brs_handle* h) {
  if (!h) return 0;
  // state read + state written + action (8) + obs (24) + terminal obs (24) + reward (4) + two flags (2)
  return (int64_t)(2 * h->ops->bytes_per_env + 8 + 24 + 24 + 4 + 2);
}
#if defined(BRS_TIMING)
// diagnostic builds only: read and clear the per-phase cycle sums
int brs_debug_waves(unsigned long long* out16384) {
  return hipMemcpyFromSymbol(out16384, HIP_SYMBOL(brs_dbg_wave), 16 * 1024 * sizeof(unsigned long long)) == hipSuccess ? BRS_OK : BRS_ERR_HIP;
}
int brs_debug_counters(unsigned long long* out16) {
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(brs_dbg), 16 * sizeof(unsigned long long)) != hipSuccess) return BRS_ERR_HIP;
  unsigned long long z[16] = {0};
  if (hipMemcpyToSymbol(HIP_SYMBOL(brs_dbg), z, sizeof z) != hipSuccess) return BRS_ERR_HIP;
  return BRS_OK;
}
#endif
#ifndef BRS_BUILD_ID
#define BRS_BUILD_ID "unstamped"
#endif
const char* brs_build_id(void) { return BRS_BUILD_ID; }
const char* brs_step_kernel_name(const brs_handle* h) {
  if (!h) return "";
  // the instantiation brs_step launches, spelled as rocprofv3 prints it
  static thread_local char name[64];
  const StepKernel* k = step_kernel_of(h);
  if (k->occ2) std::snprintf(name, sizeof name, "brs_step_kernel_occ2<%d>", k->variant);
  else std::snprintf(name, sizeof name, "brs_step_kernel<%s, %d>", k->blk ? "true" : "false", k->variant);
  return name;
}

}  // extern "C"
