// brs_offpolicy.hip -- the DDPG data path of include/brs_policy.h: actor with exploration noise, critic, TD
// target from the two target networks, replay buffer add and fused sample, as HIP kernels for gfx950; and TD3's target with
// smoothing noise and two target critics; and SAC's squashed-Gaussian actor and its entropy target.
//
// One forward routine (forward_tile, brs_ddpg_tile.hpp, shared with brs_ddpg_learner.hip) serves brs_ddpg_act, brs_ddpg_q and brs_ddpg_td_target.  It is brs_policy.hip's scheme for
// wider layers: fp32 on the MATRIX cores (v_mfma_f32_32x32x2_f32: exact fp32 products, a k-ordered fma chain), the product
// computed TRANSPOSED, D[unit][row] = sum_k W[unit][k] h[k][row], so that the accumulator of one layer (lane l holds 16 units of
// ITS row l % 32 per M-tile) is, after the ReLU, the B operand of the next: hidden activations never leave their registers, no
// LDS round trip and nothing in HBM.  A wave owns 32 rows; the widths are padded to the 32-unit tile (300 -> 320, 200 -> 224,
// 150 -> 160): 10 + 7 accumulator tiles = 272 registers for the actor, which is why a wave has one N-tile and a workgroup of
// four waves (one per SIMD) 128 rows.  The first layer (K = 6 / 8), the biases and the output layer live in LDS for the whole
// kernel; the second layer (200 x 300 = 240 KB) does not fit and is staged in K-chunks of 32 input units -- one chunk is
// what one M-tile of the first layer feeds -- [H2 padded][33] words each (row stride 33: the 32 lanes of a half hit 32 banks),
// double-buffered: the next chunk is fetched into registers before the matrix instructions of this one and written to the other
// buffer after them, one barrier per chunk.  PADDING: padded units get zero weight rows, zero weight columns and zero bias in
// the LDS image (written, not assumed), so a padded hidden unit is ReLU(0) = 0 and meets a zero column; rows past n are
// computed on zero inputs (the matrix instructions need whole waves) and not stored.
// Architectures: the SAC act, the SAC target and the critic's forward are templates over the networks of the handle's
// architecture; SB3's default [256, 256] is eight tiles per layer with no padded unit (LDS image 80,912 bytes: two workgroups per CU).
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/brs.h"
#include "../../include/brs_policy.h"
#include "brs_host.hpp"
#include "brs_ddpg_tile.hpp"
#include "brs_offpolicy.hpp"
#include "brs_sac.hpp"

namespace {

using namespace brs::offpolicy;
using namespace brs::ddpg_tile;
using brs::sac::SacActor;
// (the SAC actor's image is the DDPG actor's with two more rows of the output layer)
static_assert(Tile<SacActor>::L_SIZE == Tile<Actor>::L_SIZE + 2 * Tile<Actor>::H2P, "LDS");

// row i's ACT words of an output that may be absent
__device__ __forceinline__ void store_row(float* __restrict__ dst, const int i, const float (&v)[ACT]) {
  if (!dst) return;
#pragma unroll
  for (int k = 0; k < ACT; k++) dst[(size_t)ACT * i + k] = v[k];
}

__global__ void __launch_bounds__(THREADS) ddpg_act_kernel(const float* __restrict__ actor, const int n, const float* __restrict__ obs,
                                                           const uint64_t seed, const int64_t gid_base, const uint32_t step, const float sigma,
                                                           float* __restrict__ action, float* __restrict__ mean, float* __restrict__ noise) {
  __shared__ float L[Tile<Actor>::L_SIZE];
  const int i = tile_row();
  float xb[OBS / 2], mu[ACT];
  load_obs_operands(obs, n, i, xb);
  forward_tile<Actor>(actor, L, xb, mu);  // (no lane leaves before the matrix instructions: they need the whole wave)
  if (i >= n || !finishes_row()) return;
  float a[ACT], m[ACT], z[ACT];
  act_tail(seed, gid_base + (int64_t)i, step, sigma, 0, mu, a, m, z);
  store_row(action, i, a);
  store_row(mean, i, m);
  store_row(noise, i, z);
}

// the learning_starts phase: no network
__global__ void __launch_bounds__(256) ddpg_random_kernel(const int n, const uint64_t seed, const int64_t gid_base, const uint32_t step,
                                                          const float sigma, float* __restrict__ action, float* __restrict__ mean,
                                                          float* __restrict__ noise) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float none[ACT] = {0.0f, 0.0f};
  float a[ACT], m[ACT], z[ACT];
  act_tail(seed, gid_base + (int64_t)i, step, sigma, 1, none, a, m, z);
  store_row(action, i, a);
  store_row(mean, i, m);
  store_row(noise, i, z);
}

template <class Q> __global__ void __launch_bounds__(THREADS) ddpg_q_kernel(const float* __restrict__ critic, const int n, const float* __restrict__ obs,
                                                                           const float* __restrict__ act, float* __restrict__ q) {
  __shared__ float L[Tile<Q>::L_SIZE];
  const int i = tile_row();
  float xb[(OBS + ACT) / 2], v[1];
  load_obs_operands(obs, n, i, xb);
  xb[OBS / 2] = i < n ? act[(size_t)ACT * i + wave_half()] : 0.0f;
  forward_tile<Q>(critic, L, xb, v);
  if (i < n && finishes_row()) q[i] = v[0];
}

// The three targets are one shape: the actor's forward -> the rule's action -> the forwards of the rule's CRITICS target critics, laid
// back to back -> the rule's combine -> the rule's optional outputs, in one launch; the forwards share the LDS image L one after the
// other.  A Rule names the networks (Pi, Qf, and PiNet / QfNet as forward_tile is to walk them), and holds the call's scalars and,
// between action() and store(), what the row's sample left.  Both halves of a wave compute the row's action: it is the B operand of both.
template <class R> __device__ __forceinline__ void target_body(R rule, float* __restrict__ L, const float* __restrict__ actor,
                                                               const float* __restrict__ critics, const int m, const float* __restrict__ next_obs,
                                                               const float* __restrict__ reward, const uint8_t* __restrict__ done, const float gamma,
                                                               float* __restrict__ y) {
  const int i = tile_row();
  float sb[OBS / 2], out[R::Pi::OUT], a[ACT], q[R::CRITICS];
  load_obs_operands(next_obs, m, i, sb);
  forward_tile<typename R::PiNet>(actor, L, sb, out);
  rule.action(i, out, a);
  const float xb[(OBS + ACT) / 2] = {sb[0], sb[1], sb[2], wave_half() ? a[1] : a[0]};
#pragma unroll
  for (int k = 0; k < R::CRITICS; k++) {
    float v[1];
    forward_tile<typename R::QfNet>(critics + k * nparam<typename R::Qf>(), L, xb, v);
    q[k] = v[0];
  }
  if (i >= m || !finishes_row()) return;
  y[i] = rule.combine(reward[i], done[i], gamma, q);
  rule.store(i, a);
}

// DDPG: the target actor's action as it is, one critic
struct DdpgTarget {
  using Pi = Actor; using Qf = Critic; using PiNet = Actor; using QfNet = Critic;
  static constexpr int CRITICS = 1;
  __device__ __forceinline__ void action(int, const float (&mu)[ACT], float (&a)[ACT]) { a[0] = mu[0]; a[1] = mu[1]; }
  __device__ __forceinline__ float combine(float reward, uint8_t done, float gamma, const float (&q)[1]) const { return td_combine(reward, done, gamma, q[0]); }
  __device__ __forceinline__ void store(int, const float (&)[ACT]) const {}
};
// TD3: smoothing noise and two clamps on the action, the minimum of two critics
struct Td3Target {
  using Pi = Actor; using Qf = Critic; using PiNet = Actor; using QfNet = Critic;
  static constexpr int CRITICS = 2;
  float policy_noise, noise_clip;
  uint64_t seed;
  uint32_t draw;
  float *next_action, *noise;
  float z[ACT];
  __device__ __forceinline__ void action(int i, const float (&mu)[ACT], float (&a)[ACT]) {
    td3_action_tail(seed, draw, (uint32_t)i, policy_noise, noise_clip, mu, a, z);
  }
  __device__ __forceinline__ float combine(float reward, uint8_t done, float gamma, const float (&q)[2]) const {
    return td3_combine(reward, done, gamma, q[0], q[1]);
  }
  __device__ __forceinline__ void store(int i, const float (&a)[ACT]) const { store_row(next_action, i, a); store_row(noise, i, z); }
};
// SAC: the CURRENT actor's sample and logp, the minimum of two target critics, the entropy term with alpha =
// exp(log_ent_coef), the element behind the actor's b3; A: the handle's architecture
template <class A> struct SacTarget {
  using Pi = typename A::Pi; using Qf = typename A::Qf; using PiNet = typename SeriesOf<A>::Pi; using QfNet = typename SeriesOf<A>::Qf;
  static constexpr int CRITICS = 2;
  const float* actor;
  uint64_t seed;
  uint32_t draw;
  float *next_action, *logp, *noise;
  float z[ACT];
  brs::sac::Sample sm;
  __device__ __forceinline__ void action(int i, const float (&out)[Pi::OUT], float (&a)[ACT]) {
    uint32_t o[4];
    brs::sac::sac_row_block(BRS_SAC_TAG_TARGET, seed, draw, (uint32_t)i, o);
    normal_pair(o[0], o[1], z);
    brs::sac::sample(out, z, sm);
    a[0] = sm.a[0]; a[1] = sm.a[1];
  }
  __device__ __forceinline__ float combine(float reward, uint8_t done, float gamma, const float (&q)[2]) const {
    return brs::sac::sac_combine(reward, done, gamma, q[0], q[1], brs::sac::ent_coef_of<Pi>(actor), sm.logp);
  }
  __device__ __forceinline__ void store(int i, const float (&a)[ACT]) const {
    if (logp) logp[i] = sm.logp;
    store_row(next_action, i, a);
    store_row(noise, i, z);
  }
};

__global__ void __launch_bounds__(THREADS) ddpg_td_target_kernel(const float* __restrict__ actor_t, const float* __restrict__ critic_t, const int m,
                                                                 const float* __restrict__ next_obs, const float* __restrict__ reward,
                                                                 const uint8_t* __restrict__ done, const float gamma, float* __restrict__ y) {
  __shared__ float L[lds_floats<Actor, Critic>()];
  target_body(DdpgTarget{}, L, actor_t, critic_t, m, next_obs, reward, done, gamma, y);
}

__global__ void __launch_bounds__(THREADS) td3_td_target_kernel(const float* __restrict__ actor_t, const float* __restrict__ critics_t, const int m,
                                                                const float* __restrict__ next_obs, const float* __restrict__ reward,
                                                                const uint8_t* __restrict__ done, const float gamma, const float policy_noise,
                                                                const float noise_clip, const uint64_t seed, const uint32_t draw,
                                                                float* __restrict__ y, float* __restrict__ next_action, float* __restrict__ noise) {
  __shared__ float L[lds_floats<Actor, Critic>()];
  target_body(Td3Target{policy_noise, noise_clip, seed, draw, next_action, noise}, L, actor_t, critics_t, m, next_obs, reward, done, gamma, y);
}

// SAC's actor: the forward with four outputs, then the per-row tail of brs_sac.hpp; A: the handle's architecture
// 
template <class A> __global__ void __launch_bounds__(THREADS) sac_act_kernel(const float* __restrict__ actor, const int n, const float* __restrict__ obs,
                                                                            const uint64_t seed, const int64_t gid_base, const uint32_t step,
                                                                            const int deterministic, float* __restrict__ action,
                                                                            float* __restrict__ mu, float* __restrict__ log_std,
                                                                            float* __restrict__ noise) {
  using Pi = typename A::Pi;
  __shared__ float L[Tile<Pi>::L_SIZE];
  const int i = tile_row();
  float xb[OBS / 2], out[Pi::OUT];
  load_obs_operands(obs, n, i, xb);
  forward_tile<Pi>(actor, L, xb, out);
  if (i >= n || !finishes_row()) return;
  float a[ACT], m[ACT], ls[ACT], z[ACT];
  brs::sac::sac_act_tail(seed, gid_base + (int64_t)i, step, deterministic, 0, out, a, m, ls, z);
  store_row(action, i, a);
  store_row(mu, i, m);
  store_row(log_std, i, ls);
  store_row(noise, i, z);
}

__global__ void __launch_bounds__(256) sac_random_kernel(const int n, const uint64_t seed, const int64_t gid_base, const uint32_t step,
                                                         float* __restrict__ action, float* __restrict__ mu, float* __restrict__ log_std,
                                                         float* __restrict__ noise) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float none[SacActor::OUT] = {0.0f, 0.0f, 0.0f, 0.0f};
  float a[ACT], m[ACT], ls[ACT], z[ACT];
  brs::sac::sac_act_tail(seed, gid_base + (int64_t)i, step, 0, 1, none, a, m, ls, z);
  store_row(action, i, a);
  store_row(mu, i, m);
  store_row(log_std, i, ls);
  store_row(noise, i, z);
}

template <class A> __global__ void __launch_bounds__(THREADS) sac_td_target_kernel(const float* __restrict__ actor, const float* __restrict__ critics_t,
                                                                                  const int m, const float* __restrict__ next_obs,
                                                                                  const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                                                  const float gamma, const uint64_t seed, const uint32_t draw,
                                                                                  float* __restrict__ y, float* __restrict__ next_action,
                                                                                  float* __restrict__ logp, float* __restrict__ noise) {
  __shared__ float L[lds_floats<typename A::Pi, typename A::Qf>()];
  target_body(SacTarget<A>{actor, seed, draw, next_action, logp, noise}, L, actor, critics_t, m, next_obs, reward, done, gamma, y);
}

// ------------------------------------------------------------------------------------------------ replay buffer
template <int V> struct Vec;
template <> struct Vec<1> { typedef float F; typedef uint8_t B; };
template <> struct Vec<4> { typedef float4 F; typedef uchar4 B; };

// One env step into row `pos` (cell0 = pos * n): thread t moves words V t .. V t + V - 1 of the row of every array that is
// that long.  V = 4 needs n % 4 == 0 and 16-byte aligned pointers (the host side decides); V = 1 takes everything else.
template <int V> __global__ void __launch_bounds__(256) replay_add_kernel(const brs_replay_storage s, const int n, const int64_t cell0,
                                                                           const float* __restrict__ last_obs, const float* __restrict__ action,
                                                                           const float* __restrict__ obs, const float* __restrict__ reward,
                                                                           const uint8_t* __restrict__ term, const uint8_t* __restrict__ trunc,
                                                                           const float* __restrict__ tobs) {
  typedef typename Vec<V>::F F;
  typedef typename Vec<V>::B B;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * OBS / V) return;
  reinterpret_cast<F*>(s.obs + cell0 * OBS)[t] = reinterpret_cast<const F*>(last_obs)[t];
  union { F v; float f[V]; } o, e;
  o.v = reinterpret_cast<const F*>(obs)[t];
  const int env_a = V * t / OBS, env_b = (V * t + V - 1) / OBS;  // the V words belong to at most two envs
  const bool end_a = next_is_terminal_obs(term[env_a], trunc[env_a]), end_b = next_is_terminal_obs(term[env_b], trunc[env_b]);
  if (end_a || end_b) {
    e.v = reinterpret_cast<const F*>(tobs)[t];
#pragma unroll
    for (int j = 0; j < V; j++) o.f[j] = ((V * t + j) / OBS == env_a ? end_a : end_b) ? e.f[j] : o.f[j];
  }
  reinterpret_cast<F*>(s.next_obs + cell0 * OBS)[t] = o.v;
  if (t < n * ACT / V) reinterpret_cast<F*>(s.action + cell0 * ACT)[t] = reinterpret_cast<const F*>(action)[t];
  if (t < n / V) {
    reinterpret_cast<F*>(s.reward + cell0)[t] = reinterpret_cast<const F*>(reward)[t];
    union { B v; uint8_t b[V]; } d;
    d.v = reinterpret_cast<const B*>(term)[t];
#pragma unroll
    for (int j = 0; j < V; j++) d.b[j] = stored_done(d.b[j]);
    reinterpret_cast<B*>(s.done + cell0)[t] = d.v;
  }
}

// Index and gather in one kernel.  Eight lanes per sample, each moving one 8-byte piece (obs 3, next_obs 3, action 1) and the
// eighth the reward, the done byte and the indices: the pieces of consecutive samples are contiguous in the outputs, so a wave's
// stores are runs of 24 / 8 / 4 bytes per sample back to back.  Every lane of a sample computes the same Philox block.
template <bool V2> __global__ void __launch_bounds__(256) replay_sample_kernel(const brs_replay_storage s, const int n, const int size, const int m,
                                                                               const uint64_t seed, const uint32_t draw, const brs_replay_storage out,
                                                                               int32_t* __restrict__ idx) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t j = t >> 3;
  const int part = (int)(t & 7);
  if (j >= m) return;
  uint32_t w[4];
  sample_block(seed, draw, (uint32_t)j, w);
  int32_t row, env;
  sample_cell(w[0], w[1], size, n, &row, &env);
  const int64_t cell = (int64_t)row * n + env;
  if (part == 7) {
    out.reward[j] = s.reward[cell];
    out.done[j] = s.done[cell];
    if (idx) { idx[2 * j] = row; idx[2 * j + 1] = env; }
    return;
  }
  const float* src;
  float* dst;
  if (part < 3) { src = s.obs + cell * OBS + 2 * part; dst = out.obs + j * OBS + 2 * part; }
  else if (part < 6) { src = s.next_obs + cell * OBS + 2 * (part - 3); dst = out.next_obs + j * OBS + 2 * (part - 3); }
  else { src = s.action + cell * ACT; dst = out.action + j * ACT; }
  if (V2) *reinterpret_cast<float2*>(dst) = *reinterpret_cast<const float2*>(src);
  else { dst[0] = src[0]; dst[1] = src[1]; }
}

struct brs_replay { std::string err; };  // the family of the handle-less replay calls: only its error slot exists

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

struct brs_ddpg {
  int device = 0;
  int arch = BRS_ARCH_REFERENCE;  // whose widths the SAC calls and brs_ddpg_q take
  std::string err;
};

using brs::host::DeviceGuard, brs::host::fail, brs::host::launch_on, brs::host::needs_nothing;
using brs::sac::with_arch;

static const char* reference_arch(const brs_ddpg* d) { return BRS_REFERENCE_ARCH_ONLY(d); }
static dim3 row_grid(int32_t n) { return dim3((n + WG_ROWS - 1) / WG_ROWS); }  // workgroups of 4 waves x 32 rows

extern "C" {

static int create_ddpg(const char* who, int32_t device, int32_t arch, brs_ddpg** out) {
  const std::string w(who);
  if (!out) return fail<brs_ddpg>(nullptr, BRS_ERR_ARG, w + ": null argument");
  *out = nullptr;
  if (!brs::sac::known_arch(arch)) return fail<brs_ddpg>(nullptr, BRS_ERR_ARG, w + ": unknown architecture");
  std::string why;
  if (const int rc = brs::host::check_device(device, who, &why)) return fail<brs_ddpg>(nullptr, rc, why);
  brs_ddpg* d = new brs_ddpg();
  d->device = device;
  d->arch = arch;
  *out = d;
  return BRS_OK;
}

int brs_ddpg_create(int32_t device, brs_ddpg** out) { return create_ddpg("brs_ddpg_create", device, BRS_ARCH_REFERENCE, out); }

int brs_ddpg_create_arch(int32_t device, int32_t arch, brs_ddpg** out) { return create_ddpg("brs_ddpg_create_arch", device, arch, out); }

int brs_ddpg_destroy(brs_ddpg* d) {
  if (!d) return BRS_ERR_STATE;
  delete d;
  return BRS_OK;
}

const char* brs_ddpg_last_error(const brs_ddpg* d) { return brs::host::last_error(d); }

int brs_ddpg_act(brs_ddpg* d, const float* actor_dev, int32_t n, const float* obs_dev, uint64_t seed, int64_t env_index_base, uint32_t step,
                 float sigma, int32_t random, float* action_dev, float* mean_dev, float* noise_dev, void* stream) {
  // what needs no handle is checked first (fail() records it in the family's slot when there is none)
  if (n < 1) return fail(d, BRS_ERR_ARG, "brs_ddpg_act: n must be at least 1");
  if (!(sigma >= 0.0f)) return fail(d, BRS_ERR_ARG, "brs_ddpg_act: sigma must be >= 0");
  if (!action_dev || (!random && (!actor_dev || !obs_dev))) return fail(d, BRS_ERR_ARG, "brs_ddpg_act: null argument");
  return launch_on(d, "brs_ddpg_act", reference_arch, [&] {
    if (random)
      hipLaunchKernelGGL(ddpg_random_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, seed, env_index_base, step, sigma,
                         action_dev, mean_dev, noise_dev);
    else
      hipLaunchKernelGGL(ddpg_act_kernel, row_grid(n), dim3(THREADS), 0, (hipStream_t)stream, actor_dev, n, obs_dev, seed, env_index_base, step,
                         sigma, action_dev, mean_dev, noise_dev);
  });
}

int brs_ddpg_q(brs_ddpg* d, const float* critic_dev, int32_t n, const float* obs_dev, const float* act_dev, float* q_dev, void* stream) {
  if (n < 1) return fail(d, BRS_ERR_ARG, "brs_ddpg_q: n must be at least 1");
  if (!critic_dev || !obs_dev || !act_dev || !q_dev) return fail(d, BRS_ERR_ARG, "brs_ddpg_q: null argument");
  return launch_on(d, "brs_ddpg_q", needs_nothing, [&] {
    with_arch(d->arch, [&](auto a) {
      hipLaunchKernelGGL(ddpg_q_kernel<typename decltype(a)::Qf>, row_grid(n), dim3(THREADS), 0, (hipStream_t)stream, critic_dev, n, obs_dev, act_dev,
                         q_dev);
    });
  });
}

int brs_ddpg_td_target(brs_ddpg* d, const float* actor_target_dev, const float* critic_target_dev, int32_t m, const float* next_obs_dev,
                       const float* reward_dev, const uint8_t* done_dev, float gamma, float* y_dev, void* stream) {
  if (m < 1) return fail(d, BRS_ERR_ARG, "brs_ddpg_td_target: m must be at least 1");
  if (!actor_target_dev || !critic_target_dev || !next_obs_dev || !reward_dev || !done_dev || !y_dev)
    return fail(d, BRS_ERR_ARG, "brs_ddpg_td_target: null argument");
  return launch_on(d, "brs_ddpg_td_target", reference_arch, [&] {
    hipLaunchKernelGGL(ddpg_td_target_kernel, row_grid(m), dim3(THREADS), 0, (hipStream_t)stream, actor_target_dev, critic_target_dev, m,
                       next_obs_dev, reward_dev, done_dev, gamma, y_dev);
  });
}

int brs_td3_td_target(brs_ddpg* d, const float* actor_target_dev, const float* critics_target_dev, int32_t m, const float* next_obs_dev,
                      const float* reward_dev, const uint8_t* done_dev, float gamma, float policy_noise, float noise_clip, uint64_t seed,
                      uint32_t draw, float* y_dev, float* next_action_dev, float* noise_dev, void* stream) {
  if (const char* why = td3_target_argument_error(actor_target_dev, critics_target_dev, m, next_obs_dev, reward_dev, done_dev, policy_noise,
                                                  noise_clip, y_dev))
    return fail(d, BRS_ERR_ARG, std::string("brs_td3_td_target: ") + why);
  return launch_on(d, "brs_td3_td_target", reference_arch, [&] {
    hipLaunchKernelGGL(td3_td_target_kernel, row_grid(m), dim3(THREADS), 0, (hipStream_t)stream, actor_target_dev, critics_target_dev, m,
                       next_obs_dev, reward_dev, done_dev, gamma, policy_noise, noise_clip, seed, draw, y_dev, next_action_dev, noise_dev);
  });
}

int brs_sac_act(brs_ddpg* d, const float* actor_dev, int32_t n, const float* obs_dev, uint64_t seed, int64_t env_index_base, uint32_t step,
                int32_t deterministic, int32_t random, float* action_dev, float* mu_dev, float* log_std_dev, float* z_dev, void* stream) {
  if (const char* why = brs::sac::sac_act_argument_error(actor_dev, n, obs_dev, random, action_dev))
    return fail(d, BRS_ERR_ARG, std::string("brs_sac_act: ") + why);
  return launch_on(d, "brs_sac_act", needs_nothing, [&] {
    if (random)
      hipLaunchKernelGGL(sac_random_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, seed, env_index_base, step, action_dev,
                         mu_dev, log_std_dev, z_dev);
    else
      with_arch(d->arch, [&](auto a) {
        hipLaunchKernelGGL(sac_act_kernel<decltype(a)>, row_grid(n), dim3(THREADS), 0, (hipStream_t)stream, actor_dev, n, obs_dev, seed,
                           env_index_base, step, deterministic != 0, action_dev, mu_dev, log_std_dev, z_dev);
      });
  });
}

int brs_sac_td_target(brs_ddpg* d, const float* actor_dev, const float* critics_target_dev, int32_t m, const float* next_obs_dev,
                      const float* reward_dev, const uint8_t* done_dev, float gamma, uint64_t seed, uint32_t draw, float* y_dev,
                      float* next_action_dev, float* logp_dev, float* z_dev, void* stream) {
  if (const char* why = brs::sac::sac_target_argument_error(actor_dev, critics_target_dev, m, next_obs_dev, reward_dev, done_dev, gamma, y_dev))
    return fail(d, BRS_ERR_ARG, std::string("brs_sac_td_target: ") + why);
  return launch_on(d, "brs_sac_td_target", needs_nothing, [&] {
    with_arch(d->arch, [&](auto a) {
      hipLaunchKernelGGL(sac_td_target_kernel<decltype(a)>, row_grid(m), dim3(THREADS), 0, (hipStream_t)stream, actor_dev, critics_target_dev, m,
                         next_obs_dev, reward_dev, done_dev, gamma, seed, draw, y_dev, next_action_dev, logp_dev, z_dev);
    });
  });
}

const char* brs_replay_last_error(void) { return brs::host::last_error<brs_replay>(nullptr); }

static int replay_fail(int code, const std::string& msg) { return fail<brs_replay>(nullptr, code, msg); }

// the checks brs_replay_add and brs_replay_sample share; BRS_OK or the code to return, the text recorded
static int check_storage(const char* who, const brs_replay_storage* s, int32_t n, int32_t cap) {
  const std::string w(who);
  if (!s || !s->obs || !s->next_obs || !s->action || !s->reward || !s->done) return replay_fail(BRS_ERR_ARG, w + ": null storage pointer");
  if (n < 1 || cap < 1) return replay_fail(BRS_ERR_ARG, w + ": n and cap must be at least 1");
  if (n > 0x7fffffff / OBS) return replay_fail(BRS_ERR_ARG, w + ": n * 6 exceeds 2^31 - 1");
  if ((int64_t)cap * (int64_t)n > 0x7fffffffLL) return replay_fail(BRS_ERR_ARG, w + ": cap * n exceeds 2^31 - 1");
  return BRS_OK;
}

int brs_replay_add(int32_t device, const brs_replay_storage* storage, int32_t n, int32_t cap, int32_t pos, const float* last_obs_dev,
                   const float* action_dev, const float* obs_dev, const float* reward_dev, const uint8_t* terminated_dev,
                   const uint8_t* truncated_dev, const float* terminal_obs_dev, void* stream) {
  if (const int rc = check_storage("brs_replay_add", storage, n, cap)) return rc;
  if (pos < 0 || pos >= cap) return replay_fail(BRS_ERR_ARG, "brs_replay_add: pos must be in [0, cap)");
  if (!last_obs_dev || !action_dev || !obs_dev || !reward_dev || !terminated_dev || !truncated_dev || !terminal_obs_dev)
    return replay_fail(BRS_ERR_ARG, "brs_replay_add: null argument");
  std::string why;
  if (const int rc = brs::host::check_device(device, "brs_replay_add", &why)) return replay_fail(rc, why);
  DeviceGuard g(device);
  if (!g.ok) return replay_fail(BRS_ERR_HIP, "brs_replay_add: hipSetDevice failed");
  const int64_t cell0 = (int64_t)pos * n;
  bool v4 = n % 4 == 0;
  for (const void* p : {(const void*)storage->obs, (const void*)storage->next_obs, (const void*)storage->action, (const void*)storage->reward,
                        (const void*)storage->done, (const void*)last_obs_dev, (const void*)action_dev, (const void*)obs_dev, (const void*)reward_dev,
                        (const void*)terminated_dev, (const void*)terminal_obs_dev})
    v4 = v4 && aligned(p, 16);
  if (v4)
    hipLaunchKernelGGL(replay_add_kernel<4>, dim3((n * OBS / 4 + 255) / 256), dim3(256), 0, (hipStream_t)stream, *storage, n, cell0, last_obs_dev,
                       action_dev, obs_dev, reward_dev, terminated_dev, truncated_dev, terminal_obs_dev);
  else
    hipLaunchKernelGGL(replay_add_kernel<1>, dim3((int)(((int64_t)n * OBS + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *storage, n, cell0,
                       last_obs_dev, action_dev, obs_dev, reward_dev, terminated_dev, truncated_dev, terminal_obs_dev);
  if (hipGetLastError() != hipSuccess) return replay_fail(BRS_ERR_HIP, "brs_replay_add: kernel launch failed");
  return BRS_OK;
}

int brs_replay_sample(int32_t device, const brs_replay_storage* storage, int32_t n, int32_t cap, int32_t size, int32_t m, uint64_t seed,
                      uint32_t draw, const brs_replay_storage* out, int32_t* idx_dev, void* stream) {
  if (const int rc = check_storage("brs_replay_sample", storage, n, cap)) return rc;
  if (size < 1 || size > cap) return replay_fail(BRS_ERR_ARG, "brs_replay_sample: size must be in [1, cap]");
  if (m < 1 || m > (1 << 27)) return replay_fail(BRS_ERR_ARG, "brs_replay_sample: m must be in [1, 2^27]");
  if (!out || !out->obs || !out->next_obs || !out->action || !out->reward || !out->done)
    return replay_fail(BRS_ERR_ARG, "brs_replay_sample: null output pointer");
  std::string why;
  if (const int rc = brs::host::check_device(device, "brs_replay_sample", &why)) return replay_fail(rc, why);
  DeviceGuard g(device);
  if (!g.ok) return replay_fail(BRS_ERR_HIP, "brs_replay_sample: hipSetDevice failed");
  bool v2 = true;
  for (const void* p : {(const void*)storage->obs, (const void*)storage->next_obs, (const void*)storage->action, (const void*)out->obs,
                        (const void*)out->next_obs, (const void*)out->action})
    v2 = v2 && aligned(p, 8);
  const dim3 grid((unsigned)(((int64_t)m * 8 + 255) / 256));
  if (v2) hipLaunchKernelGGL(replay_sample_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, *storage, n, size, m, seed, draw, *out, idx_dev);
  else hipLaunchKernelGGL(replay_sample_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, *storage, n, size, m, seed, draw, *out, idx_dev);
  if (hipGetLastError() != hipSuccess) return replay_fail(BRS_ERR_HIP, "brs_replay_sample: kernel launch failed");
  return BRS_OK;
}

}  // extern "C"
