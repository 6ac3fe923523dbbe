// brs_offpolicy.hpp -- the DDPG data path of include/brs_policy.h, the part shared by the HIP kernels
// (brs_offpolicy.hip) and the host build the CPU tests compare with the fp64 numpy restatement (tests/offpolicyhost): the
// shapes of the two networks, the per-row tails (exploration noise, warm-up uniform, clip, TD combine), the replay buffer's
// row rule and index map, and a plain-loop forward of the 3-layer networks.  Compiles with g++.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/brs.h"
#include "../../include/brs_policy.h"
#include "brs_core.hpp"  // philox4x32_10, BRS_HD
#include "brs_nan.hpp"   // the selects that keep a NaN

namespace brs {
namespace offpolicy {

constexpr int OBS = BRS_POLICY_OBS, ACT = BRS_POLICY_ACT;
// SB3's TD3Policy with the reference's net_arch = dict(pi=[300, 200], qf=[200, 150])
struct Actor { static constexpr int IN = OBS, H1 = 300, H2 = 200, OUT = ACT; static constexpr bool TANH = true; };
struct Critic { static constexpr int IN = OBS + ACT, H1 = 200, H2 = 150, OUT = 1; static constexpr bool TANH = false; };
template <class N> constexpr int nparam() { return N::H1 * N::IN + N::H1 + N::H2 * N::H1 + N::H2 + N::OUT * N::H2 + N::OUT; }
static_assert(nparam<Actor>() == BRS_DDPG_NACTOR && nparam<Critic>() == BRS_DDPG_NCRITIC, "include/brs_policy.h");
// BRS_ARCH_SAC_DEFAULT: SB3's default net_arch = [256, 256]; eight 32-unit tiles per layer, no padded unit
struct Critic256 { static constexpr int IN = OBS + ACT, H1 = 256, H2 = 256, OUT = 1; static constexpr bool TANH = false; };
static_assert(nparam<Critic256>() == BRS_SAC256_NCRITIC, "include/brs_policy.h");
// offsets of the blocks of a flat parameter vector: W1[H1][IN] b1[H1] W2[H2][H1] b2[H2] W3[OUT][H2] b3[OUT]
template <class N> struct Offsets {
  static constexpr int W1 = 0, B1 = W1 + N::H1 * N::IN, W2 = B1 + N::H1, B2 = W2 + N::H2 * N::H1, W3 = B2 + N::H2, B3 = W3 + N::OUT * N::H2;
};
// the hidden widths as the matrix-core kernels hold them, padded to the 32-unit tile (brs_ddpg_tile.hpp); here, without device code,
// so that the sizing table of a learner handle (brs_ddpg_learner.hpp, brs_sac.hpp) compiles with g++
constexpr int pad32(int x) { return (x + 31) / 32 * 32; }
template <class N> struct Padded { static constexpr int H1P = pad32(N::H1), H2P = pad32(N::H2); };

constexpr uint32_t TAG_ACT = BRS_DDPG_TAG_ACT, TAG_SAMPLE = BRS_DDPG_TAG_SAMPLE, TAG_TD3_NOISE = BRS_TD3_TAG_NOISE;

// the Philox block of env gid at `step` (brs_ddpg_act) and of sample j of `draw` (brs_replay_sample)
BRS_HD void act_block(uint64_t seed, int64_t gid, uint32_t step, uint32_t* o) {
  philox4x32_10(step, TAG_ACT, (uint32_t)((uint64_t)gid & 0xffffffffu), (uint32_t)((uint64_t)gid >> 32), (uint32_t)(seed & 0xffffffffu),
                (uint32_t)(seed >> 32), o);
}
BRS_HD void sample_block(uint64_t seed, uint32_t draw, uint32_t j, uint32_t* o) {
  philox4x32_10(draw, TAG_SAMPLE, j, 0u, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), o);
}

// ... and of row j of `draw` of brs_td3_td_target's smoothing noise
BRS_HD void td3_noise_block(uint64_t seed, uint32_t draw, uint32_t j, uint32_t* o) {
  philox4x32_10(draw, TAG_TD3_NOISE, j, 0u, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), o);
}

// Box-Muller on two 24-bit uniforms in (0, 1): the arithmetic of brs_policy_act, on words 0 and 1
BRS_HD void normal_pair(uint32_t w0, uint32_t w1, float* z) {
  const float u1 = ((float)(w0 >> 8) + 0.5f) * (1.0f / 16777216.0f), u2 = ((float)(w1 >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float r = sqrtf(-2.0f * logf(u1)), th = 6.283185307179586f * u2;
  z[0] = r * cosf(th); z[1] = r * sinf(th);
}

// warm-up action component from word 2 or 3: ((w >> 8) - 2^23) / 2^23, one of the 2^24 multiples of 2^-23 in [-1, 1 - 2^-23];
// every step is exact in fp32
BRS_HD float uniform_action(uint32_t w) { return (float)((int32_t)(w >> 8) - 8388608) * (1.0f / 8388608.0f); }

// SB3 _sample_action: clip(mean + sigma z, -1, 1); a product and a sum, on the device as on the host; a NaN mean stays a NaN
// (np.clip), so that the simulator's bad-state guard sees it
BRS_HD float noisy_action(float mean, float sigma, float z) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float p = sigma * z;
  const float a = mean + p;
  return clip_keep_nan(a, -1.0f, 1.0f);
}

// the per-row tail of brs_ddpg_act: mean[2] is the actor's output (ignored when random != 0)
BRS_HD void act_tail(uint64_t seed, int64_t gid, uint32_t step, float sigma, int random, const float* mean_in, float* action, float* mean,
                     float* noise) {
  uint32_t o[4];
  act_block(seed, gid, step, o);
  normal_pair(o[0], o[1], noise);
  for (int k = 0; k < ACT; k++) {
    mean[k] = random ? uniform_action(o[2 + k]) : mean_in[k];
    action[k] = noisy_action(mean[k], sigma, noise[k]);
  }
}

// y = r + (1 - done) gamma Q'(s', pi'(s')); a row with done != 0 returns r itself, bit for bit, whatever Q' is: where SB3
// computes 0 * NaN for a poisoned next_obs or target network, this returns the reward
BRS_HD float td_combine(float reward, uint8_t done, float gamma, float q_next) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (done) return reward;
  const float g = gamma * q_next;
  return reward + g;
}

// TD3's target policy smoothing: a' = clamp(mean + clamp(policy_noise z, -clip, clip), -1, 1); with
// policy_noise == 0 the target actor's output comes back as it is (it lies in [-1, 1]; -0 + mean is mean)
BRS_HD float smoothed_action(float mean, float policy_noise, float clip, float z) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float p = policy_noise * z;
  p = clip_keep_nan(p, -clip, clip);
  const float a = mean + p;
  return clip_keep_nan(a, -1.0f, 1.0f);
}
// the per-row tail of brs_td3_td_target before the two critics: z[2] from the row's Philox block, next_action[2] from mean[2]
BRS_HD void td3_action_tail(uint64_t seed, uint32_t draw, uint32_t row, float policy_noise, float clip, const float* mean, float* next_action,
                            float* z) {
  uint32_t o[4];
  td3_noise_block(seed, draw, row, o);
  normal_pair(o[0], o[1], z);
  for (int k = 0; k < ACT; k++) next_action[k] = smoothed_action(mean[k], policy_noise, clip, z[k]);
}
// ... and after them: clipped double-Q (a NaN from either critic stays, as torch.minimum), then td_combine
BRS_HD float td3_combine(float reward, uint8_t done, float gamma, float q1, float q2) { return td_combine(reward, done, gamma, min_keep_nan(q1, q2)); }
// the argument rules of brs_td3_td_target that need no device: 0 or the text after "brs_td3_td_target: "
inline const char* td3_target_argument_error(const void* actor_t, const void* critics_t, int32_t m, const void* next_obs, const void* reward,
                                             const void* done, float policy_noise, float noise_clip, const void* y) {
  if (!actor_t || !critics_t || !next_obs || !reward || !done || !y) return "null argument";
  if (m < 1) return "m must be at least 1";
  if (!(policy_noise >= 0.0f) || isinf(policy_noise)) return "policy_noise must be finite and >= 0";
  if (!(noise_clip >= 0.0f) || isinf(noise_clip)) return "noise_clip must be finite and >= 0";
  return nullptr;
}

// replay buffer, one env of one added step: which observation is the transition's successor, and its done flag
BRS_HD bool next_is_terminal_obs(uint8_t terminated, uint8_t truncated) { return (terminated | truncated) != 0; }
BRS_HD uint8_t stored_done(uint8_t terminated) { return terminated ? 1 : 0; }  // a time-limit end bootstraps, a fall does not

// sample j of a draw: two independent uniform integers from words 0 and 1, row in [0, size), env in [0, n)
BRS_HD void sample_cell(uint32_t w0, uint32_t w1, int32_t size, int32_t n, int32_t* row, int32_t* env) {
  *row = (int32_t)(((uint64_t)w0 * (uint64_t)(uint32_t)size) >> 32);
  *env = (int32_t)(((uint64_t)w1 * (uint64_t)(uint32_t)n) >> 32);
}

BRS_HD float tanh_(float x) {  // 1 - 2 / (e^(2x) + 1): e = +inf -> 1, e = 0 -> -1; absolute error ~1e-7
  const float e = expf(2.0f * x);
  return 1.0f - 2.0f / (e + 1.0f);
}

// the host's forward of one row: plain loops in fp32, k ascending (the matrix cores walk k in another order: the two
// agree to rounding, not bit for bit)
template <class N> inline void forward_row(const float* w, const float* x, float* out) {
  using O = Offsets<N>;
  float h1[N::H1], h2[N::H2];
  for (int u = 0; u < N::H1; u++) {
    float s = w[O::B1 + u];
    for (int k = 0; k < N::IN; k++) s = fmaf(w[O::W1 + u * N::IN + k], x[k], s);
    h1[u] = relu_keep_nan(s);
  }
  for (int u = 0; u < N::H2; u++) {
    float s = w[O::B2 + u];
    for (int k = 0; k < N::H1; k++) s = fmaf(w[O::W2 + u * N::H1 + k], h1[k], s);
    h2[u] = relu_keep_nan(s);
  }
  for (int u = 0; u < N::OUT; u++) {
    float s = 0.0f;
    for (int k = 0; k < N::H2; k++) s = fmaf(w[O::W3 + u * N::H2 + k], h2[k], s);
    s += w[O::B3 + u];
    out[u] = N::TANH ? tanh_(s) : s;
  }
}

}  // namespace offpolicy
}  // namespace brs
