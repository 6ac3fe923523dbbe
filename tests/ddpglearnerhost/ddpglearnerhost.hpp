// Host build of the DDPG learner's kernel source (balance_robot_mujoco_rl_amd/csrc/brs_ddpg_learner.hpp): the loss heads, the
// tanh' factor, the gate rule, the statistics, Adam plus Polyak, the split of the sample axis and the plain-loop forward/backward on host arrays, behind the
// argument rules of the C ABI (include/brs_policy.h: brs_ddpg_learner_*).  Shared by ddpglearnerhost.cpp (a library for
// tests/test_ddpg_learner_cpu.py) and ddpglearnerhost_main.cpp (a program of its own, for the sanitizers).
#pragma once
#include <stddef.h>

#include "brs_ddpg_learner.hpp"

namespace ddpglearnerhost {

using namespace brs::ddpg_learner;

inline int critic_grad(const float* critic, int m, const float* obs, const float* act, const float* y, float* grad) {
  if (!critic || !obs || !act || !y || !grad || m < 1) return BRS_ERR_ARG;
  critic_grad_host(critic, m, obs, act, y, grad);
  return BRS_OK;
}

inline int actor_grad(const float* actor, const float* critic, int m, const float* obs, float* grad) {
  if (!actor || !critic || !obs || !grad || m < 1) return BRS_ERR_ARG;
  actor_grad_host(actor, critic, m, obs, grad);
  return BRS_OK;
}

inline int apply(int n_param, float* params, const float* grad, float* m, float* v, float* target, const brs_adam_config* cfg, int64_t step,
                 float tau) {
  if (apply_argument_error(n_param, params, grad, m, v, cfg, step, tau)) return BRS_ERR_ARG;
  apply_host(n_param, params, grad, m, v, target, *cfg, step, tau);
  return BRS_OK;
}

// brs_ddpg_learner.hpp's sample_split, the split of the sample axis that launch_weight_kernels of brs_ddpg_learner.hip uses, for one m
// (out[3] = mp, span, nsplit) and checked over every m of [m_lo, m_hi]:
//   bit 0  span is no multiple of 128          bit 3  a launched split holds no real row: (nsplit - 1) span >= m
//   bit 1  nsplit is outside [1, MAX_SPLIT]    bit 4  nsplit == 1 is not the same as mp < 512
//   bit 2  the splits do not cover mp          bit 5  nsplit partial rows (single or twin) do not fit the handle's allocation
//   bit 6  mp is not m padded to 128
// -> the number of m that break a rule; *first_bad, *first_mask: the smallest such m and its bits (0, 0 if none)
inline void split_of(int m, int* out) {
  const SampleSplit s = sample_split(m);
  out[0] = s.mp; out[1] = s.span; out[2] = s.nsplit;
}
inline unsigned split_faults(int m) {
  const SampleSplit s = sample_split(m);
  const long long mp = s.mp, span = s.span, n = s.nsplit;
  unsigned bad = 0;
  if (span < 128 || span % 128 != 0) bad |= 1u;
  if (n < 1 || n > MAX_SPLIT) bad |= 2u;
  if (n * span < mp) bad |= 4u;
  if ((n - 1) * span >= m) bad |= 8u;
  if ((n == 1) != (mp < 512)) bad |= 16u;
  // a single call writes rows of at most row_len<Actor>() floats, the twin call rows of TWIN_LEN, each at a stride of its own length
  if ((size_t)n * (size_t)row_len<Actor>() > partial_floats(false) || (size_t)n * (size_t)row_len<Critic>() > partial_floats(false) ||
      (size_t)n * (size_t)TWIN_LEN > partial_floats(true) || (size_t)n * (size_t)row_len<Actor>() > partial_floats(true))
    bad |= 32u;
  if (mp < m || mp - m > 127 || mp % 128 != 0) bad |= 64u;
  return bad;
}
inline long long split_sweep(int m_lo, int m_hi, int* first_bad, unsigned* first_mask) {
  long long count = 0;
  *first_bad = 0; *first_mask = 0u;
  for (long long m = m_lo; m <= m_hi; m++) {
    const unsigned bad = split_faults((int)m);
    if (bad && !count++) { *first_bad = (int)m; *first_mask = bad; }
  }
  return count;
}

}  // namespace ddpglearnerhost
