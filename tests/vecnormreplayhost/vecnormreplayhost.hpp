// Host build of the normalising replay sample (balance_robot_mujoco_rl_amd/csrc/brs_vecnorm.hpp):
// vecnorm_replay_sample_kernel of brs_vecnorm.hip restated as loops over workgroup, thread and part on host arrays, with the
// statistics and the configuration of a HostVecNorm (tests/vecnormhost/vecnormhost.hpp) and the cells of brs_offpolicy.hpp.
// Shared by vecnormreplayhost.cpp (a library for tests/vecnorm_replay_cases.py) and vecnormreplayhost_main.cpp (a program of its
// own, for the sanitizers).
#pragma once
#include "../vecnormhost/vecnormhost.hpp"

namespace vecnormreplayhost {

using namespace brs::vecnorm;

// 0, or -1 with *why set: the argument rules of brs_replay_sample_vecnorm
inline int replay_sample(const vecnormhost::HostVecNorm& v, const brs_replay_storage& s, int n, int cap, int size, int m, uint64_t seed,
                         uint32_t draw, const brs_replay_storage& out, int32_t* idx, const char** why) {
  if (const char* w = replay_sample_argument_error(&s, n, cap, size, m, &out)) {
    if (why) *why = w;
    return -1;
  }
  const SampleNorm cfg{v.cfg.epsilon, v.cfg.clip_obs, v.cfg.clip_reward, v.cfg.norm_obs, v.cfg.norm_reward};
  const int64_t groups = ((int64_t)m * SAMPLE_PARTS + SAMPLE_THREADS - 1) / SAMPLE_THREADS;
  for (int64_t g = 0; g < groups; g++) {
    for (int thread = 0; thread < SAMPLE_THREADS; thread++) {
      const int64_t t = g * SAMPLE_THREADS + thread;
      const int64_t j = t / SAMPLE_PARTS;
      const int part = (int)(t % SAMPLE_PARTS);
      if (j >= m) continue;
      int32_t row, env;
      const int64_t cell = sample_cell_of(seed, draw, j, size, n, &row, &env);
      if (part == SAMPLE_PARTS - 1) {
        sample_tail(s, out, idx, cell, j, row, env, cfg, v.stats);
        continue;
      }
      const SamplePiece p = sample_piece(s, out, cell, j, part);
      float x[2] = {p.src[0], p.src[1]};
      normalize_piece(x, p.col, cfg, v.stats);
      p.dst[0] = x[0]; p.dst[1] = x[1];
    }
  }
  return 0;
}

}  // namespace vecnormreplayhost
