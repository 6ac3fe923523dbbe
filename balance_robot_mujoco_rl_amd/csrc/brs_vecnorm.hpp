// brs_vecnorm.hpp -- VecNormalize of include/brs_policy.h, the part shared by the HIP kernels (brs_vecnorm.hip)
// and the host build the CPU tests compare with the numpy restatement (tests/vecnormhost): the (count, mean, M2) triple and its
// merge, the thread <-> env map and the pairing of the reduction tree, the update of the running statistics, and the normalise
// and clip of one element, and the lane map of the normalising replay sample (tests/vecnormreplayhost).  All of
// it is fp64 `+ - * /` with contraction off, so host and device give the same bytes.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/brs.h"
#include "../../include/brs_policy.h"
#include "brs_offpolicy.hpp"  // sample_block, sample_cell: the cells of brs_replay_sample

#ifndef BRS_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BRS_HD __host__ __device__ __forceinline__
#else
#define BRS_HD inline
#endif
#endif

namespace brs {
namespace vecnorm {

constexpr int NOBS = 6, NCOL = 7, RET = 6;  // the six observation columns, then the discounted return
constexpr int WAVE = 64;
constexpr int MOMENT_THREADS = 256;         // moments kernel: workgroup g owns the envs [SLAB g, SLAB g + SLAB) ...
constexpr int ENVS_PER_THREAD = 4;          // ... thread t folds base + t + 256 j, j = 0..3, in ascending order
constexpr int SLAB = MOMENT_THREADS * ENVS_PER_THREAD;
constexpr int MOMENT_WAVES = MOMENT_THREADS / WAVE;
constexpr int NSTAT = 3 * NCOL;             // brs_vecnorm_stats as 21 doubles: obs mean, var, count [6] each, then the return's

BRS_HD int num_slabs(int n) { return (n + SLAB - 1) / SLAB; }
BRS_HD int mean_at(int c) { return c < NOBS ? c : 3 * NOBS; }
BRS_HD int var_at(int c) { return c < NOBS ? NOBS + c : 3 * NOBS + 1; }
BRS_HD int count_at(int c) { return c < NOBS ? 2 * NOBS + c : 3 * NOBS + 2; }

// the moments of a set of values: how many, their mean, and the sum of the squared distances from it
struct Triple {
  double n, mean, m2;
};

BRS_HD Triple empty() { return Triple{0.0, 0.0, 0.0}; }
BRS_HD Triple element(double x) { return Triple{1.0, x, 0.0}; }

// Chan's merge of two sets, a before b; an empty set leaves the other one as it is.  The branches look at the counts only, so
// a NaN or an Inf among the values goes through the arithmetic like any other number.
BRS_HD Triple merge(const Triple& a, const Triple& b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  const double d = b.mean - a.mean;
  const double n = a.n + b.n;
  Triple r;
  r.n = n;
  r.mean = a.mean + d * b.n / n;
  r.m2 = a.m2 + b.m2 + d * d * a.n * b.n / n;
  return r;
}

// SB3's RunningMeanStd.update_from_moments on one column of the 21 doubles, the batch given as its triple
BRS_HD void update_from_moments(double* stats, int c, const Triple& batch) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (batch.n == 0.0) return;
  const double bm = batch.mean, bv = batch.m2 / batch.n, bn = batch.n;
  const double mean = stats[mean_at(c)], var = stats[var_at(c)], count = stats[count_at(c)];
  const double delta = bm - mean;
  const double tot = count + bn;
  const double m2 = var * count + bv * bn + delta * delta * count * bn / tot;
  stats[mean_at(c)] = mean + delta * bn / tot;
  stats[var_at(c)] = m2 / tot;
  stats[count_at(c)] = tot;
}

// np.clip in fp64, brs_nan.hpp's clip_keep_nan for doubles: a NaN comes back as it is
BRS_HD double clip_keep_nan(double a, double lo, double hi) { return a != a ? a : fmin(hi, fmax(lo, a)); }

// one element, evaluated in fp64 and rounded once
BRS_HD float normalize_obs(float x, double mean, double var, double epsilon, double clip) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return (float)clip_keep_nan(((double)x - mean) / sqrt(var + epsilon), -clip, clip);
}

BRS_HD float normalize_reward(float r, double ret_var, double epsilon, double clip) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return (float)clip_keep_nan((double)r / sqrt(ret_var + epsilon), -clip, clip);
}

// returns[i] of a training step, before the statistics see it
BRS_HD double advance_return(double ret, double gamma, float reward) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return ret * gamma + (double)reward;
}

// What thread t of workgroup g of the moments kernel folds: the triples of its (up to) four envs, column by column.  With
// `with_ret` the discounted return of each env is advanced first and is the seventh column; without, that column stays empty
// (reset: observations only).
BRS_HD void fold_thread(int n, int g, int t, const float* obs, const float* reward, double* returns, double gamma, bool with_ret,
                        Triple* acc) {
  for (int c = 0; c < NCOL; c++) acc[c] = empty();
  for (int j = 0; j < ENVS_PER_THREAD; j++) {
    const int64_t i = (int64_t)g * SLAB + t + MOMENT_THREADS * j;
    if (i >= n) break;
    for (int c = 0; c < NOBS; c++) acc[c] = merge(acc[c], element((double)obs[i * NOBS + c]));
    if (with_ret) {
      const double r = advance_return(returns[i], gamma, reward[i]);
      returns[i] = r;
      acc[RET] = merge(acc[RET], element(r));
    }
  }
}

// The tree over the 64 lanes of a wave, step s of 1, 2, ... 32: lane l and lane l ^ s merge, the lower one first.  On the device
// every lane keeps the result (a butterfly; lane 0 then holds what a tree in which the lower partner keeps it gives); on the
// host, v[l] of the lanes l with l % 2s == 0.
inline void wave_tree_host(Triple* v) {
  for (int s = 1; s < WAVE; s <<= 1)
    for (int l = 0; l < WAVE; l += 2 * s) v[l] = merge(v[l], v[l + s]);
}

// lane l of a wave of the fold kernel: partials l, l + 64, ... of column c in ascending order
BRS_HD Triple fold_partials(const Triple* partials, int num, int c, int l) {
  Triple a = empty();
  for (int p = l; p < num; p += WAVE) a = merge(a, partials[(int64_t)p * NCOL + c]);
  return a;
}

// ---- brs_replay_sample_vecnorm: ReplayBuffer.sample(batch_size, env=vec_normalize).  The geometry is
// brs_replay_sample's: eight lanes per sample, lane `part` of sample j.  Parts 0-2 carry columns 2p, 2p + 1 of obs, parts 3-5 the
// same columns of next_obs, part 6 the action, part 7 reward, done and idx.
constexpr int SAMPLE_PARTS = 8, SAMPLE_THREADS = 256, SAMPLES_PER_GROUP = SAMPLE_THREADS / SAMPLE_PARTS;

// what the normalisation of a sample reads of the handle's configuration
struct SampleNorm {
  double epsilon, clip_obs, clip_reward;
  int norm_obs, norm_reward;
};

// the cell sample j of `draw` reads: brs_replay_sample's Philox block and row/env map
BRS_HD int64_t sample_cell_of(uint64_t seed, uint32_t draw, int64_t j, int32_t size, int32_t n, int32_t* row, int32_t* env) {
  uint32_t w[4];
  brs::offpolicy::sample_block(seed, draw, (uint32_t)j, w);
  brs::offpolicy::sample_cell(w[0], w[1], size, n, row, env);
  return (int64_t)*row * n + *env;
}

// parts 0-6: where the lane's two floats come from and go to; `col`: their first observation column, -1 for the action
struct SamplePiece {
  const float* src;
  float* dst;
  int col;
};
BRS_HD SamplePiece sample_piece(const brs_replay_storage& s, const brs_replay_storage& out, int64_t cell, int64_t j, int part) {
  constexpr int OBS = brs::offpolicy::OBS, ACT = brs::offpolicy::ACT;
  if (part < 3) return SamplePiece{s.obs + cell * OBS + 2 * part, out.obs + j * OBS + 2 * part, 2 * part};
  if (part < 6) return SamplePiece{s.next_obs + cell * OBS + 2 * (part - 3), out.next_obs + j * OBS + 2 * (part - 3), 2 * (part - 3)};
  return SamplePiece{s.action + cell * ACT, out.action + j * ACT, -1};
}

// the two floats of a piece through normalize_obs of their columns; the action and a switched-off half stay as they are
BRS_HD void normalize_piece(float* v, int col, const SampleNorm& c, const double* stats) {
  if (col < 0 || !c.norm_obs) return;
  for (int k = 0; k < 2; k++) v[k] = normalize_obs(v[k], stats[mean_at(col + k)], stats[var_at(col + k)], c.epsilon, c.clip_obs);
}

// part 7
BRS_HD void sample_tail(const brs_replay_storage& s, const brs_replay_storage& out, int32_t* idx, int64_t cell, int64_t j, int32_t row,
                        int32_t env, const SampleNorm& c, const double* stats) {
  const float r = s.reward[cell];
  out.reward[j] = c.norm_reward ? normalize_reward(r, stats[var_at(RET)], c.epsilon, c.clip_reward) : r;
  out.done[j] = s.done[cell];
  if (idx) { idx[2 * j] = row; idx[2 * j + 1] = env; }
}

// the argument rules of brs_replay_sample_vecnorm that need no device, brs_replay_sample's: 0 or the text after the call's name
inline const char* replay_sample_argument_error(const brs_replay_storage* s, int32_t n, int32_t cap, int32_t size, int32_t m,
                                                const brs_replay_storage* out) {
  if (!s || !s->obs || !s->next_obs || !s->action || !s->reward || !s->done) return "null storage pointer";
  if (n < 1 || cap < 1) return "n and cap must be at least 1";
  if (n > 0x7fffffff / brs::offpolicy::OBS) return "n * 6 exceeds 2^31 - 1";
  if ((int64_t)cap * (int64_t)n > 0x7fffffffLL) return "cap * n exceeds 2^31 - 1";
  if (size < 1 || size > cap) return "size must be in [1, cap]";
  if (m < 1 || m > (1 << 27)) return "m must be in [1, 2^27]";
  if (!out || !out->obs || !out->next_obs || !out->action || !out->reward || !out->done) return "null output pointer";
  return nullptr;
}

}  // namespace vecnorm
}  // namespace brs
