// brs_learner.hip -- the PPO learner of include/brs_policy.h as HIP kernels for gfx950: the minibatch body of
// tools/train_ppo_torch.py::train (SB3 PPO.train()), gradient and optimiser step, without torch.
//
//   learner_adv_kernel     one workgroup of 1,024: mean and unbiased std of the minibatch's advantages, fp64, fixed order.
//   learner_grad_kernel    a persistent grid of G <= max_workgroups workgroups of 256; workgroup g takes the 256-sample chunks
//                          g, g + G, ... and writes ONE partial row (gradient sums, stat sums) to the handle's scratch.
//                          A wave owns 64 samples.  Forward is brs_policy_tile.hpp's tower_forward, the one the rollout kernels
//                          run (fp32 v_mfma_f32_32x32x2_f32, transposed product D[unit][sample], padded LDS image of the tower,
//                          activations stay in accumulator layout), with a hook that keeps h1 and h2.  Backward: dz2 = (W3^T dz3) (1 - h2^2) on the vector ALU, dz1 = (W2^T dz2) (1 - h1^2)
//                          on the matrix cores again -- the SAME LDS image read with the indices swapped gives W2^T as the A operand.
//                          The weight gradients contract over SAMPLES, and the accumulator layout holds "units of my sample", so
//                          both operands of dW2 = sum_s dz2 (x) h1 have to be transposed: the four waves take turns to write
//                          their [unit][sample] images of (dz2, h1) and then (dz1, h2) to one shared LDS pair, and after each
//                          write ALL four waves contract it -- wave w owns the 32x32 tile (w / 2, w % 2) of dW2 (32 MFMAs per
//                          turn, 16 accumulator registers that live across the chunks), and the small products (dW1, dW3, the
//                          three bias sums) are rows of 64 LDS reads on the vector ALU, one output per thread.
//   learner_reduce_kernel  column c of the G partial rows, summed in ascending g in fp64 -> grad_dev[c].
//   learner_apply_kernel   one workgroup of 1,024: the two squared norms (fold + tree of fixed pairing, fp64), the clip scale,
//                          the KL early stop and the Adam step.  The norms are taken here, after a data-parallel caller's
//                          all-reduce of grad_dev, because that is the gradient torch's clip_grad_norm_ would see.
//   learner_a2c_grad_kernel, learner_rmsprop_apply_kernel   SB3's A2C.train() on the same handle: the gradient kernel
//                          with -adv log pi in the actor's head and rows 0..m-1 where idx is null; the clip scale, then RMSpropTFLike.
//                          The value loss keeps critic_head's 0.5 d^2: SB3's vf_coef = 0.5 on mse_loss is vf_coef = 1.0 here.
// The two gradient kernels are one body, grad_body, over a family (PpoFamily, A2cFamily); the two apply kernels open with the same
// grad_norms; brs_learner_grad and brs_a2c_grad enqueue through the same launch_grad.
// Padding: a lane past m (or with an index outside the buffer) feeds zero observations and its dz3 is zero, it is left out of
// the stats, the advantage statistics and the 1 / m.  No floating-point atomic, no communication between workgroups.
#include <hip/hip_runtime.h>

#include <string>

#include "brs_host.hpp"
#include "brs_learner.hpp"
#include "brs_policy_tile.hpp"  // the LDS image of a tower, stage_tower, tower_forward, BRS_UNIT

namespace {

using namespace brs::policy_tile;  // brs::learner's names with it

constexpr int GRAD_THREADS = CHUNK;  // 4 waves x 64 samples
// transposed images of one wave's 64 samples: P and Q [64 units][TLD], R [8][TLD]: rows 0..5 the observations, 6.. dz3
constexpr int TLD = 65, PQ_SIZE = HID * TLD, R_ROWS = 8, R_DZ3 = 6, R_SIZE = R_ROWS * TLD;
constexpr int NACC = ACT + NSTAT + 1;  // per-thread sums carried over the chunks: dlog_std, the stats, bad indices
static_assert((T_SIZE + 2 * PQ_SIZE + R_SIZE) * sizeof(float) <= 64 * 1024, "static LDS");
static_assert(GRAD_THREADS * NACC <= PQ_SIZE, "the final tree reuses P");

// tower_forward's hook: the activations of both layers, [mt][nt][r]: unit BRS_UNIT(mt, r) of sample 32 nt + lane % 32
struct KeepActivations {
  f32x16 (&a1)[2][2];
  f32x16 (&a2)[2][2];
  __device__ __forceinline__ void h1(int mt, int nt, int r, float v) const { a1[mt][nt][r] = v; }
  __device__ __forceinline__ void h2(int mt, int nt, int r, float v) const { a2[mt][nt][r] = v; }
};

// dz3[nt][k] (complete in both halves) -> dz2 and dz1 in accumulator layout
template <int NOUT>
__device__ __forceinline__ void tower_backward(const float* __restrict__ L, const float (&dz3)[2][NOUT], const f32x16 (&h1)[2][2],
                                               const f32x16 (&h2)[2][2], f32x16 (&dz2)[2][2], f32x16 (&dz1)[2][2]) {
  const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
#pragma unroll
  for (int mt = 0; mt < 2; mt++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      float g0 = 0.0f, g1 = 0.0f;
#pragma unroll
      for (int k = 0; k < NOUT; k++) {
        const float w3 = L[T_W3 + k * HID + BRS_UNIT(mt, r)];
        g0 = fmaf(w3, dz3[0][k], g0); g1 = fmaf(w3, dz3[1][k], g1);
      }
      dz2[mt][0][r] = g0 * (1.0f - h2[mt][0][r] * h2[mt][0][r]);
      dz2[mt][1][r] = g1 * (1.0f - h2[mt][1][r] * h2[mt][1][r]);
    }
  // D[k][sample] = sum_j W2[j][k] dz2[j][sample]: A is W2^T -- row 32 mt + c of it is COLUMN 32 mt + c of the image -- and the
  // contraction index j is walked in accumulator order, as in the forward
  f32x16 acc[2][2];
#pragma unroll
  for (int mt = 0; mt < 2; mt++)
#pragma unroll
    for (int nt = 0; nt < 2; nt++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[mt][nt][r] = 0.0f;
#pragma unroll
  for (int mtp = 0; mtp < 2; mtp++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int j = BRS_UNIT(mtp, r);
      const float a0 = L[T_W2 + j * W2_LD + c], a1 = L[T_W2 + j * W2_LD + 32 + c];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, dz2[mtp][0][r], acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, dz2[mtp][1][r], acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, dz2[mtp][0][r], acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, dz2[mtp][1][r], acc[1][1], 0, 0, 0);
    }
#pragma unroll
  for (int mt = 0; mt < 2; mt++)
#pragma unroll
    for (int nt = 0; nt < 2; nt++)
#pragma unroll
      for (int r = 0; r < 16; r++) dz1[mt][nt][r] = acc[mt][nt][r] * (1.0f - h1[mt][nt][r] * h1[mt][nt][r]);
}

// this wave's image of a [unit][sample] matrix held in accumulator layout
__device__ __forceinline__ void write_transposed(float* __restrict__ T, const f32x16 (&a)[2][2]) {
  const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
#pragma unroll
  for (int mt = 0; mt < 2; mt++)
#pragma unroll
    for (int nt = 0; nt < 2; nt++)
#pragma unroll
      for (int r = 0; r < 16; r++) T[BRS_UNIT(mt, r) * TLD + 32 * nt + c] = a[mt][nt][r];
}

__device__ __forceinline__ float row_sum(const float* __restrict__ row) {
  float s = 0.0f;
  for (int i = 0; i < 64; i++) s += row[i];
  return s;
}
__device__ __forceinline__ float row_dot(const float* __restrict__ a, const float* __restrict__ b) {
  float s = 0.0f;
  for (int i = 0; i < 64; i++) s = fmaf(a[i], b[i], s);
  return s;
}

// gradient sums of one tower that live in registers across the chunks
struct TowerSums {
  f32x16 w2;      // tile (wave / 2, wave % 2) of dW2[j][k]: rows j = 32 (wave / 2) + accumulator row, column k = 32 (wave % 2) + c
  float w1a, w1b; // dW1 entries tid and tid + 256 (< 384)
  float bias;     // tid < 64: db2[tid]; 64 <= tid < 128: db1[tid - 64]; 128 <= tid < 128 + NOUT: db3[tid - 128]
  float w3;       // tid < 64 NOUT: dW3 entry tid
};

__device__ __forceinline__ void zero(TowerSums& a) {
#pragma unroll
  for (int r = 0; r < 16; r++) a.w2[r] = 0.0f;
  a.w1a = a.w1b = a.bias = a.w3 = 0.0f;
}

// One tower of one chunk: forward, the head's dz3 (through `head`, which sees the lane's OWN sample: lane l finishes sample l of
// the wave, N-tile l / 32, column l % 32), backward, and the sample contraction into `sums`.  Called by every thread of the
// workgroup (barriers inside).
template <int NOUT, class Head>
__device__ __forceinline__ void tower_chunk(const float* __restrict__ w, float* __restrict__ Lw, float* __restrict__ P, float* __restrict__ Q,
                                            float* __restrict__ R, const float (&x)[2][OBS], TowerSums& sums, Head&& head) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  __syncthreads();  // the previous tower's image and transposed buffers are no longer read
  stage_tower<NOUT>(w, Lw, GRAD_THREADS);
  __syncthreads();
  f32x16 h1[2][2], h2[2][2], dz2[2][2], dz1[2][2];
  float out[2][NOUT], own[NOUT], d3own[NOUT], dz3[2][NOUT];
  tower_forward<NOUT>(Lw, x, out, KeepActivations{h1, h2});
#pragma unroll
  for (int k = 0; k < NOUT; k++) own[k] = h ? out[1][k] : out[0][k];
  head(own, d3own);
#pragma unroll
  for (int nt = 0; nt < 2; nt++)
#pragma unroll
    for (int k = 0; k < NOUT; k++) dz3[nt][k] = __shfl(d3own[k], 32 * nt + c, 64);
  tower_backward<NOUT>(Lw, dz3, h1, h2, dz2, dz1);
  const int mt = wave >> 1, nt = wave & 1;
#pragma unroll 1
  for (int turn = 0; turn < 4; turn++) {
    __syncthreads();
    if (wave == turn) {
      write_transposed(P, dz2);
      write_transposed(Q, h1);
#pragma unroll
      for (int k = 0; k < OBS; k++) R[k * TLD + lane] = h ? x[1][k] : x[0][k];
#pragma unroll
      for (int k = 0; k < NOUT; k++) R[(R_DZ3 + k) * TLD + lane] = d3own[k];
    }
    __syncthreads();
    // dW2 += dz2^T h1 over the 64 samples of wave `turn`: A[row j][s] = P[j][s], B[s][col k] = Q[k][s]
#pragma unroll 8
    for (int s = 0; s < 32; s++)
      sums.w2 = __builtin_amdgcn_mfma_f32_32x32x2f32(P[(32 * mt + c) * TLD + 2 * s + h], Q[(32 * nt + c) * TLD + 2 * s + h], sums.w2, 0, 0, 0);
    if (tid < HID) sums.bias += row_sum(P + tid * TLD);
    else if (tid >= 2 * HID && tid < 2 * HID + NOUT) sums.bias += row_sum(R + (R_DZ3 + tid - 2 * HID) * TLD);
    __syncthreads();
    if (wave == turn) {
      write_transposed(P, dz1);
      write_transposed(Q, h2);
    }
    __syncthreads();
    sums.w1a += row_dot(P + (tid / OBS) * TLD, R + (tid % OBS) * TLD);
    if (tid + GRAD_THREADS < HID * OBS) sums.w1b += row_dot(P + ((tid + GRAD_THREADS) / OBS) * TLD, R + ((tid + GRAD_THREADS) % OBS) * TLD);
    if (tid >= HID && tid < 2 * HID) sums.bias += row_sum(P + (tid - HID) * TLD);
    if (tid < NOUT * HID) sums.w3 += row_dot(R + (R_DZ3 + (tid >> 6)) * TLD, Q + (tid & 63) * TLD);
  }
}

template <int NOUT> __device__ __forceinline__ void store_tower(float* __restrict__ row, const TowerSums& a) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  const int mt = wave >> 1, nt = wave & 1;
#pragma unroll
  for (int r = 0; r < 16; r++) row[O_W2 + BRS_UNIT(mt, r) * HID + 32 * nt + c] = a.w2[r];
  row[O_W1 + tid] = a.w1a;
  if (tid + GRAD_THREADS < HID * OBS) row[O_W1 + tid + GRAD_THREADS] = a.w1b;
  if (tid < HID) row[O_B2 + tid] = a.bias;
  else if (tid < 2 * HID) row[O_B1 + tid - HID] = a.bias;
  else if (tid < 2 * HID + NOUT) row[O_W3 + NOUT * HID + tid - 2 * HID] = a.bias;
  if (tid < NOUT * HID) row[O_W3 + tid] = a.w3;
}

__global__ void __launch_bounds__(ADV_THREADS) learner_adv_kernel(const float* __restrict__ adv, const int32_t* __restrict__ idx, const int m,
                                                                  const int n_rows, float* __restrict__ out) {
  __shared__ double S[ADV_THREADS], SS[ADV_THREADS];
  const int t = threadIdx.x;
  double s, ss;
  fold_adv(adv, idx, m, n_rows, t, s, ss);  // idx null (A2C): the buffer's first m rows
  S[t] = s; SS[t] = ss;
  __syncthreads();
  for (int k = ADV_THREADS / 2; k >= 1; k >>= 1) {
    if (t < k) { S[t] += S[t + k]; SS[t] += SS[t + k]; }
    __syncthreads();
  }
  if (t == 0) adv_mean_denom(S[0], SS[0], m, out);
}

// The two families of the gradient kernel: PPO and A2C (7.9: -adv log pi in the actor's head, no logp_old, and the
// whole buffer in its own order where idx is null).  A family names its config, looks up the row of entry i, calls its actor head
// and says whether that head feeds the KL and clip-fraction sums.  grad_body takes it by value: it is a pointer at most.
struct PpoFamily {
  using Config = brs_ppo_config;
  static constexpr bool RATIO_STATS = true;
  const float* __restrict__ logp_old;
  __device__ __forceinline__ int32_t row(const int32_t* __restrict__ idx, int i) const { return idx[i]; }  // brs_learner_grad refuses a null idx
  __device__ __forceinline__ ActorHead head(const float (&mean)[ACT], const float (&log_std)[ACT], const float (&a)[ACT], int32_t row,
                                            float adv_n, const Config& c, float inv_m) const {
    return actor_head(mean, log_std, a, logp_old[row], adv_n, c, inv_m);
  }
};
struct A2cFamily {
  using Config = brs_a2c_config;
  static constexpr bool RATIO_STATS = false;  // the KL and clip-fraction sums stay zero
  __device__ __forceinline__ int32_t row(const int32_t* __restrict__ idx, int i) const { return row_at(idx, i); }
  __device__ __forceinline__ ActorHead head(const float (&mean)[ACT], const float (&log_std)[ACT], const float (&a)[ACT], int32_t,
                                            float adv_n, const Config& c, float inv_m) const {
    return a2c_actor_head(mean, log_std, a, adv_n, c, inv_m);
  }
};

// The gradient kernel of either family: grid, chunks, LDS images, partial row and the final tree are the same.
template <class Family>
__device__ __forceinline__ void grad_body(const Family family, const float* __restrict__ w, const int n_rows, const float* __restrict__ obs,
                                          const float* __restrict__ act, const float* __restrict__ adv, const float* __restrict__ ret,
                                          const int32_t* __restrict__ idx, const int m, const typename Family::Config& cfg,
                                          const float* __restrict__ adv_stat, float* __restrict__ partial) {
  __shared__ float Lw[T_SIZE], P[PQ_SIZE], Q[PQ_SIZE], R[R_SIZE];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31;
  const int nchunks = (m + CHUNK - 1) / CHUNK;
  const float inv_m = 1.0f / (float)m;
  const float adv_mean = cfg.normalize_adv ? adv_stat[0] : 0.0f, adv_denom = cfg.normalize_adv ? adv_stat[1] : 1.0f;
  const float log_std[ACT] = {w[OFF_LOGSTD], w[OFF_LOGSTD + 1]};
  const auto& critic_cfg = shared_fields(cfg);
  TowerSums pi, vf;
  zero(pi); zero(vf);
  float acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; k++) acc[k] = 0.0f;
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {  // uniform over the workgroup
    const int base = chunk * CHUNK + wave * 64;
    float x[2][OBS];
#pragma unroll
    for (int nt = 0; nt < 2; nt++) {
      const int e = base + 32 * nt + c;
      const int32_t row = e < m ? family.row(idx, e) : -1;
      const bool ok = row >= 0 && row < n_rows;
#pragma unroll
      for (int k = 0; k < OBS; k++) x[nt][k] = ok ? obs[(size_t)OBS * row + k] : 0.0f;
    }
    const int i = base + lane;
    const int32_t row = i < m ? family.row(idx, i) : -1;
    const bool valid = row >= 0 && row < n_rows;
    if (i < m && !valid) acc[ACT + NSTAT] += 1.0f;
    tower_chunk<ACT>(w + OFF_PI, Lw, P, Q, R, x, pi, [&](const float (&mean)[ACT], float (&d3)[ACT]) {
      ActorHead hd = zero_actor_head();
      if (valid) {
        const float a[ACT] = {act[(size_t)ACT * row], act[(size_t)ACT * row + 1]};
        hd = family.head(mean, log_std, a, row, (adv[row] - adv_mean) / adv_denom, cfg, inv_m);
      }
      d3[0] = hd.dmean[0]; d3[1] = hd.dmean[1];
      acc[0] += hd.dlog_std[0]; acc[1] += hd.dlog_std[1];
      acc[ACT + S_PL] += hd.pl; acc[ACT + S_ENT] += hd.ent;
      if constexpr (Family::RATIO_STATS) { acc[ACT + S_KL] += hd.kl; acc[ACT + S_CLIPFRAC] += hd.clipfrac; }
    });
    tower_chunk<1>(w + OFF_VF, Lw, P, Q, R, x, vf, [&](const float (&v)[1], float (&d3)[1]) {
      CriticHead hd = {0.0f, 0.0f};
      if (valid) hd = critic_head(v[0], ret[row], critic_cfg, inv_m);
      d3[0] = hd.dvalue;
      acc[ACT + S_VL] += hd.vl;
    });
  }
  float* row_out = partial + (size_t)blockIdx.x * ROW;
  store_tower<ACT>(row_out + OFF_PI, pi);
  store_tower<1>(row_out + OFF_VF, vf);
  // the per-thread sums: a tree of fixed pairing over the 256 threads
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NACC; k++) P[k * GRAD_THREADS + tid] = acc[k];
  __syncthreads();
  for (int s = GRAD_THREADS / 2; s >= 1; s >>= 1) {
    if (tid < s)
#pragma unroll
      for (int k = 0; k < NACC; k++) P[k * GRAD_THREADS + tid] += P[k * GRAD_THREADS + tid + s];
    __syncthreads();
  }
  if (tid < NACC) row_out[OFF_LOGSTD + tid] = P[tid * GRAD_THREADS];  // log_std[2], then the stats and the bad-index count: ROW's order
}

__global__ void __launch_bounds__(GRAD_THREADS) learner_grad_kernel(const float* __restrict__ w, const int n_rows, const float* __restrict__ obs,
                                                                    const float* __restrict__ act, const float* __restrict__ logp_old,
                                                                    const float* __restrict__ adv, const float* __restrict__ ret,
                                                                    const int32_t* __restrict__ idx, const int m, const brs_ppo_config cfg,
                                                                    const float* __restrict__ adv_stat, float* __restrict__ partial) {
  grad_body(PpoFamily{logp_old}, w, n_rows, obs, act, adv, ret, idx, m, cfg, adv_stat, partial);
}

__global__ void __launch_bounds__(GRAD_THREADS) learner_a2c_grad_kernel(const float* __restrict__ w, const int n_rows, const float* __restrict__ obs,
                                                                        const float* __restrict__ act, const float* __restrict__ adv,
                                                                        const float* __restrict__ ret, const int32_t* __restrict__ idx, const int m,
                                                                        const brs_a2c_config cfg, const float* __restrict__ adv_stat,
                                                                        float* __restrict__ partial) {
  grad_body(A2cFamily{}, w, n_rows, obs, act, adv, ret, idx, m, cfg, adv_stat, partial);
}

__global__ void __launch_bounds__(256) learner_reduce_kernel(const float* __restrict__ partial, const int G, float* __restrict__ grad,
                                                             brs_learner_info* __restrict__ info) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= ROW) return;
  const float s = combine_rows(partial, G, col);
  if (col < NPARAM + NSTAT) grad[col] = s;
  else info->bad_index = (int32_t)s;
}

// The opening of both apply kernels: the two squared norms of grad (fold + tree of fixed pairing, fp64) -> the norms under the
// config's clip mode, in every thread.  Called by all APPLY_THREADS threads of the one workgroup (barriers inside).
__device__ __forceinline__ void grad_norms(const float* __restrict__ grad, const brs_ppo_config& clip_cfg, float& norm_pi, float& norm_vf) {
  __shared__ double SP[APPLY_THREADS], SV[APPLY_THREADS];
  const int t = threadIdx.x;
  double sp, sv;
  fold_squares(grad, t, sp, sv);
  SP[t] = sp; SV[t] = sv;
  __syncthreads();
  for (int k = APPLY_THREADS / 2; k >= 1; k >>= 1) {
    if (t < k) { SP[t] += SP[t + k]; SV[t] += SV[t + k]; }
    __syncthreads();
  }
  norms(SP[0], SV[0], clip_cfg, norm_pi, norm_vf);
}

__global__ void __launch_bounds__(APPLY_THREADS) learner_apply_kernel(float* __restrict__ params, const float* __restrict__ grad,
                                                                      float* __restrict__ m, float* __restrict__ v, const brs_ppo_config cfg,
                                                                      brs_learner_info* __restrict__ info) {
  const int t = threadIdx.x;
  const int32_t was_stopped = info->stopped;  // read by everybody before thread 0 writes (grad_norms' barriers lie in between)
  const int64_t steps = info->steps;
  float norm_pi, norm_vf;
  grad_norms(grad, cfg, norm_pi, norm_vf);
  const bool stop = was_stopped || kl_stops(grad[NPARAM + S_KL], cfg);
  if (t == 0) {
    info->stopped = stop ? 1 : 0;
    if (!stop) info->steps = steps + 1;
    for (int k = 0; k < NSTAT; k++) info->stat[k] = grad[NPARAM + k];
    info->grad_norm_pi = norm_pi; info->grad_norm_vf = norm_vf;
  }
  if (stop) return;
  const AdamScalars a = adam_scalars(cfg, steps + 1);
  for (int i = t; i < NPARAM; i += APPLY_THREADS) {
    float p = params[i], mi = m[i], vi = v[i];
    adam_update(p, mi, vi, grad[i] * param_scale(i, norm_pi, norm_vf, cfg), a);
    params[i] = p; m[i] = mi; v[i] = vi;
  }
}

// A2C's optimiser step: learner_apply_kernel's norms and clip scale, then RMSpropTFLike.  No early stop: `stopped` is not touched.
__global__ void __launch_bounds__(APPLY_THREADS) learner_rmsprop_apply_kernel(float* __restrict__ params, const float* __restrict__ grad,
                                                                              float* __restrict__ sq, const brs_a2c_config cfg,
                                                                              brs_learner_info* __restrict__ info) {
  const int t = threadIdx.x;
  const brs_ppo_config clip_cfg = shared_fields(cfg);
  float norm_pi, norm_vf;
  grad_norms(grad, clip_cfg, norm_pi, norm_vf);
  if (t == 0) {
    info->steps = info->steps + 1;
    for (int k = 0; k < NSTAT; k++) info->stat[k] = grad[NPARAM + k];
    info->grad_norm_pi = norm_pi; info->grad_norm_vf = norm_vf;
  }
  const RmspropScalars r = rmsprop_scalars(cfg);
  for (int i = t; i < NPARAM; i += APPLY_THREADS) {
    float p = params[i], s = sq[i];
    rmsprop_tf_update(p, s, grad[i] * param_scale(i, norm_pi, norm_vf, clip_cfg), r);
    params[i] = p; sq[i] = s;
  }
}

}  // namespace

struct brs_learner {
  int device = 0, max_workgroups = 0;
  char* block = nullptr;  // the partial rows, the advantage statistics and the info slot: one allocation
  float* partial = nullptr;
  float* adv_stat = nullptr;
  brs_learner_info* info = nullptr;
  std::string err;
};

using brs::host::DeviceGuard, brs::host::fail;

// What brs_learner_grad and brs_a2c_grad enqueue on `s` once their arguments are checked and the device is set: the advantage
// statistics where asked for, the family's gradient kernel on G workgroups (`launch_grad_kernel(G, s)`), the reduce kernel.
template <class Launch>
static int launch_grad(brs_learner* l, int32_t normalize_adv, int32_t n_rows, const float* adv_dev, const int32_t* idx_dev, int32_t m,
                       float* grad_dev, hipStream_t s, Launch&& launch_grad_kernel) {
  const int nchunks = (m + CHUNK - 1) / CHUNK, G = nchunks < l->max_workgroups ? nchunks : l->max_workgroups;
  if (normalize_adv) hipLaunchKernelGGL(learner_adv_kernel, dim3(1), dim3(ADV_THREADS), 0, s, adv_dev, idx_dev, m, n_rows, l->adv_stat);
  launch_grad_kernel(G, s);
  hipLaunchKernelGGL(learner_reduce_kernel, dim3((ROW + 255) / 256), dim3(256), 0, s, l->partial, G, grad_dev, l->info);
  BRS_HIP_TRY(l, hipGetLastError());
  return BRS_OK;
}

extern "C" {

int brs_learner_create(int32_t device, int32_t max_workgroups, brs_learner** out) {
  if (!out) return fail<brs_learner>(nullptr, BRS_ERR_ARG, "brs_learner_create: null argument");
  *out = nullptr;
  std::string why;
  if (const int rc = brs::host::check_device(device, "brs_learner_create", &why)) return fail<brs_learner>(nullptr, rc, why);
  DeviceGuard g(device);
  hipDeviceProp_t prop;
  if (!g.ok || hipGetDeviceProperties(&prop, device) != hipSuccess)
    return fail<brs_learner>(nullptr, BRS_ERR_HIP, "brs_learner_create: hipGetDeviceProperties failed");
  brs_learner* l = new brs_learner();
  l->device = device;
  l->max_workgroups = max_workgroups > 0 ? max_workgroups : (prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1);
  const size_t partial_bytes = ((size_t)l->max_workgroups * ROW * sizeof(float) + 255) & ~(size_t)255;
  const size_t bytes = partial_bytes + 256 + 256;
  if (hipMalloc((void**)&l->block, bytes) != hipSuccess || hipMemset(l->block, 0, bytes) != hipSuccess) {
    if (l->block) (void)hipFree(l->block);
    delete l;
    return fail<brs_learner>(nullptr, BRS_ERR_HIP, "brs_learner_create: device allocation failed");
  }
  l->partial = (float*)l->block;
  l->adv_stat = (float*)(l->block + partial_bytes);
  l->info = (brs_learner_info*)(l->block + partial_bytes + 256);
  *out = l;
  return BRS_OK;
}

int brs_learner_destroy(brs_learner* l) {
  if (!l) return BRS_ERR_STATE;
  {
    DeviceGuard g(l->device);
    if (l->block) (void)hipFree(l->block);
  }
  delete l;
  return BRS_OK;
}

const char* brs_learner_last_error(const brs_learner* l) { return brs::host::last_error(l); }

int brs_learner_begin_iteration(brs_learner* l, void* stream) {
  if (!l) return fail<brs_learner>(nullptr, BRS_ERR_ARG, "brs_learner_begin_iteration: null handle");
  DeviceGuard g(l->device);
  if (!g.ok) return fail(l, BRS_ERR_HIP, "brs_learner_begin_iteration: hipSetDevice failed");
  BRS_HIP_TRY(l, hipMemsetAsync(&l->info->stopped, 0, sizeof(int32_t), (hipStream_t)stream));
  return BRS_OK;
}

int brs_learner_grad(brs_learner* l, const float* params_dev, int32_t n_rows, const float* obs_dev, const float* act_dev,
                     const float* logp_old_dev, const float* adv_dev, const float* ret_dev, const int32_t* idx_dev, int32_t m,
                     const brs_ppo_config* cfg, float* grad_dev, void* stream) {
  // what needs no handle is checked first (fail() records it in the family's slot when there is none)
  if (!cfg) return fail(l, BRS_ERR_ARG, "brs_learner_grad: null config");
  if (m > 0 && !idx_dev) return fail(l, BRS_ERR_ARG, "brs_learner_grad: null idx");
  if (m < 2) return fail(l, BRS_ERR_ARG, "brs_learner_grad: a minibatch needs at least two samples (unbiased std)");
  if (!l) return fail<brs_learner>(nullptr, BRS_ERR_ARG, "brs_learner_grad: null handle");
  if (n_rows <= 0 || !params_dev || !obs_dev || !act_dev || !logp_old_dev || !adv_dev || !ret_dev || !grad_dev)
    return fail(l, BRS_ERR_ARG, "brs_learner_grad: bad argument");
  if (!(cfg->ret_scale > 0.0f)) return fail(l, BRS_ERR_ARG, "brs_learner_grad: ret_scale must be positive");
  DeviceGuard g(l->device);
  if (!g.ok) return fail(l, BRS_ERR_HIP, "brs_learner_grad: hipSetDevice failed");
  return launch_grad(l, cfg->normalize_adv, n_rows, adv_dev, idx_dev, m, grad_dev, (hipStream_t)stream, [&](int G, hipStream_t s) {
    hipLaunchKernelGGL(learner_grad_kernel, dim3(G), dim3(GRAD_THREADS), 0, s, params_dev, n_rows, obs_dev, act_dev, logp_old_dev, adv_dev,
                       ret_dev, idx_dev, m, *cfg, l->adv_stat, l->partial);
  });
}

int brs_learner_apply(brs_learner* l, float* params_dev, const float* grad_dev, float* m_dev, float* v_dev, const brs_ppo_config* cfg,
                      void* stream) {
  if (!cfg) return fail(l, BRS_ERR_ARG, "brs_learner_apply: null config");
  if (!l) return fail<brs_learner>(nullptr, BRS_ERR_ARG, "brs_learner_apply: null handle");
  if (!params_dev || !grad_dev || !m_dev || !v_dev) return fail(l, BRS_ERR_ARG, "brs_learner_apply: null argument");
  DeviceGuard g(l->device);
  if (!g.ok) return fail(l, BRS_ERR_HIP, "brs_learner_apply: hipSetDevice failed");
  hipLaunchKernelGGL(learner_apply_kernel, dim3(1), dim3(APPLY_THREADS), 0, (hipStream_t)stream, params_dev, grad_dev, m_dev, v_dev, *cfg, l->info);
  BRS_HIP_TRY(l, hipGetLastError());
  return BRS_OK;
}

int brs_a2c_grad(brs_learner* l, const float* params_dev, int32_t n_rows, const float* obs_dev, const float* act_dev, const float* adv_dev,
                 const float* ret_dev, const int32_t* idx_dev, int32_t m, const brs_a2c_config* cfg, float* grad_dev, void* stream) {
  if (!cfg) return fail(l, BRS_ERR_ARG, "brs_a2c_grad: null config");
  if (m < 1) return fail(l, BRS_ERR_ARG, "brs_a2c_grad: an update needs at least one sample");
  if (cfg->normalize_adv && m < 2) return fail(l, BRS_ERR_ARG, "brs_a2c_grad: normalize_adv needs at least two samples (unbiased std)");
  if (!idx_dev && m > n_rows) return fail(l, BRS_ERR_ARG, "brs_a2c_grad: null idx takes rows 0..m-1, m must not exceed n_rows");
  if (!(cfg->ret_scale > 0.0f)) return fail(l, BRS_ERR_ARG, "brs_a2c_grad: ret_scale must be positive");
  if (!l) return fail<brs_learner>(nullptr, BRS_ERR_ARG, "brs_a2c_grad: null handle");
  if (n_rows <= 0 || !params_dev || !obs_dev || !act_dev || !adv_dev || !ret_dev || !grad_dev)
    return fail(l, BRS_ERR_ARG, "brs_a2c_grad: bad argument");
  DeviceGuard g(l->device);
  if (!g.ok) return fail(l, BRS_ERR_HIP, "brs_a2c_grad: hipSetDevice failed");
  return launch_grad(l, cfg->normalize_adv, n_rows, adv_dev, idx_dev, m, grad_dev, (hipStream_t)stream, [&](int G, hipStream_t s) {
    hipLaunchKernelGGL(learner_a2c_grad_kernel, dim3(G), dim3(GRAD_THREADS), 0, s, params_dev, n_rows, obs_dev, act_dev, adv_dev, ret_dev, idx_dev,
                       m, *cfg, l->adv_stat, l->partial);
  });
}

int brs_a2c_apply(brs_learner* l, float* params_dev, const float* grad_dev, float* sq_dev, const brs_a2c_config* cfg, void* stream) {
  if (!cfg) return fail(l, BRS_ERR_ARG, "brs_a2c_apply: null config");
  if (!l) return fail<brs_learner>(nullptr, BRS_ERR_ARG, "brs_a2c_apply: null handle");
  if (!params_dev || !grad_dev || !sq_dev) return fail(l, BRS_ERR_ARG, "brs_a2c_apply: null argument");
  DeviceGuard g(l->device);
  if (!g.ok) return fail(l, BRS_ERR_HIP, "brs_a2c_apply: hipSetDevice failed");
  hipLaunchKernelGGL(learner_rmsprop_apply_kernel, dim3(1), dim3(APPLY_THREADS), 0, (hipStream_t)stream, params_dev, grad_dev, sq_dev, *cfg, l->info);
  BRS_HIP_TRY(l, hipGetLastError());
  return BRS_OK;
}

int brs_learner_stats(brs_learner* l, brs_learner_info* out_host, void* stream) {
  if (!l) return fail<brs_learner>(nullptr, BRS_ERR_ARG, "brs_learner_stats: null handle");
  if (!out_host) return fail(l, BRS_ERR_ARG, "brs_learner_stats: null argument");
  DeviceGuard g(l->device);
  if (!g.ok) return fail(l, BRS_ERR_HIP, "brs_learner_stats: hipSetDevice failed");
  hipStream_t s = (hipStream_t)stream;
  BRS_HIP_TRY(l, hipMemcpyAsync(out_host, l->info, sizeof(brs_learner_info), hipMemcpyDeviceToHost, s));
  BRS_HIP_TRY(l, hipStreamSynchronize(s));
  return BRS_OK;
}

}  // extern "C"
