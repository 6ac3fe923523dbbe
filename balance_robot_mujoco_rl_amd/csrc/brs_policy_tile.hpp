// brs_policy_tile.hpp -- the matrix-core tiling of the 6-64-64 MlpPolicy towers that brs_policy.hip (rollout forwards)
// and brs_learner.hip (forward and backward of the PPO and A2C learners) share: the padded LDS image of a
// tower, its staging, the tanh and the forward of one tower for the 64 rows of a wave.  Device code only (hipcc).
//
// The towers are the one dense contraction of the MlpPolicy path (2 x 64 x 64 MACs per row and layer) and run on the MATRIX
// cores in fp32: v_mfma_f32_32x32x2_f32, exact fp32 products and accumulation.  Mapping: a wave owns 64 rows = two N-tiles of 32;
// the 64 units of a layer are two M-tiles; the product is computed TRANSPOSED, D[unit][row] = sum_k W[unit][k] act[k][row], so that
//   * the A operand is a weight (lane l: W[32 mt + l%32][k(l/32)]), read from a padded LDS copy of the tower (row stride 65 /
//     7 words: the 32 lanes of a half hit 32 different banks), staged once per 256-row workgroup;
//   * the B operand is an activation of row l%32 -- and the accumulator layout of this instruction (lane l holds rows
//     8 (r/4) + 4 (l/32) + r%4 of column l%32) is exactly "16 units of MY row per M-tile": after the tanh the output
//     registers of one layer ARE the B operands of the next (the K index is walked in accumulator order, the weights are
//     fetched to match), so activations never leave their registers: no LDS round trip, no shuffle between the layers.
// The 2- and 1-unit output layers are 32 FMAs per lane plus one cross-half shuffle.  tanh = 1 - 2 / (2^(2 x log2 e) + 1) on
// v_exp_f32 / v_rcp_f32 (absolute error ~1e-7).  brs_ddpg_tile.hpp is the same scheme for wider layers.
#pragma once
#include <hip/hip_runtime.h>

#include "brs_learner.hpp"  // OBS, HID, ACT, OFF_*: the flat parameter vector; O_*: the offsets inside a tower

namespace brs {
namespace policy_tile {

using namespace brs::learner;
static_assert(OBS == 6 && HID == 64 && ACT == 2, "the MFMA tiling below is written for the 6-64-64 MlpPolicy");

typedef float f32x16 __attribute__((ext_vector_type(16)));

// LDS image of one tower (floats): W2 [64][65], W1 [64][7], b1 [64], b2 [64], W3 [2][64], b3 [2]
constexpr int W2_LD = 65, W1_LD = 7;
constexpr int T_W2 = 0, T_W1 = T_W2 + HID * W2_LD, T_B1 = T_W1 + HID * W1_LD, T_B2 = T_B1 + HID, T_W3 = T_B2 + HID, T_B3 = T_W3 + 2 * HID,
              T_SIZE = T_B3 + 4;

// global parameter vector of a tower (W1[64][6] b1[64] W2[64][64] b2[64] W3[NOUT][64] b3[NOUT]) -> its LDS image; all threads.
// `stride`: the size of the workgroup as the caller has it, blockDim.x in the rollout kernels and a constant in the learner's
template <int NOUT> __device__ __forceinline__ void stage_tower(const float* __restrict__ w, float* __restrict__ L, const int stride) {
  const float* W1 = w + O_W1;
  const float* b1 = w + O_B1;
  const float* W2 = w + O_W2;
  const float* b2 = w + O_B2;
  const float* W3 = w + O_W3;
  const float* b3 = W3 + NOUT * HID;
  for (int i = threadIdx.x; i < HID * HID; i += stride) L[T_W2 + (i >> 6) * W2_LD + (i & 63)] = W2[i];
  for (int i = threadIdx.x; i < HID * OBS; i += stride) L[T_W1 + (i / OBS) * W1_LD + (i % OBS)] = W1[i];
  for (int i = threadIdx.x; i < HID; i += stride) { L[T_B1 + i] = b1[i]; L[T_B2 + i] = b2[i]; }
  for (int i = threadIdx.x; i < NOUT * HID; i += stride) L[T_W3 + i] = W3[i];
  if (threadIdx.x < NOUT) L[T_B3 + threadIdx.x] = b3[threadIdx.x];
}

__device__ __forceinline__ float fast_tanh(float x) {
  // 1 - 2 / (e^(2x) + 1): e = +inf -> 1, e = 0 -> -1; v_exp_f32 and v_rcp_f32 are 1-ulp instructions
  const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);
  return fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
}

// unit held by accumulator register r of M-tile mt in half h of the wave (a local `h` at the place of use): 32 mt + 8 (r / 4) + 4 h + r % 4
#define BRS_UNIT(mt, r) (32 * (mt) + 8 * ((r) >> 2) + 4 * h + ((r) & 3))

// `keep` sees what a backward pass needs while it is in registers (brs_learner.hip); the rollout kernels pass nothing
struct KeepNothing {
  __device__ __forceinline__ void h1(int, int, int, float) const {}  // (M-tile, N-tile, accumulator register, tanh output)
  __device__ __forceinline__ void h2(int, int, int, float) const {}
};

// One tower for the 64 rows of this wave.  x[nt][k]: observation k of row (32 nt + lane % 32) of the wave (both halves of
// the wave hold the same rows); out[nt][k]: output unit k for that row, complete in both halves.
template <int NOUT, class Keep = KeepNothing>
__device__ __forceinline__ void tower_forward(const float* __restrict__ L, const float (&x)[2][OBS], float (&out)[2][NOUT], Keep&& keep = Keep()) {
  const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
  f32x16 acc[2][2];
#pragma unroll
  for (int mt = 0; mt < 2; mt++)
#pragma unroll
    for (int r = 0; r < 16; r++) { const float b = L[T_B1 + BRS_UNIT(mt, r)]; acc[mt][0][r] = b; acc[mt][1][r] = b; }
  // layer 1: K = 6 = three steps of two; this half supplies feature 2 s + h
#pragma unroll
  for (int s = 0; s < 3; s++) {
    const float a0 = L[T_W1 + c * W1_LD + 2 * s + h], a1 = L[T_W1 + (32 + c) * W1_LD + 2 * s + h];
    const float b0 = h ? x[0][2 * s + 1] : x[0][2 * s], b1 = h ? x[1][2 * s + 1] : x[1][2 * s];
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
  }
  f32x16 h1[2][2];
#pragma unroll
  for (int mt = 0; mt < 2; mt++)
#pragma unroll
    for (int nt = 0; nt < 2; nt++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        h1[mt][nt][r] = fast_tanh(acc[mt][nt][r]);
        keep.h1(mt, nt, r, h1[mt][nt][r]);
      }
  // layer 2: K = 64 walked in ACCUMULATOR order: step (mtp, r) contracts the two units BRS_UNIT(mtp, r) of the two halves
#pragma unroll
  for (int mt = 0; mt < 2; mt++)
#pragma unroll
    for (int r = 0; r < 16; r++) { const float b = L[T_B2 + BRS_UNIT(mt, r)]; acc[mt][0][r] = b; acc[mt][1][r] = b; }
#pragma unroll
  for (int mtp = 0; mtp < 2; mtp++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int kin = BRS_UNIT(mtp, r);
      const float a0 = L[T_W2 + c * W2_LD + kin], a1 = L[T_W2 + (32 + c) * W2_LD + kin];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, h1[mtp][0][r], acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, h1[mtp][1][r], acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, h1[mtp][0][r], acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, h1[mtp][1][r], acc[1][1], 0, 0, 0);
    }
  // output layer on the vector ALU: this half's 32 units of each row, then the other half's partial sum
  float p[2][NOUT];
#pragma unroll
  for (int nt = 0; nt < 2; nt++)
#pragma unroll
    for (int k = 0; k < NOUT; k++) p[nt][k] = 0.0f;
#pragma unroll
  for (int mt = 0; mt < 2; mt++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const float t0 = fast_tanh(acc[mt][0][r]), t1 = fast_tanh(acc[mt][1][r]);
      keep.h2(mt, 0, r, t0); keep.h2(mt, 1, r, t1);
#pragma unroll
      for (int k = 0; k < NOUT; k++) {
        const float w3 = L[T_W3 + k * HID + BRS_UNIT(mt, r)];
        p[0][k] = fmaf(w3, t0, p[0][k]); p[1][k] = fmaf(w3, t1, p[1][k]);
      }
    }
#pragma unroll
  for (int nt = 0; nt < 2; nt++)
#pragma unroll
    for (int k = 0; k < NOUT; k++) out[nt][k] = p[nt][k] + __shfl_xor(p[nt][k], 32, 64) + L[T_B3 + k];
}

}  // namespace policy_tile
}  // namespace brs
