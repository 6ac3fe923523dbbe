// brs_ddpg_tile.hpp -- the matrix-core tiling of the two DDPG networks that brs_offpolicy.hip (forwards) and
// brs_ddpg_learner.hip (forward and backward) share: the padded LDS image of a network, the K-chunk staging of
// its second layer and the forward of one 32-row tile per wave.  Device code only (hipcc).
//
// The scheme is brs_policy.hip's for wider layers: fp32 on the MATRIX cores (v_mfma_f32_32x32x2_f32: exact fp32 products, a
// k-ordered fma chain), the product computed TRANSPOSED, D[unit][row] = sum_k W[unit][k] h[k][row], so that the accumulator of
// one layer (lane l holds 16 units of ITS row l % 32 per M-tile) is, after the ReLU, the B operand of the next.  A wave owns 32
// rows; the widths are padded to the 32-unit tile (300 -> 320, 200 -> 224, 150 -> 160).  The first layer, the biases and the
// output layer live in LDS for the whole kernel; the second layer is staged in K-chunks of 32 input units, [H2 padded][33]
// words each, double-buffered.  Padded units get zero weight rows, zero weight columns and zero bias in the LDS image.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "brs_offpolicy.hpp"

namespace brs {
namespace ddpg_tile {

using namespace brs::offpolicy;

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int THREADS = 256, WAVE_ROWS = 32, WG_ROWS = WAVE_ROWS * (THREADS / 64);

// unit (inside its M-tile) held by accumulator register r in half h of the wave (a local `h` at the place of use)
#define BRS_UNIT(r) (8 * ((r) >> 2) + 4 * h + ((r) & 3))

template <class N> struct Tile {
  static constexpr int H1P = Padded<N>::H1P, H2P = Padded<N>::H2P, MT1 = H1P / 32, MT2 = H2P / 32;
  static constexpr int W1_LD = N::IN + 1, CH_LD = 33;  // odd strides: no bank conflict between the 32 units of an M-tile
  static constexpr int KSTEPS1 = N::IN / 2;
  // LDS image (floats): W1 [H1P][W1_LD], b1 [H1P], b2 [H2P], W3 [OUT][H2P], b3 [4], two chunks of W2 [H2P][CH_LD]
  static constexpr int L_W1 = 0, L_B1 = L_W1 + H1P * W1_LD, L_B2 = L_B1 + H1P, L_W3 = L_B2 + H2P, L_B3 = L_W3 + N::OUT * H2P, L_CH = L_B3 + 4,
                       CH_SIZE = H2P * CH_LD, L_SIZE = L_CH + 2 * CH_SIZE;
  static constexpr int CH_PER_THREAD = H2P * 32 / THREADS;  // words of a chunk each thread moves
  static_assert(N::IN % 2 == 0 && (H2P * 32) % THREADS == 0, "tiling");
  static_assert(N::OUT >= 1 && N::OUT <= 4, "the image reserves 4 words for b3 (the SAC actor of brs_sac.hpp uses all of them)");
};
// the LDS image of a kernel that walks the networks Nets one after the other: the largest of theirs
template <class... Nets> constexpr int lds_floats() {
  constexpr int n = std::max({Tile<Nets>::L_SIZE...});
  static_assert(2 * n * sizeof(float) <= 160 * 1024, "two workgroups per CU");
  return n;
}

// what stays in LDS for the whole forward; padded units and columns are written as zeros
template <class N> __device__ __forceinline__ void stage_resident(const float* __restrict__ w, float* __restrict__ L) {
  using T = Tile<N>;
  using O = Offsets<N>;
  for (int i = threadIdx.x; i < T::H1P * T::W1_LD; i += THREADS) {
    const int u = i / T::W1_LD, k = i % T::W1_LD;
    L[T::L_W1 + i] = (u < N::H1 && k < N::IN) ? w[O::W1 + u * N::IN + k] : 0.0f;
  }
  for (int i = threadIdx.x; i < T::H1P; i += THREADS) L[T::L_B1 + i] = i < N::H1 ? w[O::B1 + i] : 0.0f;
  for (int i = threadIdx.x; i < T::H2P; i += THREADS) L[T::L_B2 + i] = i < N::H2 ? w[O::B2 + i] : 0.0f;
  for (int i = threadIdx.x; i < N::OUT * T::H2P; i += THREADS) {
    const int u = i / T::H2P, k = i % T::H2P;
    L[T::L_W3 + i] = k < N::H2 ? w[O::W3 + u * N::H2 + k] : 0.0f;
  }
  if (threadIdx.x < 4) L[T::L_B3 + threadIdx.x] = threadIdx.x < N::OUT ? w[O::B3 + threadIdx.x] : 0.0f;
}

// InSeries<N>: network N in a kernel that runs several forwards of networks WITHOUT padded units one after the other (the
// [256, 256] actor and its two critics of DESIGN.md 7.12: the SAC target and the SAC actor's chain).  The same network in every
// respect; forward_tile<InSeries<N>> only fetches its chunks by another address form: one offset per thread plus a base that is the
// same for the whole workgroup, and nothing to test.  With load_chunk's offset per word the compiler keeps the 32 offsets of every
// chunk alive from one forward to the next of the same shape and spills them (128 registers in the target, 338 in the chain), and
// every reload then waits in front of its global load.  A kernel with one forward is better off with the plain form (the
// [256, 256] critic's backward kernel: no spill against 32), and so is backward_tile's rolled loop, where the 32 bases would be
// computed at run time.
template <class N> struct InSeries : N { static_assert(N::H1 % 32 == 0 && N::H2 % 32 == 0, "no padded unit"); };
template <class N> struct in_series { static constexpr bool value = false; };
template <class N> struct in_series<InSeries<N>> { static constexpr bool value = true; };

// chunk ch of the second layer: W2[all units][32 ch .. 32 ch + 31]; word e of the chunk is unit e / 32, input 32 ch + e % 32
// (a wave reads two 128-byte runs per instruction)
template <class N> __device__ __forceinline__ void load_chunk(const float* __restrict__ w, const int ch, float (&reg)[Tile<N>::CH_PER_THREAD]) {
  if constexpr (in_series<N>::value) {
    const int mine = (threadIdx.x >> 5) * N::H1 + (threadIdx.x & 31);
#pragma unroll
    for (int j = 0; j < Tile<N>::CH_PER_THREAD; j++) reg[j] = (w + Offsets<N>::W2 + (THREADS / 32) * j * N::H1 + 32 * ch)[mine];
    return;
  }
#pragma unroll
  for (int j = 0; j < Tile<N>::CH_PER_THREAD; j++) {
    const int e = threadIdx.x + THREADS * j, u = e >> 5, k = 32 * ch + (e & 31);
    reg[j] = (u < N::H2 && k < N::H1) ? w[Offsets<N>::W2 + u * N::H1 + k] : 0.0f;
  }
}
template <class N> __device__ __forceinline__ void store_chunk(float* __restrict__ buf, const float (&reg)[Tile<N>::CH_PER_THREAD]) {
#pragma unroll
  for (int j = 0; j < Tile<N>::CH_PER_THREAD; j++) {
    const int e = threadIdx.x + THREADS * j;
    buf[(e >> 5) * Tile<N>::CH_LD + (e & 31)] = reg[j];
  }
}

// The network N for the 32 rows of this wave.  xb[s]: input 2 s + (lane / 32) of row (lane % 32) of the wave's tile, the B operand
// of step s of the first layer (each half of the wave holds the inputs it supplies); out[k]: output unit k of that row, complete
// in both halves.  Called by all threads of the workgroup.
// `keep` sees what a backward pass needs while it is in registers (brs_ddpg_learner.hip); the forwards pass nothing.
struct KeepNothing {
  __device__ __forceinline__ void h1(int, int, float) const {}   // (M-tile, accumulator register, ReLU output)
  __device__ __forceinline__ void h2(int, int, float) const {}
  __device__ __forceinline__ void pre_out(int, float) const {}   // (output unit, its value before the tanh)
};
template <class N, class Keep = KeepNothing>
__device__ __forceinline__ void forward_tile(const float* __restrict__ w, float* __restrict__ L, const float (&xb)[Tile<N>::KSTEPS1],
                                             float (&out)[N::OUT], Keep&& keep = Keep()) {
  using T = Tile<N>;
  const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
  __syncthreads();  // the previous forward of this workgroup (brs_ddpg_td_target) has finished with L
  stage_resident<N>(w, L);
  float reg[T::CH_PER_THREAD];
  load_chunk<N>(w, 0, reg);
  store_chunk<N>(L + T::L_CH, reg);
  __syncthreads();
  // layer 1: K = IN in steps of two; this half supplies input 2 s + h
  f32x16 h1[T::MT1];
#pragma unroll
  for (int mt = 0; mt < T::MT1; mt++)
#pragma unroll
    for (int r = 0; r < 16; r++) h1[mt][r] = L[T::L_B1 + 32 * mt + BRS_UNIT(r)];
#pragma unroll
  for (int s = 0; s < T::KSTEPS1; s++) {
    const float b = xb[s];
#pragma unroll
    for (int mt = 0; mt < T::MT1; mt++) {
      const float a = L[T::L_W1 + (32 * mt + c) * T::W1_LD + 2 * s + h];
      h1[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, h1[mt], 0, 0, 0);
    }
  }
#pragma unroll
  for (int mt = 0; mt < T::MT1; mt++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      h1[mt][r] = relu_keep_nan(h1[mt][r]);
      keep.h1(mt, r, h1[mt][r]);
    }
  // layer 2: K = H1P walked in ACCUMULATOR order: step (ch, r) contracts the two units 32 ch + BRS_UNIT(r) of the two halves
  f32x16 acc[T::MT2];
#pragma unroll
  for (int mt = 0; mt < T::MT2; mt++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[mt][r] = L[T::L_B2 + 32 * mt + BRS_UNIT(r)];
#pragma unroll
  for (int ch = 0; ch < T::MT1; ch++) {
    if (ch + 1 < T::MT1) load_chunk<N>(w, ch + 1, reg);
    const float* __restrict__ B = L + T::L_CH + (ch & 1) * T::CH_SIZE;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const float b = h1[ch][r];
#pragma unroll
      for (int mt = 0; mt < T::MT2; mt++) {
        const float a = B[(32 * mt + c) * T::CH_LD + BRS_UNIT(r)];
        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[mt], 0, 0, 0);
      }
    }
    if (ch + 1 < T::MT1) store_chunk<N>(L + T::L_CH + ((ch + 1) & 1) * T::CH_SIZE, reg);
    __syncthreads();
  }
  // output layer on the vector ALU: this half's units of the row, then the other half's partial sum
  float p[N::OUT];
#pragma unroll
  for (int k = 0; k < N::OUT; k++) p[k] = 0.0f;
#pragma unroll
  for (int mt = 0; mt < T::MT2; mt++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const float t = relu_keep_nan(acc[mt][r]);
      keep.h2(mt, r, t);
#pragma unroll
      for (int k = 0; k < N::OUT; k++) p[k] = fmaf(L[T::L_W3 + k * T::H2P + 32 * mt + BRS_UNIT(r)], t, p[k]);
    }
#pragma unroll
  for (int k = 0; k < N::OUT; k++) {
    const float s = p[k] + __shfl_xor(p[k], 32, 64) + L[T::L_B3 + k];
    keep.pre_out(k, s);
    out[k] = N::TANH ? tanh_(s) : s;
  }
}

// row of the batch this lane feeds into the matrix cores and, in the lower half of the wave, finishes
__device__ __forceinline__ int tile_row() { return blockIdx.x * WG_ROWS + (threadIdx.x >> 6) * WAVE_ROWS + (threadIdx.x & 31); }
__device__ __forceinline__ int wave_half() { return (threadIdx.x >> 5) & 1; }
__device__ __forceinline__ bool finishes_row() { return wave_half() == 0; }
// the observation words row i feeds into the first layer from this half of the wave; rows past n read as zero
__device__ __forceinline__ void load_obs_operands(const float* __restrict__ obs, const int n, const int i, float* xb) {
#pragma unroll
  for (int s = 0; s < OBS / 2; s++) xb[s] = i < n ? obs[(size_t)OBS * i + 2 * s + wave_half()] : 0.0f;
}

// the networks of architecture A (brs_sac.hpp: Pi, Qf) as a kernel with several forwards names them: InSeries where no unit is
// padded, the plain network otherwise (the reference widths: their instantiations are what they were)
template <class N, bool PADDED = (N::H1 % 32 != 0 || N::H2 % 32 != 0)> struct series_net { using type = InSeries<N>; };
template <class N> struct series_net<N, true> { using type = N; };
template <class A> struct SeriesOf {
  using Pi = typename series_net<typename A::Pi>::type;
  using Qf = typename series_net<typename A::Qf>::type;
};

}  // namespace ddpg_tile
}  // namespace brs
