// brs_ddpg_learner.hip -- the DDPG learner of include/brs_policy.h as HIP kernels for gfx950: the gradient step
// of tools/train_ddpg_torch.py::DDPG.gradient_step (SB3 TD3.train as DDPG uses it) without torch.
//
//   ddpg_critic_backward_kernel  workgroups of 256 = 4 waves x 32 rows.  Critic forward (forward_tile of brs_ddpg_tile.hpp: fp32
//                                v_mfma_f32_32x32x2_f32, activations in accumulator layout), the loss head, then the backward:
//                                dz2 = (W3^T dz3) gate2 on the vector ALU, dz1 = (W2^T dz2) gate1 on the matrix cores -- the SAME
//                                K-chunk image of W2 read along a row gives W2^T as the A operand, output tile ch of dz1
//                                contracts over the units of dz2 in accumulator order.  The ReLU gates are bit masks taken in the
//                                forward.  h1, h2, dz2, dz1, dz3 and the per-row statistics go to the handle's scratch in
//                                [unit][sample] layout.
//   ddpg_actor_backward_kernel   the same for La = -mean Q(s, pi(s)) in one chain: actor forward, the action as a register of the
//                                half that supplies it, critic forward (gates only), dq = -1 / m, critic backward down to dz1_c,
//                                da = W1c[:, 6:8]^T dz1_c, dz3 = da (1 - a^2), actor backward.  No critic weight gradient.
//   ddpg_dw2_kernel              the weight gradients contract over SAMPLES: one wave owns a 32 x 32 tile of dW2 = dz2 h1^T and
//                                walks the samples of its split on the matrix cores, both operands read from the scratch.
//   ddpg_rows_kernel             the thin products on the vector ALU, one wave per scratch row: dW1 and db1 from a row of dz1,
//                                db2 and a column of dW3 from a row of dz2 / h2, db3 and the statistics from the per-sample rows.
//   ddpg_combine_kernel          at mp >= 512 the sample axis is split over up to 8 workgroup rows, each writes a partial row;
//                                column c of the partials is summed in ascending order in fp64.  Below that the two kernels
//                                write the gradient buffer themselves.
//   ddpg_apply_kernel            element-wise: Adam, then target += tau (param - target).
// TD3's twin critics are the same kernels with the critic's index on a free grid axis: blockIdx.y of the backward
// kernel, blockIdx.z of the two sample-contracting ones.  Critic k reads critics + k NCRITIC, keeps its activations in the k-th
// critic-sized scratch image and writes block k of the buffer (or of a partial row); one combine covers both.  What one critic
// computes does not depend on the other's presence: block k is brs_ddpg_learner_critic_grad's result byte for byte.
// SAC adds the actor's chain in two launches.  sac_actor_backward_kernel: the squashed-Gaussian actor's forward with
// the activations stored, the sample and logp (brs_sac.hpp), BOTH critics' forwards (gates only) and backwards -- per row the smaller
// Q takes dq = -1 / m, the other 0 -- into one d q / d action, the two dz3 formulas, dz3 and the row's shares into the per-sample
// rows.  sac_actor_tail_kernel: the actor's backward with four outputs from those rows, the gates re-read as the signs of the stored
// activations.  (In one kernel the compiler spills 352 registers per lane, 1,256 bytes of private memory; split, 22 and none.)  The
// weight kernels are instantiated for the SAC actor with five per-sample sums behind b3 (the temperature's gradient and four
// statistics).  SB3's 0.5
// in front of the critic loss is a `loss_scale` at the head of ddpg_critic_backward_kernel; the DDPG / TD3 calls pass 1.
// Architectures: every kernel of the SAC calls is a template over the networks it walks -- the critic's backward over
// the critic and its scratch layout, the two kernels of the actor's chain over the architecture (brs_sac.hpp: ArchReference,
// ArchSacDefault), the weight kernels over network and layout as before -- and ArchDims<A> holds what a handle of architecture A
// needs; the handle remembers its architecture and the SAC calls dispatch on it.  The reference instantiations are the kernels
// they were.
// Padding: a row past m runs on zero inputs; its dq / dz3 is zero, so every product it enters is zero, and it is left out of the
// statistics and of the 1 / m.  Padded units are zeros in the LDS image, their scratch rows are written (as zeros) by every call
// and their gradient is never stored.  No floating-point atomic, no communication between workgroups.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/brs.h"
#include "../../include/brs_policy.h"
#include "brs_ddpg_learner.hpp"
#include "brs_ddpg_tile.hpp"
#include "brs_host.hpp"
#include "brs_sac.hpp"

namespace {

using namespace brs::ddpg_learner;
using namespace brs::ddpg_tile;
using brs::learner::AdamScalars;
// (the scratch layouts Layout / Wide / Narrow and what a handle allocates of them: brs_ddpg_learner.hpp; brs_sac.hpp: ArchDims, handle_size)
using brs::sac::SAC_TAIL, brs::sac::ArchDims;

struct Scratch {
  float* base;
  int ld;
  __device__ __forceinline__ float* row(int r) const { return base + (size_t)r * ld; }
  // the k-th image of `rows` rows
  __device__ __forceinline__ Scratch image(int k, int rows) const { return Scratch{base + (size_t)k * rows * ld, ld}; }
};

// Scratch element (unit 32 mt + BRS_UNIT(r), sample i) = column(...)[UNIFORM_UNIT(mt, r) * ld]: the lane's share of the address
// (its sample and its half's 4 units) is in the pointer, what is left is the same for the whole wave
__device__ __forceinline__ float* column(const Scratch& s, int first_row, int i) { return s.row(first_row + 4 * wave_half()) + i; }
#define UNIFORM_UNIT(mt, r) (32 * (mt) + 8 * ((r) >> 2) + ((r) & 3))

__device__ __forceinline__ bool bit(const uint32_t* g, int mt, int r) { return (g[mt >> 1] >> (16 * (mt & 1) + r)) & 1u; }
__device__ __forceinline__ void set_gate(uint32_t* g, int mt, int r) { g[mt >> 1] |= 1u << (16 * (mt & 1) + r); }

// what the forward leaves for the backward: the gates as bit masks (tile mt, register r -> bit 16 (mt % 2) + r of word mt / 2), the
// outputs before the tanh, and, with STORE, the activations in the scratch column of this lane's row
template <class N, bool STORE, class Lay = Wide> struct Tape {
  uint32_t g1[(Tile<N>::MT1 + 1) / 2], g2[(Tile<N>::MT2 + 1) / 2];
  float pre[N::OUT];
  float *h1col, *h2col;  // null without STORE
  int ld;
  __device__ __forceinline__ Tape(const Scratch& s, int i)
      : h1col(STORE ? column(s, Lay::H1, i) : nullptr), h2col(STORE ? column(s, Lay::H2, i) : nullptr), ld(s.ld) {
#pragma unroll
    for (int k = 0; k < (Tile<N>::MT1 + 1) / 2; k++) g1[k] = 0u;
#pragma unroll
    for (int k = 0; k < (Tile<N>::MT2 + 1) / 2; k++) g2[k] = 0u;
  }
  __device__ __forceinline__ void h1(int mt, int r, float v) {
    if (relu_gate(v)) set_gate(g1, mt, r);
    if (STORE) h1col[UNIFORM_UNIT(mt, r) * ld] = v;
  }
  __device__ __forceinline__ void h2(int mt, int r, float v) {
    if (relu_gate(v)) set_gate(g2, mt, r);
    if (STORE) h2col[UNIFORM_UNIT(mt, r) * ld] = v;
  }
  __device__ __forceinline__ void pre_out(int k, float s) { pre[k] = s; }
};

// dz2 and dz1 of this lane's row into its scratch column
template <class Lay = Wide> struct StoreSink {
  float *dz1col, *dz2col;
  int ld;
  __device__ __forceinline__ StoreSink(const Scratch& s, int i) : dz1col(column(s, Lay::DZ1, i)), dz2col(column(s, Lay::DZ2, i)), ld(s.ld) {}
  __device__ __forceinline__ void dz2(int mt, int r, float v) { dz2col[UNIFORM_UNIT(mt, r) * ld] = v; }
  __device__ __forceinline__ void dz1(int mt, int r, float v) { dz1col[UNIFORM_UNIT(mt, r) * ld] = v; }
};
// the critic inside the actor's chain: only d q / d action is wanted, da[k] = sum_u W1c[u][6 + k] dz1[u] over this half's units
template <class Q = Critic> struct ActionSink {
  const float* W1;  // the critic's first layer in the LDS image
  float da[ACT];
  int h;
  __device__ __forceinline__ ActionSink(const float* L) : W1(L + Tile<Q>::L_W1), da{0.0f, 0.0f}, h(wave_half()) {}
  __device__ __forceinline__ void dz2(int, int, float) {}
  __device__ __forceinline__ void dz1(int mt, int r, float v) {
#pragma unroll
    for (int k = 0; k < ACT; k++) da[k] = fmaf(W1[(32 * mt + BRS_UNIT(r)) * Tile<Q>::W1_LD + OBS + k], v, da[k]);
  }
};

// Backward of network N for the 32 rows of this wave, after forward_tile on the same LDS image.  dz3[k]: d loss / d (output k before
// the tanh) of row lane % 32, the same in both halves.  RESTAGE: another network's image is in L.  Called by all threads.
template <class N, bool RESTAGE, class Sink>
__device__ __forceinline__ void backward_tile(const float* __restrict__ w, float* __restrict__ L, const float (&dz3)[N::OUT],
                                              const uint32_t* g1, const uint32_t* g2, Sink&& sink) {
  using T = Tile<N>;
  const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
  __syncthreads();  // every wave has finished with the chunk buffers (and, when restaging, with the resident image)
  if (RESTAGE) stage_resident<N>(w, L);
  float reg[T::CH_PER_THREAD];
  load_chunk<N>(w, 0, reg);
  store_chunk<N>(L + T::L_CH, reg);
  __syncthreads();
  f32x16 dz2[T::MT2];
#pragma unroll
  for (int mt = 0; mt < T::MT2; mt++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      float s = 0.0f;
#pragma unroll
      for (int k = 0; k < N::OUT; k++) s = fmaf(L[T::L_W3 + k * T::H2P + 32 * mt + BRS_UNIT(r)], dz3[k], s);
      dz2[mt][r] = bit(g2, mt, r) ? s : 0.0f;
      sink.dz2(mt, r, dz2[mt][r]);
    }
  // D[k][row] = sum_u W2[u][k] dz2[u][row]: tile ch of the input units needs chunk ch alone; A[k = c][u] = chunk[u][c], a row of
  // the image (32 consecutive words per half); u is walked in accumulator order
  // (a rolled loop: unrolled over the chunks the compiler spills ~1,000 registers per lane of the actor's chain; rolled, the gate
  // words are read with a run-time index from 20 to 64 bytes of private memory and nothing else is)
#pragma unroll 1
  for (int ch = 0; ch < T::MT1; ch++) {
    if (ch + 1 < T::MT1) load_chunk<N>(w, ch + 1, reg);
    const float* __restrict__ B = L + T::L_CH + (ch & 1) * T::CH_SIZE;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;
#pragma unroll
    for (int mt = 0; mt < T::MT2; mt++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const float a = B[(32 * mt + BRS_UNIT(r)) * T::CH_LD + c];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, dz2[mt][r], acc, 0, 0, 0);
      }
#pragma unroll
    for (int r = 0; r < 16; r++) sink.dz1(ch, r, bit(g1, ch, r) ? acc[r] : 0.0f);
    if (ch + 1 < T::MT1) store_chunk<N>(L + T::L_CH + ((ch + 1) & 1) * T::CH_SIZE, reg);
    __syncthreads();
  }
}

// blockIdx.y: which of the critics laid back to back in `critics` (and which scratch image); one critic, one image in the single call
template <class Q, class Lay> __global__ void __launch_bounds__(THREADS) ddpg_critic_backward_kernel(const float* __restrict__ critics, const int m,
                                                                                                     const float* __restrict__ obs,
                                                                                                     const float* __restrict__ act,
                                                                                                     const float* __restrict__ y, const Scratch all,
                                                                                                     const float loss_scale) {
  __shared__ float L[Tile<Q>::L_SIZE];
  const float* __restrict__ critic = critics + (size_t)blockIdx.y * nparam<Q>();
  const Scratch S = all.image(blockIdx.y, Lay::ROWS);
  const int i = tile_row();  // < gridDim.x * 128 <= S.ld
  float xb[(OBS + ACT) / 2], v[1];
  load_obs_operands(obs, m, i, xb);
  xb[OBS / 2] = i < m ? act[(size_t)ACT * i + wave_half()] : 0.0f;
  Tape<Q, true, Lay> tape(S, i);
  forward_tile<Q>(critic, L, xb, v, tape);
  CriticHead hd = {0.0f, 0.0f, 0.0f};
  if (i < m) hd = scale_head(critic_head(v[0], y[i], 1.0f / (float)m), loss_scale);  // 1 (exact) but for SAC's 0.5
  if (finishes_row()) {
    S.row(Lay::Z3)[i] = hd.dq;
    S.row(Lay::Z3 + 1)[i] = hd.loss;
    S.row(Lay::Z3 + 2)[i] = hd.q;
  }
  const float dz3[1] = {hd.dq};
  backward_tile<Q, false>(critic, L, dz3, tape.g1, tape.g2, StoreSink<Lay>(S, i));
}

__global__ void __launch_bounds__(THREADS) ddpg_actor_backward_kernel(const float* __restrict__ actor, const float* __restrict__ critic, const int m,
                                                                      const float* __restrict__ obs, const Scratch S) {
  __shared__ float L[lds_floats<Actor, Critic>()];
  const int i = tile_row();
  float sb[OBS / 2], mu[ACT], v[1], a[ACT], ga[ACT];
  load_obs_operands(obs, m, i, sb);
  Tape<Actor, true> ta(S, i);
  forward_tile<Actor>(actor, L, sb, mu, ta);
#pragma unroll
  for (int k = 0; k < ACT; k++) tanh_with_grad(ta.pre[k], &a[k], &ga[k]);
  const float xb[(OBS + ACT) / 2] = {sb[0], sb[1], sb[2], wave_half() ? a[1] : a[0]};
  Tape<Critic, false> tc(S, i);
  forward_tile<Critic>(critic, L, xb, v, tc);
  const float inv_m = 1.0f / (float)m;
  const float dq[1] = {i < m ? actor_dq(inv_m) : 0.0f};
  ActionSink<> to_action(L);
  backward_tile<Critic, false>(critic, L, dq, tc.g1, tc.g2, to_action);
  float dz3[ACT];
#pragma unroll
  for (int k = 0; k < ACT; k++) dz3[k] = (to_action.da[k] + __shfl_xor(to_action.da[k], 32, 64)) * ga[k];  // zero past m: dq is
  if (finishes_row()) {
    S.row(Wide::Z3)[i] = dz3[0];
    S.row(Wide::Z3 + 1)[i] = dz3[1];
    S.row(Wide::Z3 + 2)[i] = i < m ? actor_loss_share(v[0], inv_m) : 0.0f;
    S.row(Wide::Z3 + 3)[i] = i < m ? actor_sat_share(a, inv_m) : 0.0f;
  }
  backward_tile<Actor, true>(actor, L, dz3, ta.g1, ta.g2, StoreSink<Wide>(S, i));
}

// SAC's actor chain up to dz3.  Both halves of a wave compute the row's Philox block and its sample: the action is the B operand of
// both.  The critics are walked 0, 1 forward and 1, 0 backward, so that critic 1's resident image serves its own backward; the sink
// adds both critics' d q / d action (the unselected one's is an exact zero: its dq is).
template <class A> __global__ void __launch_bounds__(THREADS) sac_actor_backward_kernel(const float* __restrict__ actor, const float* __restrict__ critics,
                                                                                       const int m, const float* __restrict__ obs, const uint64_t seed,
                                                                                       const uint32_t draw, const int learn_alpha,
                                                                                       const float target_entropy, const Scratch S) {
  using Pi = typename A::Pi;
  using Qf = typename A::Qf;
  using PiLay = typename ArchDims<A>::PiLay;
  __shared__ float L[lds_floats<Pi, Qf>()];
  const int i = tile_row();
  const float* __restrict__ critic1 = critics + nparam<Qf>();
  float sb[OBS / 2], out[Pi::OUT], z[ACT], q0[1], q1[1];
  load_obs_operands(obs, m, i, sb);
  Tape<Pi, true, PiLay> ta(S, i);
  forward_tile<typename SeriesOf<A>::Pi>(actor, L, sb, out, ta);
  uint32_t o[4];
  brs::sac::sac_row_block(BRS_SAC_TAG_PI, seed, draw, (uint32_t)i, o);
  normal_pair(o[0], o[1], z);
  brs::sac::Sample sm;
  brs::sac::sample(out, z, sm);
  const float xb[(OBS + ACT) / 2] = {sb[0], sb[1], sb[2], wave_half() ? sm.a[1] : sm.a[0]};
  Tape<Qf, false> tc0(S, i), tc1(S, i);
  forward_tile<typename SeriesOf<A>::Qf>(critics, L, xb, q0, tc0);
  forward_tile<typename SeriesOf<A>::Qf>(critic1, L, xb, q1, tc1);
  const bool live = i < m;
  const float inv_m = 1.0f / (float)m, alpha = brs::sac::ent_coef_of<Pi>(actor);
  const int sel = brs::sac::min_select(q0[0], q1[0]);
  const float dq0[1] = {live && sel == 0 ? actor_dq(inv_m) : 0.0f}, dq1[1] = {live && sel == 1 ? actor_dq(inv_m) : 0.0f};
  ActionSink<Qf> to_action(L);
  backward_tile<Qf, false>(critic1, L, dq1, tc1.g1, tc1.g2, to_action);
  backward_tile<Qf, true>(critics, L, dq0, tc0.g1, tc0.g2, to_action);
  float dz3[Pi::OUT];
#pragma unroll
  for (int k = 0; k < ACT; k++) {
    const float da = to_action.da[k] + __shfl_xor(to_action.da[k], 32, 64);
    const float du = brs::sac::sac_du(da, sm.a[k], sm.g[k], alpha * inv_m);
    dz3[k] = live ? du : 0.0f;   // a row past m contributes exact zeros
    dz3[ACT + k] = live ? brs::sac::sac_dlog_std(du, sm.sigma[k], z[k], alpha * inv_m, out[ACT + k]) : 0.0f;
  }
  if (finishes_row()) {
    float share[SAC_TAIL];
    brs::sac::sac_shares(learn_alpha, target_entropy, alpha, sm.logp, sel ? q1[0] : q0[0], inv_m, share);
#pragma unroll
    for (int k = 0; k < Pi::OUT; k++) S.row(PiLay::Z3 + k)[i] = dz3[k];
#pragma unroll
    for (int k = 0; k < SAC_TAIL; k++) S.row(PiLay::Z3 + Pi::OUT + k)[i] = live ? share[k] : 0.0f;
  }
}

// ... and the second launch: the actor's backward from what the first left in the scratch -- dz3 in its four per-sample rows, the
// ReLU gates as the signs of the stored activations (relu_gate of the output is relu_gate of the pre-activation)
template <class A> __global__ void __launch_bounds__(THREADS) sac_actor_tail_kernel(const float* __restrict__ actor, const Scratch S) {
  using Pi = typename A::Pi;
  using PiLay = typename ArchDims<A>::PiLay;
  __shared__ float L[Tile<Pi>::L_SIZE];
  using T = Tile<Pi>;
  const int i = tile_row();  // < gridDim.x * 128 <= S.ld: every row of the padded batch was written by the first launch
  Tape<Pi, false> ta(S, i);
  const float* __restrict__ h1col = column(S, PiLay::H1, i);
  const float* __restrict__ h2col = column(S, PiLay::H2, i);
#pragma unroll
  for (int mt = 0; mt < T::MT1; mt++)
#pragma unroll
    for (int r = 0; r < 16; r++)
      if (relu_gate(h1col[UNIFORM_UNIT(mt, r) * S.ld])) set_gate(ta.g1, mt, r);
#pragma unroll
  for (int mt = 0; mt < T::MT2; mt++)
#pragma unroll
    for (int r = 0; r < 16; r++)
      if (relu_gate(h2col[UNIFORM_UNIT(mt, r) * S.ld])) set_gate(ta.g2, mt, r);
  float dz3[Pi::OUT];
#pragma unroll
  for (int k = 0; k < Pi::OUT; k++) dz3[k] = S.row(PiLay::Z3 + k)[i];
  backward_tile<Pi, true>(actor, L, dz3, ta.g1, ta.g2, StoreSink<PiLay>(S, i));
}

// where a workgroup row (blockIdx.y) of the two sample-contracting kernels reads and writes, for the network of its plane
// (blockIdx.z: 0 in the single calls, the critic's index in the twin call)
struct Split {
  int mp, span;        // samples padded to 128; samples per split (a multiple of 128)
  float* dst;          // the gradient buffer, or the first partial row
  int stride;          // floats between partial rows
  int net_stride;      // floats between the parameter blocks of two networks in a row
  int stat_at;         // where the statistics of network 0 begin in a row; network k's NSTAT follow at + k NSTAT
  __device__ __forceinline__ int begin() const { return blockIdx.y * span; }
  __device__ __forceinline__ int end() const { const int e = begin() + span; return e < mp ? e : mp; }
  __device__ __forceinline__ float* out() const { return dst + (size_t)blockIdx.y * stride + (size_t)blockIdx.z * net_stride; }
  __device__ __forceinline__ float* stat() const { return dst + (size_t)blockIdx.y * stride + stat_at + blockIdx.z * NSTAT; }
};

// dW2[u][k] = sum_s dz2[u][s] h1[k][s].  One wave per 32 x 32 tile; lane (c, h) supplies A[u = c][.] and B[.][k = c] for the
// samples s + 4 h .. s + 4 h + 3 of every group of eight (one 16-byte load per operand), four matrix instructions per group.
template <class N, class Lay> __global__ void __launch_bounds__(256) ddpg_dw2_kernel(const Scratch all, const Split sp) {
  using T = Tile<N>;
  const Scratch S = all.image(blockIdx.z, Lay::ROWS);
  const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= T::MT2 * T::MT1) return;  // the whole wave
  const int tu = tile / T::MT1, tk = tile % T::MT1, lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
  const float* __restrict__ A = S.row(Lay::DZ2 + 32 * tu + c) + 4 * h;
  const float* __restrict__ B = S.row(Lay::H1 + 32 * tk + c) + 4 * h;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.0f;
  const int s1 = sp.end();
  for (int s = sp.begin(); s < s1; s += 8) {
    const float4 a = *reinterpret_cast<const float4*>(A + s), b = *reinterpret_cast<const float4*>(B + s);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
  }
  float* __restrict__ out = sp.out() + Offsets<N>::W2;
  const int k = 32 * tk + c;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int u = 32 * tu + BRS_UNIT(r);
    if (u < N::H2 && k < N::H1) out[u * N::H1 + k] = acc[r];
  }
}

__device__ __forceinline__ float wave_sum(float v) {  // a butterfly: every lane ends with the same sum, the pairing is fixed
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One wave per row.  Rows [0, H1): dz1[u] -> dW1[u][:] and db1[u]; rows [H1, H1 + H2): dz2[u] -> db2[u], h2[u] -> dW3[:][u];
// then the OUT + NS per-sample rows -> db3 and the statistics (NS = NSTAT but for SAC's actor, whose five sums follow b3 in the
// buffer).  Lane l takes samples l, l + 64, ... of the split.
template <class N, class Lay, int NS = NSTAT> __global__ void __launch_bounds__(256) ddpg_rows_kernel(const Scratch all, const Split sp, const int m,
                                                                                      const float* __restrict__ obs, const float* __restrict__ act) {
  using O = Offsets<N>;
  const Scratch S = all.image(blockIdx.z, Lay::ROWS);
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int s0 = sp.begin() + lane, s1 = sp.end();
  float* __restrict__ out = sp.out();
  if (wv < N::H1) {
    const float* __restrict__ d1 = S.row(Lay::DZ1 + wv);
    float acc[N::IN + 1];
#pragma unroll
    for (int k = 0; k <= N::IN; k++) acc[k] = 0.0f;
    for (int s = s0; s < s1; s += 64) {
      const float d = d1[s];
#pragma unroll
      for (int k = 0; k < OBS; k++) acc[k] = fmaf(d, s < m ? obs[(size_t)OBS * s + k] : 0.0f, acc[k]);
      if (N::IN > OBS) {
#pragma unroll
        for (int k = 0; k < N::IN - OBS; k++) acc[OBS + k] = fmaf(d, s < m ? act[(size_t)ACT * s + k] : 0.0f, acc[OBS + k]);
      }
      acc[N::IN] += d;
    }
#pragma unroll
    for (int k = 0; k <= N::IN; k++) acc[k] = wave_sum(acc[k]);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < N::IN; k++) out[O::W1 + wv * N::IN + k] = acc[k];
      out[O::B1 + wv] = acc[N::IN];
    }
  } else if (wv < N::H1 + N::H2) {
    const int u = wv - N::H1;
    const float* __restrict__ d2 = S.row(Lay::DZ2 + u);
    const float* __restrict__ a2 = S.row(Lay::H2 + u);
    float acc[N::OUT + 1];
#pragma unroll
    for (int k = 0; k <= N::OUT; k++) acc[k] = 0.0f;
    for (int s = s0; s < s1; s += 64) {
      const float t = a2[s];
#pragma unroll
      for (int k = 0; k < N::OUT; k++) acc[k] = fmaf(S.row(Lay::Z3 + k)[s], t, acc[k]);
      acc[N::OUT] += d2[s];
    }
#pragma unroll
    for (int k = 0; k <= N::OUT; k++) acc[k] = wave_sum(acc[k]);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < N::OUT; k++) out[O::W3 + k * N::H2 + u] = acc[k];
      out[O::B2 + u] = acc[N::OUT];
    }
  } else if (wv < N::H1 + N::H2 + N::OUT + NS) {
    const int j = wv - N::H1 - N::H2;
    const float* __restrict__ z = S.row(Lay::Z3 + j);
    float acc = 0.0f;
    for (int s = s0; s < s1; s += 64) acc += z[s];
    acc = wave_sum(acc);
    if (lane == 0) {
      if (j < N::OUT) out[O::B3 + j] = acc;
      else sp.stat()[j - N::OUT] = acc;  // single calls: right behind b3, the last block; the twin call: behind both networks
    }
  }
}

__global__ void __launch_bounds__(256) ddpg_combine_kernel(const float* __restrict__ partial, const int G, const int len, float* __restrict__ grad) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col < len) grad[col] = combine_partials(partial, G, len, col);
}

__global__ void __launch_bounds__(256) ddpg_apply_kernel(const int n, float* __restrict__ params, const float* __restrict__ grad, float* __restrict__ m,
                                                         float* __restrict__ v, float* __restrict__ target, const AdamScalars a, const float tau) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float p = params[i], mi = m[i], vi = v[i];
  apply_element(p, mi, vi, grad[i], a);
  params[i] = p; m[i] = mi; v[i] = vi;
  if (target) target[i] = polyak(target[i], p, tau);
}

}  // namespace

struct brs_ddpg_learner {
  int device = 0, max_batch = 0, ld = 0;
  float* block = nullptr;    // the scratch rows, then MAX_SPLIT partial rows: one allocation
  float* partial = nullptr;
  size_t bytes = 0;
  bool twin = false;         // from brs_ddpg_learner_create_twin: two critic images fit the rows, a twin row fits a partial row
  bool sac = false;          // from brs_ddpg_learner_create_sac: a twin handle that also fits the SAC actor's image and row
  int arch = BRS_ARCH_REFERENCE;  // whose widths the SAC calls take; another than the reference's only with `sac`
  std::string err;
};

using brs::host::DeviceGuard, brs::host::fail, brs::host::launch_on;

namespace {

// what a gradient call needs of its handle, in the order the ABI checks it: the reference widths, a twin handle, a SAC handle, m rows
enum : unsigned { REFERENCE_ARCH = 1, TWIN = 2, SAC = 4 };
struct Needs {
  int m;
  unsigned of_handle;
  const char* operator()(const brs_ddpg_learner* l) const {
    if (of_handle & REFERENCE_ARCH)
      if (const char* why = BRS_REFERENCE_ARCH_ONLY(l)) return why;
    if ((of_handle & TWIN) && !l->twin) return "the handle was not created with brs_ddpg_learner_create_twin";
    if ((of_handle & SAC) && !l->sac) return "the handle was not created with brs_ddpg_learner_create_sac";
    return m > l->max_batch ? "m exceeds the handle's max_batch" : nullptr;
  }
};

// the scratch view, the split of m rows and the launches after a backward kernel
template <class N, class Lay = Wide, int NETS = 1, int NS = NSTAT> void launch_weight_kernels(brs_ddpg_learner* l, int m, const float* obs, const float* act, float* grad, hipStream_t s) {
  const SampleSplit ss = sample_split(m);  // brs_ddpg_learner.hpp
  const int mp = ss.mp, span = ss.span, nsplit = ss.nsplit;
  const Scratch S{l->block, l->ld};
  // NETS networks side by side in a row of `len` floats: their parameter blocks, then their statistics
  const int len = NETS * nparam<N>() + NETS * NS;
  const Split sp{mp, span, nsplit == 1 ? grad : l->partial, len, nparam<N>(), NETS * nparam<N>()};
  hipLaunchKernelGGL((ddpg_dw2_kernel<N, Lay>), dim3((Tile<N>::MT1 * Tile<N>::MT2 + 3) / 4, nsplit, NETS), dim3(256), 0, s, S, sp);
  hipLaunchKernelGGL((ddpg_rows_kernel<N, Lay, NS>), dim3((N::H1 + N::H2 + N::OUT + NS + 3) / 4, nsplit, NETS), dim3(256), 0, s, S, sp, m, obs, act);
  if (nsplit > 1) hipLaunchKernelGGL(ddpg_combine_kernel, dim3((len + 255) / 256), dim3(256), 0, s, l->partial, nsplit, len, grad);
}

// the gradient of loss_scale mse(Q(s, a), y) for NETS critics Q laid back to back, each in a scratch image of layout Lay
template <class Q, class Lay, int NETS> void launch_critic_grad(brs_ddpg_learner* l, const float* critics, int m, const float* obs, const float* act,
                                                                const float* y, float* grad, hipStream_t s, float loss_scale) {
  hipLaunchKernelGGL((ddpg_critic_backward_kernel<Q, Lay>), dim3(pad128(m) / WG_ROWS, NETS), dim3(THREADS), 0, s, critics, m, obs, act, y,
                     Scratch{l->block, l->ld}, loss_scale);
  launch_weight_kernels<Q, Lay, NETS>(l, m, obs, act, grad, s);
}

int create(const char* who, bool twin, bool sac, int32_t device, int32_t max_batch, brs_ddpg_learner** out, int32_t arch = BRS_ARCH_REFERENCE) {
  const std::string w(who);
  if (!out) return fail<brs_ddpg_learner>(nullptr, BRS_ERR_ARG, w + ": null argument");
  *out = nullptr;
  if (!brs::sac::known_arch(arch)) return fail<brs_ddpg_learner>(nullptr, BRS_ERR_ARG, w + ": unknown architecture");
  if (max_batch < 1 || max_batch > (1 << 22)) return fail<brs_ddpg_learner>(nullptr, BRS_ERR_ARG, w + ": max_batch must be in [1, 2^22]");
  std::string why;
  if (const int rc = brs::host::check_device(device, who, &why)) return fail<brs_ddpg_learner>(nullptr, rc, why);
  DeviceGuard g(device);
  if (!g.ok) return fail<brs_ddpg_learner>(nullptr, BRS_ERR_HIP, w + ": hipSetDevice failed");
  brs_ddpg_learner* l = new brs_ddpg_learner();
  l->device = device;
  l->max_batch = max_batch;
  l->ld = pad128(max_batch);
  l->twin = twin;
  l->sac = sac;
  l->arch = arch;
  const brs::sac::HandleSize size = brs::sac::handle_size(twin, sac, arch);
  const size_t scratch = (size_t)size.scratch_rows * l->ld, partial = (size_t)MAX_SPLIT * size.partial_len, bytes = (scratch + partial) * sizeof(float);
  if (hipMalloc((void**)&l->block, bytes) != hipSuccess || hipMemset(l->block, 0, bytes) != hipSuccess) {
    if (l->block) (void)hipFree(l->block);
    delete l;
    return fail<brs_ddpg_learner>(nullptr, BRS_ERR_HIP, w + ": device allocation failed");
  }
  l->partial = l->block + scratch;
  l->bytes = bytes;
  *out = l;
  return BRS_OK;
}

}  // namespace

extern "C" {

int brs_ddpg_learner_create(int32_t device, int32_t max_batch, brs_ddpg_learner** out) {
  return create("brs_ddpg_learner_create", false, false, device, max_batch, out);
}

int brs_ddpg_learner_create_twin(int32_t device, int32_t max_batch, brs_ddpg_learner** out) {
  return create("brs_ddpg_learner_create_twin", true, false, device, max_batch, out);
}

int brs_ddpg_learner_create_sac(int32_t device, int32_t max_batch, brs_ddpg_learner** out) {
  return create("brs_ddpg_learner_create_sac", true, true, device, max_batch, out);
}

int brs_ddpg_learner_create_sac_arch(int32_t device, int32_t max_batch, int32_t arch, brs_ddpg_learner** out) {
  return create("brs_ddpg_learner_create_sac_arch", true, true, device, max_batch, out, arch);
}

int brs_ddpg_learner_destroy(brs_ddpg_learner* l) {
  if (!l) return BRS_ERR_STATE;
  {
    DeviceGuard g(l->device);
    if (l->block) (void)hipFree(l->block);
  }
  delete l;
  return BRS_OK;
}

const char* brs_ddpg_learner_last_error(const brs_ddpg_learner* l) { return brs::host::last_error(l); }

int brs_ddpg_learner_scratch(brs_ddpg_learner* l, void** scratch_dev, int64_t* bytes) {
  if (!scratch_dev || !bytes) return fail(l, BRS_ERR_ARG, "brs_ddpg_learner_scratch: null argument");
  if (!l) return fail(l, BRS_ERR_ARG, "brs_ddpg_learner_scratch: null handle");
  *scratch_dev = l->block;
  *bytes = (int64_t)l->bytes;
  return BRS_OK;
}

int brs_ddpg_learner_critic_grad(brs_ddpg_learner* l, const float* critic_dev, int32_t m, const float* obs_dev, const float* act_dev,
                                 const float* y_dev, float* grad_dev, void* stream) {
  // what needs no handle is checked first (fail() records it in the family's slot when there is none)
  if (!critic_dev || !obs_dev || !act_dev || !y_dev || !grad_dev) return fail(l, BRS_ERR_ARG, "brs_ddpg_learner_critic_grad: null argument");
  if (m < 1) return fail(l, BRS_ERR_ARG, "brs_ddpg_learner_critic_grad: m must be at least 1");
  return launch_on(l, "brs_ddpg_learner_critic_grad", Needs{m, REFERENCE_ARCH}, [&] {
    launch_critic_grad<Critic, Wide, 1>(l, critic_dev, m, obs_dev, act_dev, y_dev, grad_dev, (hipStream_t)stream, 1.0f);
  });
}

int brs_ddpg_learner_twin_critic_grad(brs_ddpg_learner* l, const float* critics_dev, int32_t m, const float* obs_dev, const float* act_dev,
                                      const float* y_dev, float* grad_dev, void* stream) {
  if (!critics_dev || !obs_dev || !act_dev || !y_dev || !grad_dev)
    return fail(l, BRS_ERR_ARG, "brs_ddpg_learner_twin_critic_grad: null argument");
  if (m < 1) return fail(l, BRS_ERR_ARG, "brs_ddpg_learner_twin_critic_grad: m must be at least 1");
  return launch_on(l, "brs_ddpg_learner_twin_critic_grad", Needs{m, REFERENCE_ARCH | TWIN}, [&] {
    launch_critic_grad<Critic, Narrow, 2>(l, critics_dev, m, obs_dev, act_dev, y_dev, grad_dev, (hipStream_t)stream, 1.0f);
  });
}

int brs_sac_twin_critic_grad(brs_ddpg_learner* l, const float* critics_dev, int32_t m, const float* obs_dev, const float* act_dev, const float* y_dev,
                             float* grad_dev, void* stream) {
  if (const char* why = brs::sac::sac_critic_grad_argument_error(critics_dev, m, obs_dev, act_dev, y_dev, grad_dev))
    return fail(l, BRS_ERR_ARG, std::string("brs_sac_twin_critic_grad: ") + why);
  return launch_on(l, "brs_sac_twin_critic_grad", Needs{m, SAC}, [&] {
    brs::sac::with_arch(l->arch, [&](auto a) {
      using A = decltype(a);
      launch_critic_grad<typename A::Qf, typename ArchDims<A>::QfLay, 2>(l, critics_dev, m, obs_dev, act_dev, y_dev, grad_dev, (hipStream_t)stream, 0.5f);
    });
  });
}

int brs_sac_actor_grad(brs_ddpg_learner* l, const float* actor_dev, const float* critics_dev, int32_t m, const float* obs_dev, uint64_t seed,
                       uint32_t draw, int32_t learn_alpha, float target_entropy, float* grad_dev, void* stream) {
  if (const char* why = brs::sac::sac_actor_grad_argument_error(actor_dev, critics_dev, m, obs_dev, target_entropy, grad_dev))
    return fail(l, BRS_ERR_ARG, std::string("brs_sac_actor_grad: ") + why);
  return launch_on(l, "brs_sac_actor_grad", Needs{m, SAC}, [&] {
    brs::sac::with_arch(l->arch, [&](auto a) {
      using A = decltype(a);
      using PiLay = typename ArchDims<A>::PiLay;
      hipStream_t s = (hipStream_t)stream;
      const dim3 grid(pad128(m) / WG_ROWS);
      hipLaunchKernelGGL(sac_actor_backward_kernel<A>, grid, dim3(THREADS), 0, s, actor_dev, critics_dev, m, obs_dev, seed, draw, learn_alpha != 0,
                         target_entropy, Scratch{l->block, l->ld});
      hipLaunchKernelGGL(sac_actor_tail_kernel<A>, grid, dim3(THREADS), 0, s, actor_dev, Scratch{l->block, l->ld});
      launch_weight_kernels<typename A::Pi, PiLay, 1, SAC_TAIL>(l, m, obs_dev, nullptr, grad_dev, s);
    });
  });
}

int brs_ddpg_learner_actor_grad(brs_ddpg_learner* l, const float* actor_dev, const float* critic_dev, int32_t m, const float* obs_dev,
                                float* grad_dev, void* stream) {
  if (!actor_dev || !critic_dev || !obs_dev || !grad_dev) return fail(l, BRS_ERR_ARG, "brs_ddpg_learner_actor_grad: null argument");
  if (m < 1) return fail(l, BRS_ERR_ARG, "brs_ddpg_learner_actor_grad: m must be at least 1");
  return launch_on(l, "brs_ddpg_learner_actor_grad", Needs{m, REFERENCE_ARCH}, [&] {
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ddpg_actor_backward_kernel, dim3(pad128(m) / WG_ROWS), dim3(THREADS), 0, s, actor_dev, critic_dev, m, obs_dev,
                       Scratch{l->block, l->ld});
    launch_weight_kernels<Actor>(l, m, obs_dev, nullptr, grad_dev, s);
  });
}

int brs_ddpg_learner_apply(brs_ddpg_learner* l, int32_t n_param, float* params_dev, const float* grad_dev, float* m_dev, float* v_dev,
                           float* target_dev, const brs_adam_config* cfg, int64_t step, float tau, void* stream) {
  if (const char* why = apply_argument_error(n_param, params_dev, grad_dev, m_dev, v_dev, cfg, step, tau))
    return fail(l, BRS_ERR_ARG, std::string("brs_ddpg_learner_apply: ") + why);
  return launch_on(l, "brs_ddpg_learner_apply", brs::host::needs_nothing, [&] {
    hipLaunchKernelGGL(ddpg_apply_kernel, dim3((unsigned)(((int64_t)n_param + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_param, params_dev,
                       grad_dev, m_dev, v_dev, target_dev, adam_scalars(*cfg, step), tau);
  });
}

}  // extern "C"
