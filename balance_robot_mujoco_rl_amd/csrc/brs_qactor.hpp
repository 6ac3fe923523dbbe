// brs_qactor.hpp -- the int8 off-policy actor of include/brs_qpolicy.h (6 -> 300 -> ReLU -> 200 -> ReLU -> 2 -> tanh), the part
// shared by the HIP kernel (brs_qactor.hip) and the host build the CPU tests compare with the numpy reference
// (tests/qactorhost): the device image of a model, the per-env scalar form of steps 1-6, and (host only) the checks and the
// zero-point fold of brs_qpolicy_actor_set_model.  The arithmetic of single steps is brs_qpolicy.hpp's.  Image, act_env and
// build_image are templates over the hidden widths (WidthsReference, Widths256: SB3's SAC default 6 -> 256 -> 256 -> 2); the names
// without a parameter (Image, H0, H1, ...) are the reference widths'.
#pragma once
#include <stddef.h>

#include "brs_qpolicy.hpp"

namespace brs {
namespace qactor {

using qpolicy::dequantize_output;
using qpolicy::quantize_input;
using qpolicy::quantize_multiplier;
using qpolicy::requantize;
using qpolicy::unit_of;
using qpolicy::w1_pos;

constexpr int OBS = BRS_QACTOR_OBS, H0 = BRS_QACTOR_H0, H1 = BRS_QACTOR_H1, ACT = BRS_QACTOR_ACT;  // the reference widths
constexpr int W0_LD = 8;  // bytes per row of the first layer's weights: inputs 0..5, two zeros

// The hidden widths a handle can serve, one struct per architecture of include/brs_qpolicy.h (BRS_QACTOR_ARCH_*): H0 / H1 and
// the same padded to whole 32-unit tiles.  Image, act_env, build_image and the kernel are templates over it, as the SAC kernels
// are over their networks (brs_sac.hpp); another width set is another struct here and another case where the arch is dispatched.
struct WidthsReference {  // the reference's DDPG pi=[300, 200]: 10 and 7 tiles, 20 and 24 pad units
  static constexpr int ID = BRS_QACTOR_ARCH_REFERENCE, H0 = BRS_QACTOR_H0, H1 = BRS_QACTOR_H1, H0P = 320, H1P = 224;
  static constexpr const char* NETWORK = "6-300-200-2";
};
struct Widths256 {  // SB3's default [256, 256]: 8 and 8 tiles, no pad unit
  static constexpr int ID = BRS_QACTOR_ARCH_SAC_DEFAULT, H0 = BRS_QACTOR256_H0, H1 = BRS_QACTOR256_H1, H0P = 256, H1P = 256;
  static constexpr const char* NETWORK = "6-256-256-2";
};
inline bool known_arch(int32_t arch) { return arch == WidthsReference::ID || arch == Widths256::ID; }

template <class A> struct Dims {
  static_assert(A::H0P % 32 == 0 && A::H1P % 32 == 0 && A::H0P >= A::H0 && A::H1P >= A::H1 && A::H0P - A::H0 < 32 && A::H1P - A::H1 < 32, "whole tiles");
  static constexpr int MT0 = A::H0P / 32, MT1 = A::H1P / 32;
  // bytes per row of the second layer's weights: 21 (reference) or 17 ([256, 256]) groups of 16 bytes, an odd number, so that the
  // 32 rows a half-wave reads 16 bytes of fall into different groups of four LDS banks
  static constexpr int W1_LD = A::H0P + 16;
  static_assert((W1_LD / 16) % 2 == 1, "an odd number of 16-byte groups per row");
};
constexpr int H0P = WidthsReference::H0P, H1P = WidthsReference::H1P, MT0 = Dims<WidthsReference>::MT0, MT1 = Dims<WidthsReference>::MT1,
              W1_LD = Dims<WidthsReference>::W1_LD;

// Byte of a w1 row that multiplies unit k of the first hidden layer: K-step k / 32, inside it w1_pos, so that byte j of half
// h in step s is unit_of(s, j, h) and a layer's requantised accumulators ARE the next B operand.
BRS_HD int w1_at(int k) { return (k & ~31) + w1_pos(k & 31); }

// What the kernel reads: one block of plain data, copied to the device by set_model and to LDS by every workgroup.  Biases
// have the input zero point folded in; w1 is stored in the order the matrix cores consume it (w1_at).
template <class A> struct ImageT {
  double input_scale, action_scale;
  int32_t input_zero, action_zero, oz[3], pad0;
  int32_t b2[ACT], m2[ACT], t2[ACT], pad1[4];
  int32_t b0[A::H0P], m0[A::H0P], t0[A::H0P];
  int32_t b1[A::H1P], m1[A::H1P], t1[A::H1P];
  int32_t w2[ACT][A::H1P];
  int8_t lut[256];
  alignas(16) int8_t w0[A::H0P * W0_LD];
  alignas(16) int8_t w1[A::H1P * Dims<A>::W1_LD];
};
using Image = ImageT<WidthsReference>;
using Image256 = ImageT<Widths256>;
template <class A> constexpr bool image_fits() {
  static_assert(sizeof(ImageT<A>) % 16 == 0, "the image is copied to LDS 16 bytes at a time");
  static_assert(offsetof(ImageT<A>, w1) % 16 == 0 && offsetof(ImageT<A>, w0) % 16 == 0 && offsetof(ImageT<A>, b0) % 16 == 0, "16-byte reads");
  static_assert(sizeof(ImageT<A>) <= 160 * 1024, "one workgroup stages the whole image in the 160 KiB of LDS of a CDNA4 CU");
  return true;
}
static_assert(image_fits<WidthsReference>() && image_fits<Widths256>(), "both instantiations");
static_assert(sizeof(Image) == 86480 && sizeof(Image256) == 80208, "the sizes DESIGN.md 7.11 states");

// steps 3 and 4 of a hidden layer
BRS_HD int32_t requantize_relu(int32_t acc, int32_t m, int32_t t, int32_t oz) {
  const int32_t q = requantize(acc, m, t, oz);
  return q < oz ? oz : q;
}

// steps 1-6 for one env, one unit at a time (the kernel does the two wide layers on the matrix cores instead)
template <class A> BRS_HD void act_env(const ImageT<A>& im, const float* obs, float* action, int8_t* action_q) {
  constexpr int H0 = A::H0, H1 = A::H1, W1_LD = Dims<A>::W1_LD;
  int32_t q0[OBS], h0[H0], h1[H1];
  for (int i = 0; i < OBS; i++) q0[i] = quantize_input(obs[i], im.input_scale, im.input_zero);
  for (int c = 0; c < H0; c++) {
    int64_t acc = im.b0[c];
    for (int i = 0; i < OBS; i++) acc += (int32_t)im.w0[c * W0_LD + i] * q0[i];
    h0[c] = requantize_relu((int32_t)acc, im.m0[c], im.t0[c], im.oz[0]);
  }
  for (int c = 0; c < H1; c++) {
    int64_t acc = im.b1[c];
    for (int k = 0; k < H0; k++) acc += (int32_t)im.w1[c * W1_LD + w1_at(k)] * h0[k];
    h1[c] = requantize_relu((int32_t)acc, im.m1[c], im.t1[c], im.oz[1]);
  }
  for (int a = 0; a < ACT; a++) {
    int64_t acc = im.b2[a];
    for (int k = 0; k < H1; k++) acc += im.w2[a][k] * h1[k];
    const int32_t q = im.lut[requantize((int32_t)acc, im.m2[a], im.t2[a], im.oz[2]) + 128];
    action[a] = dequantize_output(q, im.action_zero, im.action_scale);
    if (action_q) action_q[a] = (int8_t)q;
  }
}

// ------------------------------------------------------------------------------------------------------------ host only
// The checks of brs_qpolicy_actor_set_model and the image it copies to the device, for the widths of A (deduced from the image).
template <class A> int build_image(const brs_qactor_model* q, ImageT<A>* im, std::string* err) {
  constexpr int H0 = A::H0, H1 = A::H1, H0P = A::H0P, H1P = A::H1P, W1_LD = Dims<A>::W1_LD;
  auto bad = [&](const std::string& m) { if (err) *err = "brs_qpolicy_actor_set_model: " + m; return (int)BRS_ERR_ARG; };
  if (!q || !im) return bad("null argument");
  static const int NIN[3] = {OBS, H0, H1}, NOUT[3] = {H0, H1, ACT}, NOUTP[3] = {H0P, H1P, ACT};
  if (!(q->input_scale > 0.0) || !isfinite(q->input_scale)) return bad("input_scale must be positive and finite");
  if (q->input_zero < -128 || q->input_zero > 127) return bad("input_zero outside [-128, 127]");
  if (!(q->action_scale > 0.0) || !isfinite(q->action_scale)) return bad("action_scale must be positive and finite");
  if (q->action_zero < -128 || q->action_zero > 127) return bad("action_zero outside [-128, 127]");
  // PADDING.  Everything starts as zero: the pad channels (at the reference widths units 300..319 and 200..223; [256, 256] has none)
  // have zero weights and a zero bias, and every weight that READS a pad unit (bytes w1_at(300..319) of a w1 row, w2[.][200..223]) is zero.  So whatever code a
  // pad unit holds cannot reach an output; it only has to be computable, hence the valid multiplier (1/2) given to it below.
  *im = ImageT<A>{};
  im->input_scale = q->input_scale;
  im->input_zero = q->input_zero;
  im->action_scale = q->action_scale;
  im->action_zero = q->action_zero;
  int32_t z_in = q->input_zero;
  for (int k = 0; k < 3; k++) {
    const brs_qlayer& L = q->layer[k];
    const std::string name = "layer " + std::to_string(k);
    if (L.n_in != NIN[k] || L.n_out != NOUT[k]) return bad(name + ": the network must be " + A::NETWORK);
    if (!L.weight || !L.bias || !L.bias_scale) return bad(name + ": null pointer");
    if ((k == 2) != (L.tanh_table != nullptr)) return bad(name + (k == 2 ? ": the output layer needs a tanh table" : ": a hidden layer takes no table"));
    if (!(L.out_scale > 0.0) || !isfinite(L.out_scale)) return bad(name + ": out_scale must be positive and finite");
    if (L.out_zero < -128 || L.out_zero > 127) return bad(name + ": out_zero outside [-128, 127]");
    im->oz[k] = L.out_zero;
    int32_t* B = k == 0 ? im->b0 : (k == 1 ? im->b1 : im->b2);
    int32_t* Mm = k == 0 ? im->m0 : (k == 1 ? im->m1 : im->m2);
    int32_t* T = k == 0 ? im->t0 : (k == 1 ? im->t1 : im->t2);
    for (int c = NOUT[k]; c < NOUTP[k]; c++) { Mm[c] = 1 << 30; T[c] = 31; }
    const int64_t span = z_in >= 0 ? 128 + (int64_t)z_in : 127 - (int64_t)z_in;  // max |q - z_in| over int8 q
    for (int c = 0; c < L.n_out; c++) {
      const std::string chan = name + ", channel " + std::to_string(c);
      int64_t sum = 0, sum_abs = 0;
      for (int i = 0; i < L.n_in; i++) {
        const int64_t w = L.weight[c * L.n_in + i];
        sum += w;
        sum_abs += w < 0 ? -w : w;
      }
      const int64_t b = L.bias[c], folded = b - (int64_t)z_in * sum;
      // as specified (q - z_in), and as computed (folded bias, then int8 x int8 partial sums in any order)
      if ((b < 0 ? -b : b) + sum_abs * span > INT32_MAX || (folded < 0 ? -folded : folded) + sum_abs * 128 > INT32_MAX)
        return bad(chan + ": the accumulator can leave int32");
      B[c] = (int32_t)folded;
      if (!(L.bias_scale[c] > 0.0) || !isfinite(L.bias_scale[c])) return bad(chan + ": bias_scale must be positive and finite");
      if (quantize_multiplier(L.bias_scale[c] / L.out_scale, &Mm[c], &T[c]) != BRS_OK)
        return bad(chan + ": bias_scale / out_scale is not a valid multiplier");
      for (int i = 0; i < L.n_in; i++) {
        const int8_t w = L.weight[c * L.n_in + i];
        if (k == 0) im->w0[c * W0_LD + i] = w;
        else if (k == 1) im->w1[c * W1_LD + w1_at(i)] = w;
        else im->w2[c][i] = w;
      }
    }
    z_in = L.out_zero;
  }
  for (int j = 0; j < 256; j++) im->lut[j] = q->layer[2].tanh_table[j];
  return BRS_OK;
}

}  // namespace qactor
}  // namespace brs
