// brs_qpolicy.hpp -- the int8 actor of include/brs_qpolicy.h, the part shared by the HIP kernel (brs_qpolicy.hip) and
// the host build the CPU tests compare with the numpy reference (tests/qpolicyhost): the device image of a model, the
// per-env scalar form of steps 1-5, and (host only) the multiplier decomposition and the checks / zero-point fold of
// brs_qpolicy_set_model.
#pragma once
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/brs.h"
#include "../../include/brs_qpolicy.h"

#ifndef BRS_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BRS_HD __host__ __device__ __forceinline__
#else
#define BRS_HD inline
#endif
#endif

namespace brs {
namespace qpolicy {

constexpr int OBS = BRS_QPOLICY_OBS, HID = BRS_QPOLICY_HID, ACT = BRS_QPOLICY_ACT;
constexpr int W0_LD = 8;   // bytes per row of the first layer's weights: inputs 0..5, two zeros
constexpr int W1_LD = 80;  // bytes per row of the second layer's weights: 64 + 16 of padding, so that the 32 rows a half-wave
                           // reads 16 bytes of fall into 32 different groups of four LDS banks

// What the kernel reads: one block of plain data, copied to the device by set_model and to LDS by every workgroup.
// Biases have the input zero point folded in.  w1 is stored in the order the matrix cores consume it (w1_pos).
struct Image {
  double input_scale, out_scale;
  int32_t input_zero, oz[3];
  int32_t b0[HID], m0[HID], t0[HID], b1[HID], m1[HID], t1[HID];
  int32_t b2[ACT], m2[ACT], t2[ACT], pad[2];
  int32_t w2[ACT][HID];
  int8_t lut[2][256];
  alignas(16) int8_t w0[HID * W0_LD];
  alignas(16) int8_t w1[HID * W1_LD];
};
static_assert(sizeof(Image) % 16 == 0, "the image is copied to LDS in whole words and w1 is read 16 bytes at a time");

// Hidden unit held by accumulator register r (0..15) of M-tile mt in lane half h of a 32x32 matrix-core result.
BRS_HD int unit_of(int mt, int r, int h) { return 32 * mt + 8 * (r >> 2) + 4 * h + (r & 3); }
// Byte of a w1 row that multiplies hidden unit k: K-step k / 32, then lane half, then element -- the inverse of unit_of, so
// that element j of half h in step s is unit_of(s, j, h): a layer's requantised accumulators ARE the next B operand.
BRS_HD int w1_pos(int k) {
  const int v = k & 31;
  return (k & 32) + 16 * ((v >> 2) & 1) + 4 * (v >> 3) + (v & 3);
}

// step 1
BRS_HD int32_t quantize_input(float x, double scale, int32_t zero) {
  double v = rint((double)x / scale);
  if (v != v) v = 0.0;  // NaN -> the zero point
  v += (double)zero;
  v = v < -128.0 ? -128.0 : (v > 127.0 ? 127.0 : v);
  return (int32_t)v;
}

// step 3
BRS_HD int32_t requantize(int32_t acc, int32_t m, int32_t t, int32_t oz) {
  const int64_t p = (int64_t)acc * (int64_t)m + ((int64_t)1 << (t - 1));
  const int64_t q = (p >> t) + oz;
  return (int32_t)(q < -128 ? -128 : (q > 127 ? 127 : q));
}

// step 5
BRS_HD float dequantize_output(int32_t q, int32_t oz, double scale) { return (float)((double)(q - oz) * scale); }

// steps 1-5 for one env, one unit at a time (the kernel does the two wide layers on the matrix cores instead)
BRS_HD void act_env(const Image& im, const float* obs, float* action, int8_t* action_q) {
  int32_t q0[OBS], h0[HID], h1[HID];
  for (int i = 0; i < OBS; i++) q0[i] = quantize_input(obs[i], im.input_scale, im.input_zero);
  for (int c = 0; c < HID; c++) {
    int64_t acc = im.b0[c];
    for (int i = 0; i < OBS; i++) acc += (int32_t)im.w0[c * W0_LD + i] * q0[i];
    h0[c] = im.lut[0][requantize((int32_t)acc, im.m0[c], im.t0[c], im.oz[0]) + 128];
  }
  for (int c = 0; c < HID; c++) {
    int64_t acc = im.b1[c];
    for (int k = 0; k < HID; k++) acc += (int32_t)im.w1[c * W1_LD + w1_pos(k)] * h0[k];
    h1[c] = im.lut[1][requantize((int32_t)acc, im.m1[c], im.t1[c], im.oz[1]) + 128];
  }
  for (int a = 0; a < ACT; a++) {
    int64_t acc = im.b2[a];
    for (int k = 0; k < HID; k++) acc += im.w2[a][k] * h1[k];
    const int32_t q = requantize((int32_t)acc, im.m2[a], im.t2[a], im.oz[2]);
    action[a] = dequantize_output(q, im.oz[2], im.out_scale);
    if (action_q) action_q[a] = (int8_t)q;
  }
}

// ------------------------------------------------------------------------------------------------------------ host only
inline int quantize_multiplier(double M, int32_t* m, int32_t* t) {
  if (!m || !t || !(M > 0.0) || !isfinite(M)) return BRS_ERR_ARG;
  int e = 0;
  const double f = frexp(M, &e);                            // M = f 2^e, f in [0.5, 1)
  int64_t mm = (int64_t)floor(f * 2147483648.0 + 0.5);      // exact: f 2^31 has at most 22 fraction bits
  if (mm == ((int64_t)1 << 31)) { mm = (int64_t)1 << 30; e += 1; }
  const int tt = 31 - e;
  if (tt < 1 || tt > 62) return BRS_ERR_ARG;
  *m = (int32_t)mm;
  *t = tt;
  return BRS_OK;
}

// The checks of brs_qpolicy_set_model and the image it copies to the device.
inline int build_image(const brs_qmodel* q, Image* im, std::string* err) {
  auto bad = [&](const std::string& m) { if (err) *err = "brs_qpolicy_set_model: " + m; return (int)BRS_ERR_ARG; };
  if (!q || !im) return bad("null argument");
  static const int NIN[3] = {OBS, HID, HID}, NOUT[3] = {HID, HID, ACT};
  if (!(q->input_scale > 0.0) || !isfinite(q->input_scale)) return bad("input_scale must be positive and finite");
  if (q->input_zero < -128 || q->input_zero > 127) return bad("input_zero outside [-128, 127]");
  *im = Image{};
  im->input_scale = q->input_scale;
  im->input_zero = q->input_zero;
  int32_t z_in = q->input_zero;
  for (int k = 0; k < 3; k++) {
    const brs_qlayer& L = q->layer[k];
    const std::string name = "layer " + std::to_string(k);
    if (L.n_in != NIN[k] || L.n_out != NOUT[k]) return bad(name + ": the network must be 6-64-64-2");
    if (!L.weight || !L.bias || !L.bias_scale) return bad(name + ": null pointer");
    if ((k < 2) != (L.tanh_table != nullptr)) return bad(name + (k < 2 ? ": a hidden layer needs a tanh table" : ": the output layer takes no table"));
    if (!(L.out_scale > 0.0) || !isfinite(L.out_scale)) return bad(name + ": out_scale must be positive and finite");
    if (L.out_zero < -128 || L.out_zero > 127) return bad(name + ": out_zero outside [-128, 127]");
    if (k < 2 && (L.tanh_zero < -128 || L.tanh_zero > 127)) return bad(name + ": tanh_zero outside [-128, 127]");
    im->oz[k] = L.out_zero;
    int32_t* B = k == 0 ? im->b0 : (k == 1 ? im->b1 : im->b2);
    int32_t* Mm = k == 0 ? im->m0 : (k == 1 ? im->m1 : im->m2);
    int32_t* T = k == 0 ? im->t0 : (k == 1 ? im->t1 : im->t2);
    const int64_t span = z_in >= 0 ? 128 + (int64_t)z_in : 127 - (int64_t)z_in;  // max |q - z_in| over int8 q
    for (int c = 0; c < L.n_out; c++) {
      int64_t sum = 0, sum_abs = 0;
      for (int i = 0; i < L.n_in; i++) {
        const int64_t w = L.weight[c * L.n_in + i];
        sum += w;
        sum_abs += w < 0 ? -w : w;
      }
      const int64_t b = L.bias[c], folded = b - (int64_t)z_in * sum;
      // as specified (q - z_in), and as computed (folded bias, then int8 x int8 partial sums in any order)
      if ((b < 0 ? -b : b) + sum_abs * span > INT32_MAX || (folded < 0 ? -folded : folded) + sum_abs * 128 > INT32_MAX)
        return bad(name + ", channel " + std::to_string(c) + ": the accumulator can leave int32");
      B[c] = (int32_t)folded;
      if (quantize_multiplier(L.bias_scale[c] / L.out_scale, &Mm[c], &T[c]) != BRS_OK)
        return bad(name + ", channel " + std::to_string(c) + ": bias_scale / out_scale is not a valid multiplier");
      for (int i = 0; i < L.n_in; i++) {
        const int8_t w = L.weight[c * L.n_in + i];
        if (k == 0) im->w0[c * W0_LD + i] = w;
        else if (k == 1) im->w1[c * W1_LD + w1_pos(i)] = w;
        else im->w2[c][i] = w;
      }
    }
    if (k < 2) {
      for (int j = 0; j < 256; j++) im->lut[k][j] = L.tanh_table[j];
      z_in = L.tanh_zero;
    }
  }
  im->out_scale = q->layer[2].out_scale;
  return BRS_OK;
}

}  // namespace qpolicy
}  // namespace brs
