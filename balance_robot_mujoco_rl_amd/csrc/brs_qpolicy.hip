// brs_qpolicy.hip -- the int8 actor of include/brs_qpolicy.h as a HIP kernel for gfx950: what the reference does with the
// TFLite interpreter, one env at a time, before it flashes a policy (src/sb_rl.py:285-364), for all envs next to brs_step.
//
// Integer arithmetic only (brs_qpolicy.hpp holds the per-env scalar form; the host tests build it with g++).  The two
// 64-wide layers run on the int8 MATRIX cores, v_mfma_i32_32x32x32_i8, with the mapping of brs_policy.hip: a wave owns
// 64 envs = two N-tiles of 32, the 64 units of a layer are two M-tiles, and the product is computed TRANSPOSED,
// D[unit][env] = sum_k W[unit][k] q[k][env]:
//   * the accumulator layout (lane l holds rows 8 (r / 4) + 4 (l / 32) + r % 4 of column l % 32) is "16 units of MY env per
//     M-tile", so after requantisation and the tanh table the 16 registers of M-tile s, packed to 16 bytes, ARE the B operand
//     of K-step s of the next layer: no LDS round trip, no shuffle.  The K index is therefore walked in accumulator order,
//     and set_model stores the rows of W1 in that order (w1_pos), 16 bytes per (K-step, lane half): one ds_read_b128 each.
//   * A and B of this instruction use the same (lane half, byte) -> k map, so which k of a step a byte is does not matter
//     as long as both operands put the same unit there; the random-model tests (exact integer data) check it.
//   * the first layer (K = 6) is one matrix instruction per tile with the six codes in bytes 0..5 of lane half 0 and zeros
//     elsewhere; the 2-unit output layer is 32 integer multiply-adds per lane and one cross-half shuffle.
// The image (weights, folded biases, multipliers, shifts, tables: 8 KB) is staged in LDS once per 256-env workgroup.
#include <hip/hip_runtime.h>

#include <string>

#include "brs_host.hpp"
#include "brs_qpolicy.hpp"

namespace {

using namespace brs::qpolicy;

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int QPOLICY_THREADS = 256;  // 4 waves x 64 envs share one staged image

__global__ void __launch_bounds__(QPOLICY_THREADS) qpolicy_act_kernel(const Image* __restrict__ image, const int n, const float* __restrict__ obs,
                                                                      float* __restrict__ action, int8_t* __restrict__ action_q) {
  __shared__ Image im;
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(image);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&im);
    for (int i = threadIdx.x; i < (int)(sizeof(Image) / 4); i += QPOLICY_THREADS) dst[i] = src[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
  const int wave_base = blockIdx.x * QPOLICY_THREADS + (threadIdx.x & ~63);

  // step 1: the observation of env (32 nt + c) of the wave as six int8 codes; lane half 0 supplies them, half 1 zeros
  i32x4 bq[2];
#pragma unroll
  for (int nt = 0; nt < 2; nt++) {
    const int e = wave_base + 32 * nt + c;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < OBS; k++) {
      const float x = e < n ? obs[(size_t)OBS * e + k] : 0.0f;  // rows beyond n are computed and never stored
      const uint32_t q = (uint32_t)quantize_input(x, im.input_scale, im.input_zero) & 255u;
      if (k < 4) lo |= q << (8 * k); else hi |= q << (8 * (k - 4));
    }
    bq[nt] = h ? i32x4{0, 0, 0, 0} : i32x4{(int)lo, (int)hi, 0, 0};
  }

  // layer 0
  i32x16 acc[2][2];
#pragma unroll
  for (int mt = 0; mt < 2; mt++) {
#pragma unroll
    for (int r = 0; r < 16; r++) { const int b = im.b0[unit_of(mt, r, h)]; acc[mt][0][r] = b; acc[mt][1][r] = b; }
    const int* row = reinterpret_cast<const int*>(&im.w0[(32 * mt + c) * W0_LD]);
    const i32x4 a = {row[0], row[1], 0, 0};
    acc[mt][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bq[0], acc[mt][0], 0, 0, 0);
    acc[mt][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bq[1], acc[mt][1], 0, 0, 0);
  }
  // steps 3, 4 and the packing: byte j of K-step s is unit_of(s, j, h) of this lane's env
  i32x4 h0[2][2];
#pragma unroll
  for (int mt = 0; mt < 2; mt++)
#pragma unroll
    for (int nt = 0; nt < 2; nt++) {
      uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int u = unit_of(mt, r, h);
        const int q = im.lut[0][requantize(acc[mt][nt][r], im.m0[u], im.t0[u], im.oz[0]) + 128];
        w[r >> 2] |= ((uint32_t)q & 255u) << (8 * (r & 3));
      }
      h0[mt][nt] = i32x4{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
    }

  // layer 1: two K-steps of 32
#pragma unroll
  for (int mt = 0; mt < 2; mt++)
#pragma unroll
    for (int r = 0; r < 16; r++) { const int b = im.b1[unit_of(mt, r, h)]; acc[mt][0][r] = b; acc[mt][1][r] = b; }
#pragma unroll
  for (int s = 0; s < 2; s++)
#pragma unroll
    for (int mt = 0; mt < 2; mt++) {
      const i32x4 a = *reinterpret_cast<const i32x4*>(&im.w1[(32 * mt + c) * W1_LD + 32 * s + 16 * h]);
      acc[mt][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, h0[s][0], acc[mt][0], 0, 0, 0);
      acc[mt][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, h0[s][1], acc[mt][1], 0, 0, 0);
    }

  // layer 2 on the vector ALU: this half's 32 units of each env, then the other half's partial sum
  int p[2][ACT] = {{0, 0}, {0, 0}};
#pragma unroll
  for (int mt = 0; mt < 2; mt++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int u = unit_of(mt, r, h);
      const int m = im.m1[u], t = im.t1[u];
#pragma unroll
      for (int nt = 0; nt < 2; nt++) {
        const int q = im.lut[1][requantize(acc[mt][nt][r], m, t, im.oz[1]) + 128];
#pragma unroll
        for (int k = 0; k < ACT; k++) p[nt][k] += im.w2[k][u] * q;
      }
    }
#pragma unroll
  for (int nt = 0; nt < 2; nt++)
#pragma unroll
    for (int k = 0; k < ACT; k++) p[nt][k] += __shfl_xor(p[nt][k], 32, 64);

  const int i = wave_base + lane;  // lane l finishes env l of the wave: N-tile h, column c
  if (i >= n) return;
#pragma unroll
  for (int k = 0; k < ACT; k++) {
    const int q = requantize((h ? p[1][k] : p[0][k]) + im.b2[k], im.m2[k], im.t2[k], im.oz[2]);
    action[(size_t)ACT * i + k] = dequantize_output(q, im.oz[2], im.out_scale);
    if (action_q) action_q[(size_t)ACT * i + k] = (int8_t)q;
  }
}

}  // namespace

struct brs_qpolicy {
  int device = 0;
  brs::qpolicy::Image* image_dev = nullptr;
  bool has_model = false;
  std::string err;
};

using brs::host::DeviceGuard, brs::host::fail;  // fail<brs_qpolicy>(nullptr, ...): the error of a call without a handle

extern "C" {

int brs_qpolicy_create(int32_t device, brs_qpolicy** out) {
  if (!out) return fail<brs_qpolicy>(nullptr, BRS_ERR_ARG, "brs_qpolicy_create: null argument");
  *out = nullptr;
  std::string why;
  if (const int rc = brs::host::check_device(device, "brs_qpolicy_create", &why)) return fail<brs_qpolicy>(nullptr, rc, why);
  brs_qpolicy* p = new brs_qpolicy();
  p->device = device;
  DeviceGuard g(device);
  if (!g.ok || hipMalloc(&p->image_dev, sizeof(brs::qpolicy::Image)) != hipSuccess) {
    delete p;
    return fail<brs_qpolicy>(nullptr, BRS_ERR_HIP, "brs_qpolicy_create: device allocation failed");
  }
  *out = p;
  return BRS_OK;
}

int brs_qpolicy_destroy(brs_qpolicy* p) {
  if (!p) return BRS_ERR_STATE;
  {
    DeviceGuard g(p->device);
    if (p->image_dev) (void)hipFree(p->image_dev);
  }
  delete p;
  return BRS_OK;
}

const char* brs_qpolicy_last_error(const brs_qpolicy* p) { return brs::host::last_error(p); }

int brs_qpolicy_quantize_multiplier(double M, int32_t* m, int32_t* t) { return brs::qpolicy::quantize_multiplier(M, m, t); }

int brs_qpolicy_set_model(brs_qpolicy* p, const brs_qmodel* model) {
  brs::qpolicy::Image im;
  std::string why;
  const int rc = brs::qpolicy::build_image(model, &im, &why);  // before the handle: a model can be checked without a device
  if (rc != BRS_OK) return fail(p, rc, why);
  if (!p) return BRS_ERR_STATE;
  DeviceGuard g(p->device);
  if (!g.ok) return fail(p, BRS_ERR_HIP, "brs_qpolicy_set_model: hipSetDevice failed");
  // kernels enqueued earlier on any stream may still be reading the image: drain the device before overwriting it
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(p->image_dev, &im, sizeof(im), hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(p, BRS_ERR_HIP, std::string("brs_qpolicy_set_model: ") + hipGetErrorString(e));
  p->has_model = true;
  return BRS_OK;
}

int brs_qpolicy_act(brs_qpolicy* p, int32_t n, const float* obs_dev, float* action_dev, int8_t* action_q_dev, void* stream) {
  if (!p) return BRS_ERR_STATE;
  if (n <= 0 || !obs_dev || !action_dev) return fail(p, BRS_ERR_ARG, "brs_qpolicy_act: bad argument");
  if (!p->has_model) return fail(p, BRS_ERR_STATE, "brs_qpolicy_act: no model has been set");
  DeviceGuard g(p->device);
  if (!g.ok) return fail(p, BRS_ERR_HIP, "brs_qpolicy_act: hipSetDevice failed");
  hipLaunchKernelGGL(qpolicy_act_kernel, dim3((n + QPOLICY_THREADS - 1) / QPOLICY_THREADS), dim3(QPOLICY_THREADS), 0, (hipStream_t)stream,
                     p->image_dev, n, obs_dev, action_dev, action_q_dev);
  if (hipGetLastError() != hipSuccess) return fail(p, BRS_ERR_HIP, "brs_qpolicy_act: kernel launch failed");
  return BRS_OK;
}

}  // extern "C"
