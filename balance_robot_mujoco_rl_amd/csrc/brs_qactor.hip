// brs_qactor.hip -- the int8 off-policy actor of include/brs_qpolicy.h (6 -> 300 -> ReLU -> 200 -> ReLU -> 2 -> tanh, the
// network DDPG, TD3 and SAC train) as a HIP kernel for gfx950.  Integer arithmetic only; brs_qactor.hpp holds the per-env
// scalar form the host tests build with g++.
//
// The scheme is brs_qpolicy.hip's, widened.  A wave owns 64 envs = two N-tiles of 32 and computes the two wide layers
// TRANSPOSED on v_mfma_i32_32x32x32_i8, D[unit][env] = sum_k W[unit][k] q[k][env]: a lane's 16 accumulators of M-tile s are 16
// units of ITS env, so requantised, ReLU'd and packed to 16 bytes they are the B operand of K-step s of the next layer -- no
// LDS round trip, no shuffle (unit_of / w1_at say which unit sits where).  300 pads to 320 = 10 M-tiles and 10 K-steps, 200
// to 224 = 7 M-tiles; brs_qactor.hpp (build_image) has the argument why the pad units cannot reach an output.
//   * layer 0: 10 M-tiles x 2 N-tiles = 20 matrix instructions; each tile is requantised and packed as soon as it is done,
//     so the live state is 32 accumulators and the 80 registers of packed activations.
//   * layer 1: 7 M-tiles x 10 K-steps x 2 N-tiles = 140 matrix instructions, one ds_read_b128 of A per (M-tile, K-step); each
//     M-tile's 32 accumulators are requantised and multiplied straight into the four partial sums of layer 2, so layer 1's
//     output is never stored.
//   * layer 2 (2 x 200) on the vector ALU, one cross-half shuffle, then the tanh table: one LDS read per action component.
// The image (85 KB: 74 KB of it the bank-padded layer-1 weights) is staged in LDS once per 256-env workgroup; a CDNA4 CU has
// 160 KiB and this kernel keeps one workgroup = one wave per SIMD on it.
//
// The kernel is a template over the hidden widths (brs_qactor.hpp: WidthsReference, Widths256) and is instantiated once per
// architecture a handle can have; the numbers above are the reference widths'.  SB3's [256, 256] is eight whole tiles per layer:
// no pad unit, 16 + 128 matrix instructions, 64 registers of packed activations, an 80 KB image (17 groups of 16 bytes per row).
#include <hip/hip_runtime.h>

#include <memory>
#include <string>

#include "../../include/brs_policy.h"
#include "brs_host.hpp"
#include "brs_qactor.hpp"

static_assert(BRS_QACTOR_ARCH_REFERENCE == BRS_ARCH_REFERENCE && BRS_QACTOR_ARCH_SAC_DEFAULT == BRS_ARCH_SAC_DEFAULT,
              "brs_qpolicy.h restates the architecture ids of brs_policy.h");

namespace {

using namespace brs::qactor;

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int QACTOR_THREADS = 256;  // 4 waves x 64 envs share one staged image

// One wave per SIMD, said to the compiler: two [256, 256] images (2 x 80,208 B) would fit a CU's LDS, so left alone it plans for two
// waves per SIMD, caps the registers at 256 and puts 32 bytes per lane in scratch; at one wave it needs 211 + 32 registers and no
// scratch.  The reference widths' image never allowed a second workgroup: that instantiation compiles to what it was without this.
template <class A>
__global__ void __launch_bounds__(QACTOR_THREADS) __attribute__((amdgpu_waves_per_eu(1, 1)))
qactor_act_kernel(const ImageT<A>* __restrict__ image, const int n, const float* __restrict__ obs, float* __restrict__ action,
                  int8_t* __restrict__ action_q) {
  using Image = ImageT<A>;
  constexpr int MT0 = Dims<A>::MT0, MT1 = Dims<A>::MT1, W1_LD = Dims<A>::W1_LD;
  __shared__ Image im;
  {
    const i32x4* src = reinterpret_cast<const i32x4*>(image);
    i32x4* dst = reinterpret_cast<i32x4*>(&im);
    for (int i = threadIdx.x; i < (int)(sizeof(Image) / 16); i += QACTOR_THREADS) dst[i] = src[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
  const int wave_base = blockIdx.x * QACTOR_THREADS + (threadIdx.x & ~63);

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

  // layer 0, M-tile by M-tile: steps 2-4 and the packing; byte j of K-step s is unit_of(s, j, h) of this lane's env
  const int oz0 = im.oz[0], oz1 = im.oz[1];
  i32x4 h0[MT0][2];
#pragma unroll
  for (int mt = 0; mt < MT0; mt++) {
    i32x16 acc[2];
#pragma unroll
    for (int r = 0; r < 16; r++) { const int b = im.b0[unit_of(mt, r, h)]; acc[0][r] = b; acc[1][r] = b; }
    const int* row = reinterpret_cast<const int*>(&im.w0[(32 * mt + c) * W0_LD]);
    const i32x4 a = {row[0], row[1], 0, 0};
    acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bq[0], acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bq[1], acc[1], 0, 0, 0);
    uint32_t w[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int u = unit_of(mt, r, h);
      const int m = im.m0[u], t = im.t0[u];
#pragma unroll
      for (int nt = 0; nt < 2; nt++) w[nt][r >> 2] |= ((uint32_t)requantize_relu(acc[nt][r], m, t, oz0) & 255u) << (8 * (r & 3));
    }
#pragma unroll
    for (int nt = 0; nt < 2; nt++) h0[mt][nt] = i32x4{(int)w[nt][0], (int)w[nt][1], (int)w[nt][2], (int)w[nt][3]};
  }

  // layers 1 and 2: an M-tile of layer 1 over its MT0 K-steps, then its 16 units of each env into layer 2's partial sums
  int p[2][ACT] = {{0, 0}, {0, 0}};
#pragma unroll 1
  for (int mt = 0; mt < MT1; mt++) {
    i32x16 acc[2];
#pragma unroll
    for (int r = 0; r < 16; r++) { const int b = im.b1[unit_of(mt, r, h)]; acc[0][r] = b; acc[1][r] = b; }
    const int8_t* row = &im.w1[(32 * mt + c) * W1_LD + 16 * h];
#pragma unroll
    for (int s = 0; s < MT0; s++) {
      const i32x4 a = *reinterpret_cast<const i32x4*>(row + 32 * s);
      acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, h0[s][0], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, h0[s][1], acc[1], 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int u = unit_of(mt, r, h);
      const int m = im.m1[u], t = im.t1[u];
#pragma unroll
      for (int nt = 0; nt < 2; nt++) {
        const int q = requantize_relu(acc[nt][r], m, t, oz1);
#pragma unroll
        for (int k = 0; k < ACT; k++) p[nt][k] += im.w2[k][u] * q;
      }
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
    const int q = im.lut[requantize((h ? p[1][k] : p[0][k]) + im.b2[k], im.m2[k], im.t2[k], im.oz[2]) + 128];
    action[(size_t)ACT * i + k] = dequantize_output(q, im.action_zero, im.action_scale);
    if (action_q) action_q[(size_t)ACT * i + k] = (int8_t)q;
  }
}

}  // namespace

struct brs_qactor {
  int device = 0;
  int arch = BRS_QACTOR_ARCH_REFERENCE;  // whose widths set_model takes and act runs, fixed at create
  void* image_dev = nullptr;             // an ImageT of that architecture
  bool has_model = false;
  std::string err;
};

using brs::host::DeviceGuard, brs::host::fail;

namespace {

template <class A> size_t image_bytes() { return sizeof(ImageT<A>); }

// build_image for the widths of A, then (with a handle) the copy to the device
template <class A> int set_model_as(brs_qactor* p, const brs_qactor_model* model) {
  const std::unique_ptr<ImageT<A>> im(new ImageT<A>);
  std::string why;
  const int rc = build_image(model, im.get(), &why);  // before the handle: a model can be checked without a device
  if (rc != BRS_OK) return fail(p, rc, why);
  if (!p) return BRS_ERR_STATE;
  DeviceGuard g(p->device);
  if (!g.ok) return fail(p, BRS_ERR_HIP, "brs_qpolicy_actor_set_model: hipSetDevice failed");
  // kernels enqueued earlier on any stream may still be reading the image: drain the device before overwriting it
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(p->image_dev, im.get(), sizeof(ImageT<A>), hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(p, BRS_ERR_HIP, std::string("brs_qpolicy_actor_set_model: ") + hipGetErrorString(e));
  p->has_model = true;
  return BRS_OK;
}

template <class A> void launch_as(brs_qactor* p, int32_t n, const float* obs_dev, float* action_dev, int8_t* action_q_dev, void* stream) {
  hipLaunchKernelGGL(qactor_act_kernel<A>, dim3((n + QACTOR_THREADS - 1) / QACTOR_THREADS), dim3(QACTOR_THREADS), 0, (hipStream_t)stream,
                     static_cast<const ImageT<A>*>(p->image_dev), n, obs_dev, action_dev, action_q_dev);
}

}  // namespace

extern "C" {

int brs_qpolicy_actor_create_arch(int32_t device, int32_t arch, brs_qactor** out) {
  const char* who = arch == BRS_QACTOR_ARCH_REFERENCE ? "brs_qpolicy_actor_create" : "brs_qpolicy_actor_create_arch";
  if (!out) return fail<brs_qactor>(nullptr, BRS_ERR_ARG, std::string(who) + ": null argument");
  *out = nullptr;
  if (!known_arch(arch))
    return fail<brs_qactor>(nullptr, BRS_ERR_ARG, "brs_qpolicy_actor_create_arch: unknown architecture " + std::to_string(arch) +
                                                      " (0: 6-300-200-2, 1: 6-256-256-2)");
  std::string why;
  if (const int rc = brs::host::check_device(device, who, &why)) return fail<brs_qactor>(nullptr, rc, why);
  brs_qactor* p = new brs_qactor();
  p->device = device;
  p->arch = arch;
  DeviceGuard g(device);
  if (!g.ok || hipMalloc(&p->image_dev, arch == Widths256::ID ? image_bytes<Widths256>() : image_bytes<WidthsReference>()) != hipSuccess) {
    delete p;
    return fail<brs_qactor>(nullptr, BRS_ERR_HIP, std::string(who) + ": device allocation failed");
  }
  *out = p;
  return BRS_OK;
}

int brs_qpolicy_actor_create(int32_t device, brs_qactor** out) { return brs_qpolicy_actor_create_arch(device, BRS_QACTOR_ARCH_REFERENCE, out); }

int brs_qpolicy_actor_destroy(brs_qactor* p) {
  if (!p) return BRS_ERR_STATE;
  {
    DeviceGuard g(p->device);
    if (p->image_dev) (void)hipFree(p->image_dev);
  }
  delete p;
  return BRS_OK;
}

const char* brs_qpolicy_actor_last_error(const brs_qactor* p) { return brs::host::last_error(p); }

int brs_qpolicy_actor_set_model(brs_qactor* p, const brs_qactor_model* model) {
  // without a handle the model is held against the reference widths
  return p && p->arch == Widths256::ID ? set_model_as<Widths256>(p, model) : set_model_as<WidthsReference>(p, model);
}

int brs_qpolicy_actor_check_model(int32_t arch, const brs_qactor_model* model) {
  if (!known_arch(arch))
    return fail<brs_qactor>(nullptr, BRS_ERR_ARG, "brs_qpolicy_actor_check_model: unknown architecture " + std::to_string(arch) +
                                                      " (0: 6-300-200-2, 1: 6-256-256-2)");
  const int rc = arch == Widths256::ID ? set_model_as<Widths256>(nullptr, model) : set_model_as<WidthsReference>(nullptr, model);
  return rc == BRS_ERR_STATE ? BRS_OK : rc;  // a good model and no handle
}

int brs_qpolicy_actor_act(brs_qactor* p, int32_t n, const float* obs_dev, float* action_dev, int8_t* action_q_dev, void* stream) {
  if (!p) return BRS_ERR_STATE;
  if (n <= 0 || !obs_dev || !action_dev) return fail(p, BRS_ERR_ARG, "brs_qpolicy_actor_act: bad argument");
  if (!p->has_model) return fail(p, BRS_ERR_STATE, "brs_qpolicy_actor_act: no model has been set");
  DeviceGuard g(p->device);
  if (!g.ok) return fail(p, BRS_ERR_HIP, "brs_qpolicy_actor_act: hipSetDevice failed");
  if (p->arch == Widths256::ID) launch_as<Widths256>(p, n, obs_dev, action_dev, action_q_dev, stream);
  else launch_as<WidthsReference>(p, n, obs_dev, action_dev, action_q_dev, stream);
  if (hipGetLastError() != hipSuccess) return fail(p, BRS_ERR_HIP, "brs_qpolicy_actor_act: kernel launch failed");
  return BRS_OK;
}

}  // extern "C"
