// brs_render.hip -- batched ray-cast rendering (include/brs_render.h) for gfx950.
//
// One workgroup = one TILE_W x TILE_H tile of one env's image, one lane per pixel: a wave covers two 32-pixel rows, so
// every store of a wave is two contiguous row segments (96 B of rgb, 128 B of depth, 32 B of seg).  The env's pose is
// read with wave-uniform loads and turned into the Scene (rotations, lookat-relative centres, fp64 folds) once per
// workgroup; the camera basis does not depend on the pose and is built once per launch on the host (a kernel argument).
// Every pixel tests every geom (at most 5): no acceleration structure.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "../../include/brs_render.h"
#include "brs_host.hpp"
#include "brs_render.hpp"

namespace {

constexpr int TILE_W = 32, TILE_H = 8;

thread_local char g_err[256];

int fail(int code, const char* msg) {
  snprintf(g_err, sizeof g_err, "brs_render: %s", msg);
  return code;
}

__global__ __launch_bounds__(TILE_W* TILE_H) void brs_render_kernel(const double* __restrict__ qpos, int nq, int has_block,
                                                                     brs::render::Camera cam, int tiles_x, int tiles_y,
                                                                     uint8_t* __restrict__ rgb, float* __restrict__ depth,
                                                                     uint8_t* __restrict__ seg) {
  using namespace brs::render;
  const int tiles = tiles_x * tiles_y;
  const int env = blockIdx.x / tiles, tile = blockIdx.x - env * tiles;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const Scene sc = make_scene(qpos + (size_t)env * nq, has_block);  // uniform: scalar loads
  const int j = tx * TILE_W + (int)(threadIdx.x % TILE_W), i = ty * TILE_H + (int)(threadIdx.x / TILE_W);
  if (i >= cam.height || j >= cam.width) return;
  const Pixel p = shade_pixel(cam, sc, (float)j + 0.5f, (float)i + 0.5f);
  const size_t pix = ((size_t)env * cam.height + i) * cam.width + j;
  rgb[3 * pix + 0] = to_u8(p.r);
  rgb[3 * pix + 1] = to_u8(p.g);
  rgb[3 * pix + 2] = to_u8(p.b);
  if (depth) depth[pix] = p.depth;
  if (seg) seg[pix] = (uint8_t)p.seg;
}

}  // namespace

extern "C" {

void brs_render_default_camera(brs_camera* cam) {
  if (cam) *cam = brs_camera{800, 800, 45.0f, 1.25f, 45.0f, -25.0f};
}

const char* brs_render_last_error(void) { return g_err; }

int brs_render(int32_t device, int32_t variant, int32_t k, const double* qpos_dev, const brs_camera* cam,
               uint8_t* rgb_dev, float* depth_dev, uint8_t* seg_dev, void* stream) {
  g_err[0] = 0;
  int32_t nq = 0;
  if (brs_sizes(variant, &nq, nullptr, nullptr, nullptr) != BRS_OK) return fail(BRS_ERR_ARG, "unknown variant");
  if (k < 1) return fail(BRS_ERR_ARG, "k must be >= 1");
  if (!cam) return fail(BRS_ERR_ARG, "cam is NULL");
  if (!qpos_dev) return fail(BRS_ERR_ARG, "qpos_dev is NULL");
  if (!rgb_dev) return fail(BRS_ERR_ARG, "rgb_dev is NULL");
  if (cam->width < 1 || cam->width > 4096 || cam->height < 1 || cam->height > 4096)
    return fail(BRS_ERR_ARG, "width and height must be in [1, 4096]");
  if (!(cam->fovy_deg > 0.0f && cam->fovy_deg < 180.0f)) return fail(BRS_ERR_ARG, "fovy_deg must be in (0, 180)");
  if (!(cam->distance > 0.0f) || !isfinite(cam->distance)) return fail(BRS_ERR_ARG, "distance must be finite and > 0");
  if (!isfinite(cam->azimuth_deg) || !isfinite(cam->elevation_deg)) return fail(BRS_ERR_ARG, "angles must be finite");
  const int tiles_x = (cam->width + TILE_W - 1) / TILE_W, tiles_y = (cam->height + TILE_H - 1) / TILE_H;
  const long long blocks = (long long)k * tiles_x * tiles_y;
  if (blocks > 0x7fffffffLL) return fail(BRS_ERR_ARG, "k x tiles exceeds the grid limit");
  std::string why;  // (unused: this entry point has always reported any unusable ordinal as an argument error)
  if (brs::host::check_device(device, "brs_render", &why) != BRS_OK) return fail(BRS_ERR_ARG, "bad device ordinal");

  const int has_block = brs::host::has_block(variant);
  const brs::render::Camera c = brs::render::make_camera(cam->width, cam->height, cam->fovy_deg, cam->distance,
                                                          cam->azimuth_deg, cam->elevation_deg);
  brs::host::DeviceGuard g(device);
  if (!g.ok) return fail(BRS_ERR_HIP, "hipSetDevice failed");
  hipLaunchKernelGGL(brs_render_kernel, dim3((unsigned)blocks), dim3(TILE_W * TILE_H), 0, (hipStream_t)stream, qpos_dev,
                     (int)nq, has_block, c, tiles_x, tiles_y, rgb_dev, depth_dev, seg_dev);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(g_err, sizeof g_err, "brs_render: launch failed: %s", hipGetErrorString(e));
    return BRS_ERR_HIP;
  }
  return BRS_OK;
}

}  // extern "C"
