// host build of balance_robot_mujoco_rl_amd/csrc/brs_render.hpp, for CPU tests only (tests/test_render_cpu.py compiles it
// with g++ into a temporary directory and compares it with the numpy reference tests/ref_render.py)
#include <stdint.h>

#include "brs_render.hpp"

using namespace brs::render;

extern "C" {

// k images of k qpos rows ([k][nq] f64); outputs [k][H][W]: rgb x3 u8, depth f32, seg / shadow u8, checker i8 (-1: none)
void rh_render(int has_block, int k, const double* qpos, int nq, int width, int height, float fovy, float distance,
               float azimuth, float elevation, uint8_t* rgb, float* depth, uint8_t* seg, uint8_t* shadow, int8_t* checker) {
  const Camera cam = make_camera(width, height, fovy, distance, azimuth, elevation);
  for (int e = 0; e < k; e++) {
    const Scene sc = make_scene(qpos + (size_t)e * nq, has_block);
    for (int i = 0; i < height; i++)
      for (int j = 0; j < width; j++) {
        const Pixel p = shade_pixel(cam, sc, (float)j + 0.5f, (float)i + 0.5f);
        const size_t pix = ((size_t)e * height + i) * width + j;
        rgb[3 * pix] = to_u8(p.r); rgb[3 * pix + 1] = to_u8(p.g); rgb[3 * pix + 2] = to_u8(p.b);
        depth[pix] = p.depth; seg[pix] = (uint8_t)p.seg; shadow[pix] = (uint8_t)p.shadow; checker[pix] = (int8_t)p.checker;
      }
  }
}

// camera-relative origin and direction of the ray through image point (px, py) of the camera
void rh_pixel_ray(int width, int height, float fovy, float distance, float azimuth, float elevation, float px, float py,
                  float* origin, float* dir) {
  const Camera cam = make_camera(width, height, fovy, distance, azimuth, elevation);
  const V3 d = pixel_dir(cam, px, py);
  origin[0] = cam.origin.x; origin[1] = cam.origin.y; origin[2] = cam.origin.z;
  dir[0] = d.x; dir[1] = d.y; dir[2] = d.z;
}

}  // extern "C"
