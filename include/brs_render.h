/*
 * brs_render.h -- batched rgb_array rendering of the balance-robot scenes (libbrs_hip.so).
 *
 * Replaces the reference's offscreen MuJoCo renderer as RecordVideo uses it (envs/RobotBaseEnv.py: render_mode
 * 'rgb_array', DEFAULT_CAMERA_CONFIG, _update_camera_follow) with a ray caster of the analytic scene: no GL, no display.
 * A visual approximation, not pixel parity with MuJoCo's OpenGL output.
 *
 * Conventions: as include/brs.h (status codes, device pointers, enqueue-only on `stream`).  brs_render performs no
 * allocation, no synchronisation and no host copy: it may be captured into a graph.
 */
#ifndef BRS_RENDER_H
#define BRS_RENDER_H
#include <stdint.h>

#include "brs.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int32_t width, height;   /* image size in pixels, each in [1, 4096] */
  float fovy_deg;          /* vertical field of view, in (0, 180) */
  float distance;          /* camera distance from the robot body position, > 0 */
  float azimuth_deg, elevation_deg;
} brs_camera;

/* 800x800, fovy 45, distance 1.25, azimuth 45, elevation -25: the reference's camera */
void brs_render_default_camera(brs_camera* cam);

/* k envs of `variant`; qpos_dev [k][nq] f64 row-major on `device` (brs.h layout, nq from brs_sizes);
 * rgb_dev [k][H][W][3] u8 (row 0 = top); depth_dev [k][H][W] f32 = distance along the camera's forward axis in metres,
 * +inf on background; seg_dev [k][H][W] u8 (0 background, 1 floor, 2 torso, 3 / 4 left / right wheel, 5 block).
 * depth_dev / seg_dev may be NULL.  Enqueues on `stream` (a hipStream_t of `device`, NULL = default stream) only. */
int brs_render(int32_t device, int32_t variant, int32_t k, const double* qpos_dev, const brs_camera* cam,
               uint8_t* rgb_dev, float* depth_dev, uint8_t* seg_dev, void* stream);

/* text of the last failed brs_render call of this thread ("" if none) */
const char* brs_render_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
