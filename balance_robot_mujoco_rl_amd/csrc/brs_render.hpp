// brs_render.hpp -- per-pixel arithmetic of the batched ray-cast renderer.
//
// The scene is analytic: floor plane, torso box, two wheel cylinders and, on the Env03 ids, the block box.  One call of
// shade_pixel() casts the primary ray of one pixel, finds the nearest geom, shades it (headlight + the scene's
// directional light with a hard shadow ray) and returns rgb, depth along the camera's forward axis and the segmentation id.
//
// brs_render.hip runs this with one lane per pixel; make_camera() / make_scene() run once per workgroup on wave-uniform
// inputs.  The same header compiles on the host (tests/renderhost) so that the arithmetic is checked against an
// independent numpy ray caster (tests/ref_render.py) without a GPU.
//
// Precision: fp32 ray math in coordinates relative to the camera's lookat point (= the robot body position).  Everything
// that can be large (robot and block positions, floor checker phase, wheel angles) is reduced in fp64 first.
#pragma once
#include <math.h>
#include <stdint.h>

#include "brs_model.hpp"

#ifndef BRS_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BRS_HD __host__ __device__ __forceinline__
#else
#define BRS_HD inline
#endif
#endif

namespace brs {
namespace render {

enum Seg : uint8_t { SEG_BG = 0, SEG_FLOOR = 1, SEG_TORSO = 2, SEG_WHEEL_L = 3, SEG_WHEEL_R = 4, SEG_BLOCK = 5 };

// scene constants that are not geometry (geometry comes from brs_model.hpp's ModelRaw)
constexpr float kExtent = 0.8f;                // <statistic extent>: znear = 0.01 extent, zfar = 50 extent
constexpr float kZnear = 0.01f * kExtent, kZfar = 50.0f * kExtent;
constexpr double kCheckerCell = 0.1;           // groundplane: texrepeat 5 per metre, 2x2 checker -> 0.1-m squares
constexpr float kWheelSectors = 8.0f;          // wheel checker: sectors of wheel-local angle
constexpr float kHeadAmbient = 0.3f, kHeadDiffuse = 0.6f, kLightDiffuse = 0.7f;

struct V3 { float x, y, z; };
BRS_HD V3 v3(float x, float y, float z) { return V3{x, y, z}; }
BRS_HD V3 add(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
BRS_HD V3 sub(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
BRS_HD V3 mul(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
BRS_HD float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
BRS_HD V3 normalize(V3 a) { return mul(a, 1.0f / sqrtf(dot(a, a))); }

// rotation matrix, columns = the frame's axes in world coordinates
struct M3 { V3 c0, c1, c2; };
BRS_HD V3 rot(const M3& R, V3 v) { return add(add(mul(R.c0, v.x), mul(R.c1, v.y)), mul(R.c2, v.z)); }
BRS_HD V3 rot_t(const M3& R, V3 v) { return v3(dot(R.c0, v), dot(R.c1, v), dot(R.c2, v)); }

// MuJoCo quaternion (w, x, y, z), normalised in fp64
BRS_HD M3 quat_to_mat(const double* q) {
  double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
  M3 R;
  R.c0 = v3((float)(1 - 2 * (y * y + z * z)), (float)(2 * (x * y + w * z)), (float)(2 * (x * z - w * y)));
  R.c1 = v3((float)(2 * (x * y - w * z)), (float)(1 - 2 * (x * x + z * z)), (float)(2 * (y * z + w * x)));
  R.c2 = v3((float)(2 * (x * z + w * y)), (float)(2 * (y * z - w * x)), (float)(1 - 2 * (x * x + y * y)));
  return R;
}

// x - period * floor(x / period), in [0, period)
BRS_HD double fold(double x, double period) { return x - period * floor(x / period); }

struct Camera {
  V3 fwd, up, right, origin;  // origin relative to lookat: -distance * fwd
  float tan_y, aspect;        // tan(fovy / 2), width / height
  int width, height;
};

// MuJoCo's free camera (mjv_updateCamera): forward from azimuth / elevation, up in the vertical plane, right = fwd x up
BRS_HD Camera make_camera(int width, int height, float fovy_deg, float distance, float azimuth_deg, float elevation_deg) {
  const double d2r = 3.14159265358979323846 / 180.0;
  double a = azimuth_deg * d2r, e = elevation_deg * d2r;
  double ca = cos(a), sa = sin(a), ce = cos(e), se = sin(e);
  Camera c;
  c.fwd = v3((float)(ce * ca), (float)(ce * sa), (float)se);
  c.up = v3((float)(-se * ca), (float)(-se * sa), (float)ce);
  c.right = v3((float)sa, (float)-ca, 0.0f);
  c.origin = v3((float)(-distance * ce * ca), (float)(-distance * ce * sa), (float)(-distance * se));
  c.tan_y = (float)tan(0.5 * fovy_deg * d2r);
  c.aspect = (float)width / (float)height;
  c.width = width;
  c.height = height;
  return c;
}

// direction of the ray through image point (px, py) (pixel units, row 0 at the top; pixel centres at i + 1/2).  Its
// forward component is 1, so the ray parameter t IS the depth along the camera's forward axis.
BRS_HD V3 pixel_dir(const Camera& c, float px, float py) {
  float x = (2.0f * px / (float)c.width - 1.0f) * c.tan_y * c.aspect;
  float y = (1.0f - 2.0f * py / (float)c.height) * c.tan_y;
  return add(c.fwd, add(mul(c.right, x), mul(c.up, y)));
}

struct Scene {
  float floor_z;            // floor height relative to lookat
  float check_u0, check_v0; // lookat x, y folded modulo two checker cells (fp64)
  M3 Rb;                    // robot body rotation
  V3 torso_c, wheel_c[2];   // centres relative to lookat
  float wheel_phase[2];     // hinge angle with sign of the hinge axis, folded modulo the checker period (fp64)
  int has_block;
  M3 Rk;
  V3 block_c;
};

// qpos row in MuJoCo convention (include/brs.h): free joint pos3 + quat wxyz, left / right wheel hinge, [block pos3 + quat]
BRS_HD Scene make_scene(const double* qpos, int has_block) {
  const ModelRaw m{};
  Scene s;
  const double* p = qpos;
  s.floor_z = (float)(m.floor_z - p[2]);
  s.check_u0 = (float)fold(p[0], 2 * kCheckerCell);
  s.check_v0 = (float)fold(p[1], 2 * kCheckerCell);
  s.Rb = quat_to_mat(p + 3);
  s.torso_c = rot(s.Rb, v3(0, 0, (float)m.torso_gz));
  s.wheel_c[0] = rot(s.Rb, v3((float)-m.wheel_px, 0, (float)m.wheel_pz));
  s.wheel_c[1] = rot(s.Rb, v3((float)m.wheel_px, 0, (float)m.wheel_pz));
  // hinge axes: left -x, right +x.  A material point at body angle phi0 sits at phi0 + sign * theta; the pattern repeats
  // every two sectors
  const double period = 2.0 * (2.0 * 3.14159265358979323846 / kWheelSectors);
  s.wheel_phase[0] = (float)fold(-p[7], period);
  s.wheel_phase[1] = (float)fold(p[8], period);
  s.has_block = has_block;
  if (has_block) {
    s.block_c = v3((float)(p[9] - p[0]), (float)(p[10] - p[1]), (float)(p[11] - p[2]));
    s.Rk = quat_to_mat(p + 12);
  } else {
    s.block_c = v3(0, 0, 0);
    s.Rk = M3{v3(1, 0, 0), v3(0, 1, 0), v3(0, 0, 1)};
  }
  return s;
}

// ray/convex-solid interval [t_in, t_out]; n = outward normal (local frame) at t_in.  hit iff t_in <= t_out.
struct Span { float t_in, t_out; V3 n; };

// one slab |o + t d| <= h along a local axis; updates the span, axis direction `e` for the entry normal
BRS_HD void slab(Span& s, float o, float d, float h, V3 e) {
  if (fabsf(d) < 1e-20f) {
    if (fabsf(o) > h) s.t_out = -INFINITY;  // parallel and outside
    return;
  }
  float inv = 1.0f / d;
  float t1 = (-h - o) * inv, t2 = (h - o) * inv;
  float tn = fminf(t1, t2), tf = fmaxf(t1, t2);
  if (tn > s.t_in) { s.t_in = tn; s.n = d > 0 ? mul(e, -1.0f) : e; }
  s.t_out = fminf(s.t_out, tf);
}

// box of half sizes h, centre c, rotation R
BRS_HD Span hit_box(V3 o, V3 d, V3 c, const M3& R, V3 h) {
  V3 ol = rot_t(R, sub(o, c)), dl = rot_t(R, d);
  Span s{-INFINITY, INFINITY, v3(0, 0, 0)};
  slab(s, ol.x, dl.x, h.x, v3(1, 0, 0));
  slab(s, ol.y, dl.y, h.y, v3(0, 1, 0));
  slab(s, ol.z, dl.z, h.z, v3(0, 0, 1));
  return s;
}

// finite cylinder along the local x axis (radius r, half length hl): the x slab (caps) intersected with the infinite
// cylinder's quadratic.  The quadratic is solved about the point of closest approach, so that the discriminant does not
// come from the difference of two large numbers (the camera is ~40 radii away)
BRS_HD Span hit_cyl(V3 o, V3 d, V3 c, const M3& R, float r, float hl) {
  V3 ol = rot_t(R, sub(o, c)), dl = rot_t(R, d);
  Span s{-INFINITY, INFINITY, v3(0, 0, 0)};
  slab(s, ol.x, dl.x, hl, v3(1, 0, 0));
  float a = dl.y * dl.y + dl.z * dl.z;
  if (a < 1e-20f) {
    if (ol.y * ol.y + ol.z * ol.z > r * r) s.t_out = -INFINITY;
    return s;
  }
  float t0 = -(ol.y * dl.y + ol.z * dl.z) / a;
  float py = ol.y + t0 * dl.y, pz = ol.z + t0 * dl.z;
  float c0 = py * py + pz * pz - r * r;
  if (c0 > 0) { s.t_out = -INFINITY; return s; }
  float half = sqrtf(-c0 / a);
  float tn = t0 - half, tf = t0 + half;
  if (tn > s.t_in) {
    s.t_in = tn;
    s.n = mul(v3(0, ol.y + tn * dl.y, ol.z + tn * dl.z), 1.0f / r);
  }
  s.t_out = fminf(s.t_out, tf);
  return s;
}

BRS_HD bool span_hit(const Span& s) { return s.t_in <= s.t_out; }

// interval of moving geom `g` (SEG_TORSO .. SEG_BLOCK) along o + t d; normal in WORLD coordinates
BRS_HD Span hit_geom(const Scene& sc, int g, V3 o, V3 d) {
  const ModelRaw m{};
  Span s;
  if (g == SEG_TORSO) {
    s = hit_box(o, d, sc.torso_c, sc.Rb, v3((float)m.torso_s[0], (float)m.torso_s[1], (float)m.torso_s[2]));
    s.n = rot(sc.Rb, s.n);
  } else if (g == SEG_BLOCK) {
    float h = (float)m.block_s;
    s = hit_box(o, d, sc.block_c, sc.Rk, v3(h, h, h));
    s.n = rot(sc.Rk, s.n);
  } else {
    s = hit_cyl(o, d, g == SEG_WHEEL_L ? sc.wheel_c[0] : sc.wheel_c[1], sc.Rb, (float)m.wheel_r, (float)m.wheel_hl);
    s.n = rot(sc.Rb, s.n);
  }
  return s;
}

BRS_HD int last_geom(const Scene& sc) { return sc.has_block ? SEG_BLOCK : SEG_WHEEL_R; }

// hard shadow: does the ray from p toward the light cross a moving geom other than `self`?  (Every geom is convex: a
// point can only shadow itself where it faces away from the light, and there the diffuse term is zero already.)
BRS_HD bool shadowed(const Scene& sc, int self, V3 p, V3 to_light) {
  bool sh = false;
  for (int g = SEG_TORSO; g <= last_geom(sc); g++) {
    if (g == self) continue;
    Span s = hit_geom(sc, g, p, to_light);
    sh = sh || (span_hit(s) && s.t_out > 0.0f);
  }
  return sh;
}

struct Pixel { float r, g, b, depth; int seg, shadow, checker; };

BRS_HD Pixel shade_pixel(const Camera& cam, const Scene& sc, float px, float py) {
  const V3 d = pixel_dir(cam, px, py), o = cam.origin;
  const V3 vhat = normalize(d);
  Pixel out;
  // nearest geom entered inside [znear, zfar]
  float best = INFINITY;
  int seg = SEG_BG;
  V3 n = v3(0, 0, 1);
  if (d.z != 0.0f) {
    float t = (sc.floor_z - o.z) / d.z;
    if (t >= kZnear && t <= kZfar) { best = t; seg = SEG_FLOOR; n = v3(0, 0, o.z >= sc.floor_z ? 1.0f : -1.0f); }
  }
  for (int g = SEG_TORSO; g <= last_geom(sc); g++) {
    Span s = hit_geom(sc, g, o, d);
    if (span_hit(s) && s.t_in >= kZnear && s.t_in <= kZfar && s.t_in < best) { best = s.t_in; seg = g; n = s.n; }
  }
  out.seg = seg;
  out.shadow = 0;
  out.checker = -1;
  if (seg == SEG_BG) {  // skybox gradient: 0.8 grey straight up, black straight down
    float v = 0.4f * (vhat.z + 1.0f);
    out.r = out.g = out.b = v;
    out.depth = INFINITY;
    return out;
  }
  out.depth = best;
  const V3 p = add(o, mul(d, best));
  V3 albedo;
  if (seg == SEG_FLOOR) {
    const float cell = (float)kCheckerCell;
    int iu = (int)floorf((sc.check_u0 + p.x) / cell), iv = (int)floorf((sc.check_v0 + p.y) / cell);
    out.checker = (iu + iv) & 1;
    albedo = out.checker ? v3(0.1f, 0.2f, 0.3f) : v3(0.2f, 0.3f, 0.4f);
  } else if (seg == SEG_TORSO) {
    albedo = v3(0.5f, 0.5f, 0.5f);
  } else if (seg == SEG_BLOCK) {
    albedo = v3(1.0f, 0.0f, 0.0f);
  } else {
    // (selects, not indexing: a run-time index into the Scene would put it in scratch memory)
    const bool left = seg == SEG_WHEEL_L;
    V3 q = rot_t(sc.Rb, sub(p, left ? sc.wheel_c[0] : sc.wheel_c[1]));
    float phi = atan2f(q.z, q.y) - (left ? sc.wheel_phase[0] : sc.wheel_phase[1]);
    out.checker = (int)floorf(phi * (kWheelSectors / (2.0f * 3.14159265f))) & 1;
    albedo = out.checker ? v3(0.2f, 0.2f, 0.2f) : v3(0.0f, 0.0f, 0.0f);
  }
  const V3 to_light = normalize(v3(0.5f, 0.5f, 1.0f));  // the scene's directional light shines along (-0.5, -0.5, -1)
  float ld = fmaxf(0.0f, dot(n, to_light));
  if (ld > 0.0f && shadowed(sc, seg, p, to_light)) { out.shadow = 1; ld = 0.0f; }
  float hd = fmaxf(0.0f, -dot(n, vhat));
  float k = kHeadAmbient + kHeadDiffuse * hd + kLightDiffuse * ld;
  out.r = albedo.x * k;
  out.g = albedo.y * k;
  out.b = albedo.z * k;
  return out;
}

BRS_HD uint8_t to_u8(float c) { return (uint8_t)(fminf(fmaxf(c, 0.0f), 1.0f) * 255.0f + 0.5f); }

}  // namespace render
}  // namespace brs
