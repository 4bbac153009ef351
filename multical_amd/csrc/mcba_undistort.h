// mcba_undistort.h -- what a calibration is used for first: projecting points, undistorting points, the undistortion map of a
// camera and the bicubic remap of an image through it.
//
// Restates (paths relative to the reference's multical/):
//   Camera.project / CameraFisheye.project            camera.py:124-128, camera_fisheye.py:113-117   cv2.projectPoints
//   Camera.undistort_points                           camera.py:119-122, camera_fisheye.py:108-111   cv2.undistortPoints(P = K)
//   Camera.undistort_map                              camera.py:113-117, camera_fisheye.py:102-106   cv2.initUndistortRectifyMap
//   camera.undistort_images                           camera.py:244-258                              cv2.remap(INTER_CUBIC)
// on top of the project's own projection (project_point, distort_* of mcba_math.h) and its exact Newton inverse
// (pnp::undistort_point of mcba_pnp.h); nothing of either is restated here.
//   * coordinates are FP64 and rounded ONCE to float32, the format of the map cv2 materialises (CV_32FC2);
//   * the interpolation is float32.  Every multiply-add of cubic_weights and remap_pixel is an explicit fmaf or a single
//     operation in one fixed order, so that a build that contracts (the device, -ffp-contract=on) and one that does not (the g++
//     build of tests/undistort_host, -ffp-contract=off) execute the same IEEE operations: their images are byte-identical.
// Deviations from cv2: the inverse is the exact inverse of our projection, not cv2's fixed-point sweeps;
// the weights are exact float32 functions of the fractional coordinate, not 1/32-pixel tables of 15-bit fixed-point weights.
// MCBA_HD like mcba_pnp.h: the kernels of mcba_undistort_kernels.h and tests/undistort_host compile this source.
#pragma once
#include <stdint.h>
#include "mcba_pnp.h"

namespace mcba {
namespace undistort {

constexpr int ST_OK = 0, ST_NOT_CONVERGED = 1;     // mcba.h: MCBA_UNDISTORT_*
constexpr int PIXEL_U8 = 0, PIXEL_F32 = 1;         // mcba.h: MCBA_PIXEL_*
constexpr float CUBIC_A = -0.75f;                  // OpenCV's bicubic kernel (imgproc: interpolateCubic)

MCBA_HD double quiet_nan() { return __builtin_nan(""); }
MCBA_HD bool finite_d(double v) { return v - v == 0.0; }

// pixel of the camera-frame point X through the camera's own family; cam: a camera_entry, nd: its own coefficient count
MCBA_HD void project_any(const double* cam, int nd, bool fisheye, const double* X, double* uv) {
  const double* ext = cam + CAM_TILT;
  if (fisheye) { project_point<4, 1, false>(cam, ext, X, uv, nullptr, nullptr); return; }
  switch (nd) {
    case 4: project_point<4, 0, false>(cam, ext, X, uv, nullptr, nullptr); break;
    case 5: project_point<5, 0, false>(cam, ext, X, uv, nullptr, nullptr); break;
    case 8: project_point<8, 0, false>(cam, ext, X, uv, nullptr, nullptr); break;
    case 12: project_point<12, 0, false>(cam, ext, X, uv, nullptr, nullptr); break;
    case 14: project_point<14, 0, false>(cam, ext, X, uv, nullptr, nullptr); break;
    default: uv[0] = uv[1] = quiet_nan(); break;
  }
}

// source coordinate of destination pixel (u, v): [x y w] = iR [u v 1], iR = (P R)^-1 formed on the host, projected through the
// camera (which reads fx fy cx cy of its entry only), each coordinate rounded once to float32.  w <= 0 (behind the camera) or
// a non-finite result: (NaN, NaN), which remap_pixel turns into the border value.
MCBA_HD void map_coordinate(const double* cam, int nd, bool fisheye, const double* iR, double u, double v, float& mx, float& my) {
  double X[3], uv[2];
  X[0] = iR[0] * u + iR[1] * v + iR[2];
  X[1] = iR[3] * u + iR[4] * v + iR[5];
  X[2] = iR[6] * u + iR[7] * v + iR[8];
  if (!(X[2] > 0.0)) { mx = my = (float)quiet_nan(); return; }
  project_any(cam, nd, fisheye, X, uv);
  if (!finite_d(uv[0]) || !finite_d(uv[1])) { mx = my = (float)quiet_nan(); return; }
  mx = (float)uv[0];
  my = (float)uv[1];
}

// pixel (u, v) -> P [X/W, Y/W, 1] with [X Y W] = R [x y 1] of the undistorted normalised point (x, y); R == nullptr: identity,
// P == nullptr: the normalised point itself.  NOT_CONVERGED (outside the model's monotone range): NaN.
MCBA_HD int undistort_pixel(const double* cam, int nd, bool fisheye, const double* R, const double* P, double u, double v,
                            double* out) {
  double x, y;
  if (!pnp::undistort_point(cam, nd, fisheye, u, v, x, y)) {
    out[0] = out[1] = quiet_nan();
    return ST_NOT_CONVERGED;
  }
  if (R != nullptr) {
    const double X = R[0] * x + R[1] * y + R[2], Y = R[3] * x + R[4] * y + R[5], W = R[6] * x + R[7] * y + R[8];
    x = X / W;
    y = Y / W;
  }
  if (P != nullptr) {
    const double X = P[0] * x + P[1] * y + P[2], Y = P[3] * x + P[4] * y + P[5], W = P[6] * x + P[7] * y + P[8];
    x = X / W;
    y = Y / W;
  }
  out[0] = x;
  out[1] = y;
  return ST_OK;
}

// OpenCV's bicubic weights (A = -0.75) of the taps at floor(m) - 1 .. floor(m) + 2, t = m - floor(m).  t == 0: exactly (0, 1, 0, 0).
MCBA_HD void cubic_weights(float t, float* w) {
  const float A = CUBIC_A;
  const float x = t + 1.0f;
  w[0] = fmaf(fmaf(fmaf(A, x, -5.0f * A), x, 8.0f * A), x, -4.0f * A);
  const float p1 = fmaf(A + 2.0f, t, -(A + 3.0f));
  const float q1 = p1 * t;
  w[1] = fmaf(q1, t, 1.0f);
  const float s = 1.0f - t;
  const float p2 = fmaf(A + 2.0f, s, -(A + 3.0f));
  const float q2 = p2 * s;
  w[2] = fmaf(q2, s, 1.0f);
  const float d0 = 1.0f - w[0];
  const float d1 = d0 - w[1];
  w[3] = d1 - w[2];
}

MCBA_HD float to_float(uint8_t v) { return (float)v; }
MCBA_HD float to_float(float v) { return v; }

// the stored value of an interpolated sum: uint8 images saturate, float32 images keep the sum
MCBA_HD uint8_t saturate_u8(float s) {
  const float r = rintf(s);
  return (uint8_t)(r < 0.0f ? 0.0f : r > 255.0f ? 255.0f : r);
}

// Bicubic sample of src [Hs][Ws][CH] at (mx, my) -> out[CH], float32 sums.  A tap outside the source contributes `border`.  A
// coordinate that is not finite, or whose 16 taps all lie outside, gives exactly `border` without arithmetic -- the range test
// comes before the floor, so +-1e30 never reaches an integer conversion.  Sums: along a row first, then down the four rows.
template <int CH, class T>
MCBA_HD void remap_pixel(const T* src, int Hs, int Ws, float mx, float my, float border, float* out) {
  if (!(mx >= -2.0f && mx < (float)(Ws + 1) && my >= -2.0f && my < (float)(Hs + 1))) {
    MCBA_UNROLL
    for (int c = 0; c < CH; ++c) out[c] = border;
    return;
  }
  const float fx = floorf(mx), fy = floorf(my);
  const int ix = (int)fx - 1, iy = (int)fy - 1;       // first tap: -3 .. Ws - 1, -3 .. Hs - 1
  float wx[4], wy[4];
  cubic_weights(mx - fx, wx);
  cubic_weights(my - fy, wy);
  float rows[4][CH];
  if (ix >= 0 && ix + 3 < Ws && iy >= 0 && iy + 3 < Hs) {          // all 16 taps inside: no test per tap
    MCBA_UNROLL
    for (int j = 0; j < 4; ++j) {
      const T* p = src + ((size_t)(iy + j) * Ws + ix) * CH;
      MCBA_UNROLL
      for (int c = 0; c < CH; ++c) {
        float r = wx[0] * to_float(p[c]);
        r = fmaf(wx[1], to_float(p[CH + c]), r);
        r = fmaf(wx[2], to_float(p[2 * CH + c]), r);
        r = fmaf(wx[3], to_float(p[3 * CH + c]), r);
        rows[j][c] = r;
      }
    }
  } else {
    MCBA_UNROLL
    for (int j = 0; j < 4; ++j) {
      const int y = iy + j;
      const bool yin = y >= 0 && y < Hs;
      float tap[4][CH];
      MCBA_UNROLL
      for (int i = 0; i < 4; ++i) {
        const int x = ix + i;
        const bool in = yin && x >= 0 && x < Ws;
        const T* p = src + ((size_t)(in ? y : 0) * Ws + (in ? x : 0)) * CH;
        MCBA_UNROLL
        for (int c = 0; c < CH; ++c) tap[i][c] = in ? to_float(p[c]) : border;
      }
      MCBA_UNROLL
      for (int c = 0; c < CH; ++c) {
        float r = wx[0] * tap[0][c];
        r = fmaf(wx[1], tap[1][c], r);
        r = fmaf(wx[2], tap[2][c], r);
        r = fmaf(wx[3], tap[3][c], r);
        rows[j][c] = r;
      }
    }
  }
  MCBA_UNROLL
  for (int c = 0; c < CH; ++c) {
    float s = wy[0] * rows[0][c];
    s = fmaf(wy[1], rows[1][c], s);
    s = fmaf(wy[2], rows[2][c], s);
    s = fmaf(wy[3], rows[3][c], s);
    out[c] = s;
  }
}

}  // namespace undistort
}  // namespace mcba
