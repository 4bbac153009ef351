// mcba_undistort_driver.h -- host side of the undistortion entry points that does not touch the device: argument checks, camera
// entries and the inverse rectification matrices iR = (P R)^-1.  Shared by the driver (mcba_undistort.hip) and the host build of the
// mathematics (tests/undistort_host), so that both serve the same calls with the same tables.
#pragma once
#include <math.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/mcba.h"
#include "mcba_undistort.h"

namespace mcba {
namespace undistort {

constexpr int MAX_IMAGE_SIDE = 1 << 15;   // pixel indices stay exact in float32 and a row of float32 RGB below 2^31 bytes

struct CameraPlan {
  std::vector<double> cam;          // [C][CAM_STRIDE] camera_entry of every camera
  std::vector<int32_t> cam_nd;      // [C] the camera's own coefficient count
  std::vector<uint8_t> cam_fish;    // [C]
  std::vector<double> K;            // [C][9] the camera's own matrix [fx skew cx; 0 fy cy; 0 0 1]
};

inline bool plan_cameras(const mcba_camera_set* s, const char* who, CameraPlan& out, std::string& err) {
  const std::string w(who);
  if (!s || s->C <= 0 || !s->cameras) { err = w + ": no cameras"; return false; }
  if (s->n_dist < 0 || s->n_dist > MAX_DIST) { err = w + ": n_dist must be 0 .. 14"; return false; }
  const int stride = 5 + s->n_dist;
  out.cam.assign((size_t)s->C * CAM_STRIDE, 0.0);
  out.cam_nd.resize(s->C);
  out.cam_fish.resize(s->C);
  out.K.assign((size_t)s->C * 9, 0.0);
  for (int c = 0; c < s->C; ++c) {
    const bool fish = s->is_fisheye && s->is_fisheye[c];
    const int nd = fish ? 4 : (s->camera_n_dist ? s->camera_n_dist[c] : s->n_dist);
    if (nd > s->n_dist || !pnp::supported_model(nd, fish)) {
      char msg[200];
      snprintf(msg, sizeof msg, "%s: camera %d: %d distortion coefficients (4, 5, 8, 12, 14; fisheye 4) in blocks of %d: "
               "unsupported camera family", who, c, nd, s->n_dist);
      err = msg;
      return false;
    }
    const double* blk = s->cameras + (size_t)c * stride;
    if (!(blk[0] > 0.0) || !(blk[1] > 0.0)) { err = w + ": focal lengths must be positive"; return false; }
    camera_entry(blk, nd, 0.0, false, out.cam.data() + (size_t)c * CAM_STRIDE, fish);
    out.cam_nd[c] = nd;
    out.cam_fish[c] = fish ? 1 : 0;
    double* K = out.K.data() + (size_t)c * 9;
    K[0] = blk[0]; K[1] = blk[4]; K[2] = blk[2]; K[4] = blk[1]; K[5] = blk[3]; K[8] = 1.0;
  }
  return true;
}

inline bool check_camera_index(const int32_t* index, long long n, int C, const char* who, std::string& err) {
  if (!index) return true;
  for (long long i = 0; i < n; ++i)
    if (index[i] < 0 || index[i] >= C) {
      char msg[160];
      snprintf(msg, sizeof msg, "%s: entry %lld names camera / map %d of %d", who, i, (int)index[i], C);
      err = msg;
      return false;
    }
  return true;
}

inline bool mat3_inverse(const double* M, double* out) {
  const double c0 = M[4] * M[8] - M[5] * M[7], c1 = M[5] * M[6] - M[3] * M[8], c2 = M[3] * M[7] - M[4] * M[6];
  const double det = M[0] * c0 + M[1] * c1 + M[2] * c2;
  if (!(fabs(det) > 0.0) || !(fabs(det) < 1e300)) return false;
  const double id = 1.0 / det;
  out[0] = c0 * id; out[1] = (M[2] * M[7] - M[1] * M[8]) * id; out[2] = (M[1] * M[5] - M[2] * M[4]) * id;
  out[3] = c1 * id; out[4] = (M[0] * M[8] - M[2] * M[6]) * id; out[5] = (M[2] * M[3] - M[0] * M[5]) * id;
  out[6] = c2 * id; out[7] = (M[1] * M[6] - M[0] * M[7]) * id; out[8] = (M[0] * M[4] - M[1] * M[3]) * id;
  return true;
}

// iR [C][9] = (P_c R_c)^-1; R == nullptr: identity, P == nullptr: the camera's own matrix (cv2.initUndistortRectifyMap)
inline bool inverse_rectifications(const CameraPlan& plan, const double* R, const double* P, const char* who, std::vector<double>& iR,
                                   std::string& err) {
  const size_t C = plan.cam_nd.size();
  iR.assign(C * 9, 0.0);
  for (size_t c = 0; c < C; ++c) {
    const double* Pc = P ? P + 9 * c : plan.K.data() + 9 * c;
    double PR[9];
    if (R) mat3_mul(Pc, R + 9 * c, PR);
    else for (int i = 0; i < 9; ++i) PR[i] = Pc[i];
    if (!mat3_inverse(PR, iR.data() + 9 * c)) {
      char msg[120];
      snprintf(msg, sizeof msg, "%s: camera %d: P R is singular", who, (int)c);
      err = msg;
      return false;
    }
  }
  return true;
}

inline bool check_image_format(int channels, int dtype, double border, const char* who, std::string& err) {
  const std::string w(who);
  if (channels != 1 && channels != 3) { err = w + ": images of 1 or 3 channels are served, not " + std::to_string(channels); return false; }
  if (dtype != PIXEL_U8 && dtype != PIXEL_F32) { err = w + ": unsupported pixel type " + std::to_string(dtype) + " (uint8, float32)"; return false; }
  if (!(fabs(border) < 1e30)) { err = w + ": the border value must be finite"; return false; }
  return true;
}

inline bool check_image_size(long long n, int h, int w_, const char* who, std::string& err) {
  if (n < 0 || h <= 0 || w_ <= 0 || h > MAX_IMAGE_SIDE || w_ > MAX_IMAGE_SIDE) {
    err = std::string(who) + ": image sizes must be 1 .. 32768 a side";
    return false;
  }
  return true;
}

// the images of every camera, in image order: out = camera_start [C + 1] | camera_images [n]  (index checked before)
inline void images_by_camera(const int32_t* index, int n, int C, std::vector<int32_t>& out) {
  out.assign((size_t)C + 1 + (size_t)n, 0);
  for (int i = 0; i < n; ++i) ++out[(size_t)index[i] + 1];
  for (int c = 0; c < C; ++c) out[(size_t)c + 1] += out[c];
  std::vector<int32_t> next(out.begin(), out.begin() + C);
  for (int i = 0; i < n; ++i) out[(size_t)C + 1 + (size_t)next[index[i]]++] = i;
}

inline size_t pixel_bytes(int dtype) { return dtype == PIXEL_U8 ? 1 : 4; }

}  // namespace undistort
}  // namespace mcba
