// mcba_warp_kernels.h -- the kernels of mcba_warp.h: k_warp_points and k_warp_map.
//
//   * k_warp_points: the forward or the inverse warp, one point per lane in a grid-stride loop; the camera (its image extent and its
//     block of control values) is chosen per point.  The pass that corrects a whole [C, F, B, P, 2] observation table is this kernel
//     over its flat list of slots.
//   * k_warp_map: one destination pixel per lane, map_coordinate_corrected, one 8-byte store -- a wavefront writes 512 contiguous
//     bytes.  blockIdx.y is the camera: a workgroup stays inside one, copies its control grid (at most 62 x 2 doubles) to LDS once
//     and every field evaluation of the Newton inverse reads it from there; the 64 pixels of a wavefront almost always share one
//     spline cell, so the 16 control points of an evaluation are LDS broadcasts.
// One barrier after the copy; no atomics, no cross-block waits.
#pragma once
#include <hip/hip_runtime.h>
// (mcba_undistort_kernels.h is the one statement of CameraTable, RemapArgs and remap_launch, and it DEFINES k_point_ops and
//  k_undistort_map, which belong to mcba_undistort.hip: in this unit they carry other names so that the library links, and nothing
//  launches these copies)
#define k_point_ops k_point_ops_copy_of_warp_unit
#define k_undistort_map k_undistort_map_copy_of_warp_unit
#include "mcba_undistort_kernels.h"
#undef k_point_ops
#undef k_undistort_map
#include "mcba_warp.h"

namespace mcba {
namespace warp {

struct FieldTable {
  const double* coef;         // [C][K][2]
  const double* size;         // [C][2] W, H
  int nx, ny, K;
};

struct WarpPointsArgs {
  long long n;
  int inverse;                // 0: raw -> corrected, 1: corrected -> raw
  FieldTable f;
  const int32_t* camera_of;   // [n] or null = camera 0
  const double* in;           // [n][2]
  double* out;                // [n][2]
  uint8_t* status;            // [n] or null
};

struct WarpMapArgs {
  undistort::CameraTable t;
  const double* iR;           // [C][9]
  FieldTable f;
  int C, H, W;
  float* maps;                // [C][H][W][2]
};

constexpr int WARP_THREADS = 256;
constexpr int WARP_POINTS_MAX_BLOCKS = 2048;      // grid cap of k_warp_points (256 CUs x 8 workgroups): beyond it lanes stride

__global__ __launch_bounds__(WARP_THREADS) void k_warp_points(WarpPointsArgs a) {
  const long long stride = (long long)gridDim.x * WARP_THREADS;
  for (long long i = (long long)blockIdx.x * WARP_THREADS + threadIdx.x; i < a.n; i += stride) {
    const int c = a.camera_of ? a.camera_of[i] : 0;
    const Field f{a.f.coef + (size_t)c * a.f.K * 2, a.f.size[2 * c], a.f.size[2 * c + 1], a.f.nx, a.f.ny};
    const double2 p = reinterpret_cast<const double2*>(a.in)[i];
    double o[2];
    const int st = a.inverse ? warp_inverse(f, p.x, p.y, o) : warp_forward(f, p.x, p.y, o);
    reinterpret_cast<double2*>(a.out)[i] = make_double2(o[0], o[1]);
    if (a.status) a.status[i] = (uint8_t)st;
  }
}

__global__ __launch_bounds__(WARP_THREADS) void k_warp_map(WarpMapArgs a) {
  __shared__ double s_coef[2 * MAX_K];
  const int c = blockIdx.y;
  const double* coef = a.f.coef + (size_t)c * a.f.K * 2;
  for (int k = threadIdx.x; k < 2 * a.f.K; k += WARP_THREADS) s_coef[k] = coef[k];
  __syncthreads();
  const long long per = (long long)a.H * a.W;
  const long long r = (long long)blockIdx.x * WARP_THREADS + threadIdx.x;
  if (r >= per) return;
  const Field f{s_coef, a.f.size[2 * c], a.f.size[2 * c + 1], a.f.nx, a.f.ny};
  const int y = (int)(r / a.W), x = (int)(r - (long long)y * a.W);
  float2 m;
  map_coordinate_corrected(a.t.cam + (size_t)c * CAM_STRIDE, a.t.nd[c], a.t.fish[c] != 0, a.iR + 9 * (size_t)c, f, (double)x, (double)y,
                           m.x, m.y);
  reinterpret_cast<float2*>(a.maps)[(size_t)c * per + r] = m;
}

}  // namespace warp
}  // namespace mcba
