// mcba_pnp_kernels.h -- k_view_pose: the per-view board pose of mcba_pnp.h, one wavefront per view.
//
// Launched over the COMPACTED list of active views (the pose table is about 0.3 full): the host gathers the pixel rows and
// mask bytes of the views that are estimated, so entry k of every input and output below belongs to active view k.
//   * four views per 256-thread workgroup, no LDS, no barrier: the waves of a workgroup are independent;
//   * lane l holds corners l, l + 64, ... of its view in registers (LanePoints<NPL>: undistorted point + board point, 10 VGPRs a
//     corner), loaded and undistorted once and reused by every Levenberg-Marquardt iteration.  NPL = 2, 6 or 16 covers boards
//     of up to 128, 384 and 1024 corners; the launcher picks the smallest;
//   * the 28 (45 for the homography) sums of an iteration are per-lane partials folded by an xor butterfly (__shfl_xor): every
//     lane ends with the same bits, so the 6x6 Cholesky, the 9x9 Jacobi sweeps and all control flow that follows are uniform
//     across the wave without a broadcast;
//   * the camera family is a run-time switch inside the undistortion (wave-uniform: a view has one camera); the refinement works
//     on undistorted points and does not depend on it.
#pragma once
#include <hip/hip_runtime.h>
#include "mcba_pnp.h"

namespace mcba {
namespace pnp {

struct ViewPoseArgs {
  int n_active, P, max_iter;
  const double* pixel;        // [n_active][P][2]
  const uint8_t* valid;       // [n_active][P]
  const int32_t* desc;        // [n_active][2] camera, board
  const double* init;         // [n_active][16] or null
  const double* board;        // [B][P][3]
  const double* cam;          // [C][CAM_STRIDE]
  const int32_t* cam_nd;      // [C]
  const uint8_t* cam_fish;    // [C]
  const double* planes;       // [B][PLANE_STRIDE]
  double* pose;               // [n_active][16]
  double* sse;                // [n_active]
  int32_t* n_used;            // [n_active]
  int32_t* iters;             // [n_active]
  uint8_t* status;            // [n_active]
};

// ---- wave idioms shared by the per-view / per-camera / per-problem kernels (k_view_pose, k_calibrate_camera, k_hand_eye) ----
typedef double wave_double4 __attribute__((ext_vector_type(4)));   // accumulator of v_mfma_f64_16x16x4_f64

__device__ __forceinline__ void wave_fence() {
  // LDS and global accesses of one wavefront complete in issue order; the fence stops the compiler from moving them across
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// sum over the 64 lanes by the xor butterfly: every lane ends with the same bits
__device__ __forceinline__ double wave_xor_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

struct WaveReducer {
  template <int K, class Pts, class F>
  __device__ __forceinline__ void sum(const Pts& pts, F f, double* out) const {
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
#pragma unroll
    for (int i = 0; i < Pts::size(); ++i)
      if (pts.ok(i)) {
        double t[K];
        f(i, t);
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += t[k];
      }
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = wave_xor_sum(acc[k]);
  }
};

constexpr int VIEW_POSE_THREADS = 256;   // four views per workgroup

template <int NPL>
__global__ __launch_bounds__(VIEW_POSE_THREADS) void k_view_pose(ViewPoseArgs a) {
  const int k = blockIdx.x * (VIEW_POSE_THREADS / 64) + (threadIdx.x >> 6);
  if (k >= a.n_active) return;                  // (wave-uniform: whole waves leave)
  const int lane = threadIdx.x & 63;
  const int c = a.desc[2 * k], b = a.desc[2 * k + 1];
  const double* cam = a.cam + (size_t)c * CAM_STRIDE;
  LanePoints<NPL> pts;
  load_view(pts, lane, 64, a.P, a.pixel + (size_t)k * a.P * 2, a.valid + (size_t)k * a.P, a.board + (size_t)b * a.P * 3, cam,
            a.cam_nd[c], a.cam_fish[c] != 0);
  double pose[16], sse;
  int n_used, status, iters;
  view_pose(pts, WaveReducer(), cam, a.planes + (size_t)b * PLANE_STRIDE, a.init ? a.init + (size_t)k * 16 : nullptr, a.max_iter,
            pose, &sse, &n_used, &status, &iters);
  if (lane < 16) {
    double v = pose[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) v = (lane == i) ? pose[i] : v;
    a.pose[(size_t)k * 16 + lane] = v;
  }
  if (lane == 0) {
    a.sse[k] = sse;
    a.n_used[k] = n_used;
    a.iters[k] = iters;
    a.status[k] = (uint8_t)status;
  }
}

// corners per lane the launcher uses for boards of up to P corners (0: not served)
inline int view_pose_npl(int P) { return P <= 128 ? 2 : P <= 384 ? 6 : P <= 1024 ? 16 : 0; }

void view_pose_launch(const ViewPoseArgs& a, hipStream_t st);   // mcba_pnp.hip

}  // namespace pnp
}  // namespace mcba
