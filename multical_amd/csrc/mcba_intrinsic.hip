// translation unit of the intrinsic calibration kernels (mcba_intrinsic_kernels.h): the homography kernel in the three
// register-array sizes of k_view_pose, the focal start, and k_calibrate_camera for every camera family
#include "mcba_intrinsic_kernels.h"

namespace mcba {
namespace intr {

hipError_t intrinsic_start_launch(const IntrinsicArgs& a, int n_views, int C, hipStream_t st) {
  if (n_views <= 0) return hipSuccess;
  const dim3 grid((n_views + pnp::VIEW_POSE_THREADS / 64 - 1) / (pnp::VIEW_POSE_THREADS / 64)), block(pnp::VIEW_POSE_THREADS);
  switch (pnp::view_pose_npl(a.P)) {
    case 2: hipLaunchKernelGGL(k_intrinsic_homography<2>, grid, block, 0, st, a, n_views); break;
    case 6: hipLaunchKernelGGL(k_intrinsic_homography<6>, grid, block, 0, st, a, n_views); break;
    case 16: hipLaunchKernelGGL(k_intrinsic_homography<16>, grid, block, 0, st, a, n_views); break;
    default: return hipErrorInvalidValue;   // (refused by the caller)
  }
  hipLaunchKernelGGL(k_intrinsic_focal, dim3(C), dim3(64), 0, st, a);
  return hipGetLastError();
}

template <int ND, bool FISH>
static hipError_t launch_family(const IntrinsicArgs& a, int n_cameras, hipStream_t st) {
  // 124.5 KiB of LDS for the one workgroup a camera gets: above the default limit of a launch
  const hipError_t e = hipFuncSetAttribute((const void*)k_calibrate_camera<ND, FISH>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)CAL_LDS_BYTES);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_calibrate_camera<ND, FISH>), dim3(n_cameras), dim3(CAL_THREADS), CAL_LDS_BYTES, st, a);
  return hipGetLastError();
}

hipError_t calibrate_camera_launch(const IntrinsicArgs& a, int nd, bool fisheye, int n_cameras, hipStream_t st) {
  if (n_cameras <= 0) return hipSuccess;
  if (fisheye) return launch_family<4, true>(a, n_cameras, st);
  switch (nd) {
    case 4: return launch_family<4, false>(a, n_cameras, st);
    case 5: return launch_family<5, false>(a, n_cameras, st);
    case 8: return launch_family<8, false>(a, n_cameras, st);
    case 12: return launch_family<12, false>(a, n_cameras, st);
    case 14: return launch_family<14, false>(a, n_cameras, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace intr
}  // namespace mcba
