// translation unit of k_view_pose (mcba_pnp_kernels.h): the three register-array sizes, camera family switched at run time
#include "mcba_pnp_kernels.h"

namespace mcba {
namespace pnp {

void view_pose_launch(const ViewPoseArgs& a, hipStream_t st) {
  if (a.n_active <= 0) return;
  const dim3 grid((a.n_active + VIEW_POSE_THREADS / 64 - 1) / (VIEW_POSE_THREADS / 64)), block(VIEW_POSE_THREADS);
  switch (view_pose_npl(a.P)) {
    case 2: hipLaunchKernelGGL(k_view_pose<2>, grid, block, 0, st, a); break;
    case 6: hipLaunchKernelGGL(k_view_pose<6>, grid, block, 0, st, a); break;
    case 16: hipLaunchKernelGGL(k_view_pose<16>, grid, block, 0, st, a); break;
    default: break;   // (refused by the caller)
  }
}

}  // namespace pnp
}  // namespace mcba
