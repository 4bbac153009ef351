// translation unit of k_hand_eye (mcba_handeye_kernels.h)
#include "mcba_handeye_kernels.h"

namespace mcba {
namespace handeye {

void hand_eye_launch(const HandEyeArgs& a, hipStream_t st) {
  if (a.n_problems <= 0) return;
  const dim3 grid(a.n_problems), block(64);
  hipLaunchKernelGGL(k_hand_eye, grid, block, 0, st, a);
}

}  // namespace handeye
}  // namespace mcba
