// translation unit of k_point_ops, k_undistort_map and k_remap_cubic (mcba_undistort_kernels.h)
#include "mcba_undistort_kernels.h"

namespace mcba {
namespace undistort {

namespace {
int grid_for(long long work_items, long long per_block) {
  const long long blocks = (work_items + per_block - 1) / per_block;
  return (int)(blocks < 1 ? 1 : blocks > (1 << 20) ? (1 << 20) : blocks);
}

template <int CH, class T, bool FUSED>
void launch_remap(const RemapArgs& a, hipStream_t st) {
  long long blocks;
  if (a.flat) {
    blocks = ((long long)a.N * a.Hd * a.Wd + 3) / 4;
    blocks = (blocks + UNDISTORT_THREADS - 1) / UNDISTORT_THREADS;
  } else {
    blocks = (long long)(FUSED ? a.C : a.N) * ((a.Hd + TILE_H - 1) / TILE_H) * ((a.Wd + TILE_W - 1) / TILE_W);
  }
  if (a.flat) hipLaunchKernelGGL((k_remap_cubic<CH, T, FUSED, true>), dim3(grid_for(blocks, 1)), dim3(UNDISTORT_THREADS), 0, st, a);
  else hipLaunchKernelGGL((k_remap_cubic<CH, T, FUSED, false>), dim3(grid_for(blocks, 1)), dim3(UNDISTORT_THREADS), 0, st, a);
}

template <bool FUSED>
bool launch_remap_format(const RemapArgs& a, int channels, int dtype, hipStream_t st) {
  if (channels == 1 && dtype == PIXEL_U8) launch_remap<1, uint8_t, FUSED>(a, st);
  else if (channels == 3 && dtype == PIXEL_U8) launch_remap<3, uint8_t, FUSED>(a, st);
  else if (channels == 1 && dtype == PIXEL_F32) launch_remap<1, float, FUSED>(a, st);
  else if (channels == 3 && dtype == PIXEL_F32) launch_remap<3, float, FUSED>(a, st);
  else return false;
  return true;
}
}  // namespace

void point_ops_launch(const PointOpsArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_point_ops, dim3(grid_for(a.n, UNDISTORT_THREADS)), dim3(UNDISTORT_THREADS), 0, st, a);
}

void undistort_map_launch(const MapArgs& a, hipStream_t st) {
  const long long total = (long long)a.C * a.H * a.W;
  if (total <= 0) return;
  hipLaunchKernelGGL(k_undistort_map, dim3(grid_for(total, UNDISTORT_THREADS)), dim3(UNDISTORT_THREADS), 0, st, a);
}

bool remap_launch(const RemapArgs& a, int channels, int dtype, bool fused, hipStream_t st) {
  if ((long long)a.N * a.Hd * a.Wd <= 0) return true;
  return fused ? launch_remap_format<true>(a, channels, dtype, st) : launch_remap_format<false>(a, channels, dtype, st);
}

}  // namespace undistort
}  // namespace mcba
