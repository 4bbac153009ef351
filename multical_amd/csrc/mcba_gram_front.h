// mcba_gram_front.h -- the front end that k_view_schur (mcba_guidance_kernels.h) and k_rig_gram (mcba_rigview_kernels.h) share: the
// rows of a view's points staged in LDS and their Gram matrix accumulated by f64 MFMA.  The head of mcba_guidance_kernels.h states
// the layout.
#pragma once
#include <hip/hip_runtime.h>
#include "mcba_guidance.h"
#include "mcba_pnp_kernels.h"

namespace mcba {
namespace guidance {

constexpr int SCHUR_THREADS = 128, SCHUR_WAVES = SCHUR_THREADS / 64;
constexpr int LDV = 25, STAGE = 128 * LDV + 8;
static_assert(GS * GS <= STAGE, "a wave's Gram tiles reuse its staging buffer");

// The front end of a view's Gram matrix, one wave's share (k_view_schur and k_rig_gram): the wave takes the n points in chunks of 64,
// round-robin over SCHUR_WAVES waves; rows(i, row_u, row_v) writes the two rows of point i (`cols` entries, zero where it is not
// visible) into the wave's staging buffer V and says whether it is visible; the upper tiles 00, 01, 11 are accumulated as the head of
// this file states and end in V: entry (i, j), i <= j, at V[i GS + j].  Returns the wave's visible count.
template <class Rows>
__device__ __forceinline__ int wave_gram_tiles(double* V, int n, int cols, int wave, int lane, const Rows& rows) {
  const int rsub = lane >> 4, csub = lane & 15;
  pnp::wave_double4 acc00 = {0.0, 0.0, 0.0, 0.0}, acc01 = acc00, acc11 = acc00;
  int count = 0;
  for (int base = wave * 64; base < n; base += SCHUR_THREADS) {          // (uniform over the wave)
    const int i = base + lane;
    double* row_u = V + (2 * lane) * LDV;
    double* row_v = row_u + LDV;
    bool visible = false;
    if (i < n) {
      visible = rows(i, row_u, row_v);
    } else {
      for (int j = 0; j < cols; ++j) row_u[j] = row_v[j] = 0.0;
    }
    count += __popcll(__ballot(visible));
    pnp::wave_fence();
    const int nrows = 2 * min(64, n - base), nsteps = (nrows + 3) >> 2;
    const double* vp = V + rsub * LDV + csub;
    for (int st = 0; st < nsteps; ++st) {
      const double a0 = vp[(4 * st) * LDV];
      acc00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, a0, acc00, 0, 0, 0);
      if (cols > 16) {
        const double a1 = vp[(4 * st) * LDV + 16];
        acc01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, a1, acc01, 0, 0, 0);
        acc11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, a1, acc11, 0, 0, 0);
      }
    }
    pnp::wave_fence();
  }
  // the wave's tiles take the place of its staged rows
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    V[(rsub + 4 * q) * GS + csub] = acc00[q];
    V[(rsub + 4 * q) * GS + 16 + csub] = acc01[q];
    V[(16 + rsub + 4 * q) * GS + 16 + csub] = acc11[q];
  }
  return count;
}

}  // namespace guidance
}  // namespace mcba
