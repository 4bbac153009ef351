// mcba_subpix_kernels.h -- k_refine_corners: the corner refinement of mcba_subpix.h, one wavefront per corner.
//
//   * four corners per 256-thread workgroup, grid-stride over rounds of 4 x grid corners; the waves of a workgroup are independent
//     (they run different iteration counts): after the wave's entry there is no __syncthreads() or any other cross-wave wait, no
//     atomic and nothing between workgroups.  Every loop is bounded by max_iter <= 100 or by the corner count;
//   * per iteration the wave writes the (2 wy + 3) x (2 wx + 3) bilinear samples into a patch of its own in LDS, lanes striding over
//     the samples, four taps each straight from the image (the two fractions and the clamped base are wave-uniform); a wave_fence();
//     then the lanes stride over the window pixels and form the five per-lane partial sums, folded by the xor butterfly: every lane
//     ends with the same bits, so the 2 x 2 solve, the stop rule and all control flow are uniform without a broadcast and the same
//     call returns the same bytes every time;
//   * the weights come from the host (no exp on the device), and no product is contracted into an FMA: the g++ build that sums in
//     this order (WaveOrderReducer) returns the bits of the device;
//   * SAMPLES = doubles of one wave's patch: SMALL_SAMPLES serves every window of up to 17 x 17 samples (half windows up to (7, 7), and
//     flat ones such as (15, 1)) in 9.2 KB of LDS a workgroup, MAX_SAMPLES (33 x 33, 34.8 KB a workgroup) the rest.
#pragma once
#include <hip/hip_runtime.h>
#include "mcba_pnp_kernels.h"
#include "mcba_subpix.h"

namespace mcba {
namespace subpix {

struct RefineArgs {
  const void* images;         // [N][H][W] uint8 or float32
  int H, W;
  int n;
  const double* corners;      // [n][2]
  const int32_t* image_of;    // [n] or null = image 0
  Window w;                   // (mx, my: device pointers)
  double* refined;            // [n][2]
  uint8_t* status;            // [n]
  int32_t* iters;             // [n] or null
  double* quality;            // [n] or null
};

constexpr int SUBPIX_THREADS = 256;                  // four corners per workgroup
constexpr int SUBPIX_WAVES = SUBPIX_THREADS / 64;
constexpr int SUBPIX_MAX_GRID = 2048;                // grid cap (256 CUs x 8 workgroups): beyond it the waves stride
constexpr int SMALL_SAMPLES = 17 * 17;

// the patch of one wave in LDS: sample k is written by lane k % 64
struct LdsPatch {
  double* s;
  int lane;
  template <class F>
  __device__ __forceinline__ void fill(int n, F sample) {
    pnp::wave_fence();        // (the reads of the iteration before are complete)
    for (int k = lane; k < n; k += 64) s[k] = sample(k);
    pnp::wave_fence();
  }
  __device__ __forceinline__ double operator[](int k) const { return s[k]; }
};

// terms k, k + 64, ... in lane k % 64, then the xor butterfly
struct WaveReducer {
  int lane;
  template <int K, class F>
  __device__ __forceinline__ void sum(int n, F f, double* out) const {
    MCBA_SUBPIX_NO_CONTRACT
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (int i = lane; i < n; i += 64) {
      double t[K];
      f(i, t);
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] += t[k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = pnp::wave_xor_sum(acc[k]);
  }
};

template <class Pixel, int SAMPLES>
__global__ __launch_bounds__(SUBPIX_THREADS) void k_refine_corners(RefineArgs a) {
  __shared__ double s_patch[SUBPIX_WAVES][SAMPLES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  LdsPatch patch{s_patch[wave], lane};
  const WaveReducer red{lane};
  const Pixel* images = static_cast<const Pixel*>(a.images);
  const long long stride = (long long)gridDim.x * SUBPIX_WAVES;
  for (long long k = (long long)blockIdx.x * SUBPIX_WAVES + wave; k < a.n; k += stride) {   // (wave-uniform: whole waves leave)
    const int image = a.image_of ? a.image_of[k] : 0;
    double out[2], quality;
    int iters;
    const int status = refine_corner(images + (size_t)image * a.H * a.W, a.H, a.W, a.w, a.corners[2 * k], a.corners[2 * k + 1], patch,
                                     red, out, &iters, &quality);
    if (lane == 0) {
      reinterpret_cast<double2*>(a.refined)[k] = make_double2(out[0], out[1]);
      a.status[k] = (uint8_t)status;
      if (a.iters) a.iters[k] = iters;
      if (a.quality) a.quality[k] = quality;
    }
  }
}

// false: no instantiation for this pixel type
bool refine_corners_launch(const RefineArgs& a, int dtype, hipStream_t st);   // mcba_subpix.hip

}  // namespace subpix
}  // namespace mcba
