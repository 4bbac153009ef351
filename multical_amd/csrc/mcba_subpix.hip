// translation unit of k_refine_corners (mcba_subpix_kernels.h) and the host driver of mcba_refine_corners
#include "mcba_debug.h"
#include "mcba_host.h"
#include "mcba_subpix_kernels.h"

namespace mcba {
namespace subpix {

template <class Pixel>
static void launch_refine(const RefineArgs& a, hipStream_t st) {
  const int grid = host::capped_grid(((long long)a.n + SUBPIX_WAVES - 1) / SUBPIX_WAVES, SUBPIX_MAX_GRID);
  if ((2 * a.w.wx + 3) * (2 * a.w.wy + 3) <= SMALL_SAMPLES)
    hipLaunchKernelGGL((k_refine_corners<Pixel, SMALL_SAMPLES>), dim3(grid), dim3(SUBPIX_THREADS), 0, st, a);
  else
    hipLaunchKernelGGL((k_refine_corners<Pixel, MAX_SAMPLES>), dim3(grid), dim3(SUBPIX_THREADS), 0, st, a);
}

bool refine_corners_launch(const RefineArgs& a, int dtype, hipStream_t st) {
  if (dtype == DTYPE_U8) launch_refine<uint8_t>(a, st);
  else if (dtype == DTYPE_F32) launch_refine<float>(a, st);
  else return false;
  return true;
}

}  // namespace subpix
}  // namespace mcba

using namespace mcba;
using namespace mcba::host;

// uploads | event-timed kernel | downloads | whole call; corners refined
MCBA_TIMING_GETTER(mcba_debug_subpix_ms, g_subpix_timing, 4)

extern "C" {

namespace {
void refine_corners(const void* images, int32_t N, int32_t H, int32_t W, int32_t dtype, int32_t n, const double* corners,
                    const int32_t* image_of, int32_t win_x, int32_t win_y, int32_t zero_x, int32_t zero_y, int32_t max_iter, double eps,
                    double* refined, uint8_t* status, int32_t* iterations, double* quality) {
  const char* who = "mcba_refine_corners";
  DeviceCall call(g_subpix_timing);   // (before the buffers: see host::DeviceCall)
  call.tm.reset();
  std::string err;
  bool nothing = false;
  if (!subpix::check_refine(N, H, W, dtype, n, images, corners, image_of, win_x, win_y, max_iter, eps, refined, status, who, &nothing,
                            err))
    throw Error(err);
  if (nothing) return;                   // nothing is launched, the device is not touched
  std::vector<double> weights(2 * subpix::MAX_WEIGHTS, 0.0);
  subpix::RefineArgs a{};
  a.w = subpix::make_window(win_x, win_y, zero_x, zero_y, max_iter, eps, weights.data());
  const size_t count = (size_t)n, image_bytes = (size_t)N * H * W * (dtype == subpix::DTYPE_U8 ? 1 : 4);
  DevBuf<uint8_t> d_images;
  DevBuf<double> d_corners, d_weights, d_refined;
  DevBuf<int32_t> d_of;
  call.open(2);
  upload_async(d_images, (const uint8_t*)images, image_bytes, call.st);
  upload_async(d_corners, corners, count * 2, call.st);
  upload_vector(d_weights, weights, call.st);
  if (image_of) upload_async(d_of, image_of, count, call.st);
  d_refined.alloc(count * 2, false);
  OutBuf<uint8_t> o_status(status, count);
  OutBuf<int32_t> o_iters(iterations, count);
  OutBuf<double> o_quality(quality, count);
  a.images = d_images.p;
  a.H = H; a.W = W; a.n = n;
  a.corners = d_corners.p;
  a.image_of = image_of ? d_of.p : nullptr;
  a.w.mx = d_weights.p;
  a.w.my = d_weights.p + subpix::MAX_WEIGHTS;
  a.refined = d_refined.p; a.status = o_status.dev(); a.iters = o_iters.dev(); a.quality = o_quality.dev();
  call.mark(0);
  REQUIRE(subpix::refine_corners_launch(a, dtype, call.st), std::string(who) + ": no kernel for this pixel type");
  call.mark(1);
  call.end_kernels("k_refine_corners");
  download_async(refined, d_refined.p, count * 2, call.st);
  o_status.fetch(call.st);
  o_iters.fetch(call.st);
  o_quality.fetch(call.st);
  call.finish(n);
}
}  // namespace

int32_t mcba_refine_corners(const void* images, int32_t N, int32_t H, int32_t W, int32_t dtype, int32_t n, const double* corners,
                            const int32_t* image_of_corner, int32_t win_x, int32_t win_y, int32_t zero_x, int32_t zero_y,
                            int32_t max_iter, double eps, double* refined, uint8_t* status, int32_t* iterations, double* quality) {
  API_BEGIN
  refine_corners(images, N, H, W, dtype, n, corners, image_of_corner, win_x, win_y, zero_x, zero_y, max_iter, eps, refined, status,
                 iterations, quality);
  API_END
}

}  // extern "C"
