// TEST INFRASTRUCTURE: g++ build of the corner refinement (multical_amd/csrc/mcba_subpix.h) behind the signature of
// mcba_refine_corners: one plain loop over the corners, the patch an array and the five sums in row order (sph_refine_corners) or in
// the order of the device's lanes and butterfly (sph_refine_corners_wave_order).  The argument checks and the weights are the
// functions the driver of the API calls.
#include <string>

#include "../../include/mcba.h"
#include "../../multical_amd/csrc/mcba_subpix.h"

using namespace mcba::subpix;

static thread_local std::string g_error;

template <class Reducer, class Pixel>
static void host_refine(const Pixel* images, int H, int W, int n, const double* corners, const int32_t* image_of, const Window& w,
                        double* refined, uint8_t* status, int32_t* iterations, double* quality) {
  HostPatch patch;
  const Reducer red;
  for (int k = 0; k < n; ++k) {
    const int image = image_of ? image_of[k] : 0;
    int iters;
    double q;
    status[k] = (uint8_t)refine_corner(images + (size_t)image * H * W, H, W, w, corners[2 * k], corners[2 * k + 1], patch, red,
                                       refined + 2 * k, &iters, &q);
    if (iterations) iterations[k] = iters;
    if (quality) quality[k] = q;
  }
}

template <class Reducer>
static int32_t refine(const void* images, int32_t N, int32_t H, int32_t W, int32_t dtype, int32_t n, const double* corners,
                      const int32_t* image_of_corner, int32_t win_x, int32_t win_y, int32_t zero_x, int32_t zero_y, int32_t max_iter,
                      double eps, double* refined, uint8_t* status, int32_t* iterations, double* quality) {
  bool nothing = false;
  if (!check_refine(N, H, W, dtype, n, images, corners, image_of_corner, win_x, win_y, max_iter, eps, refined, status,
                    "mcba_refine_corners", &nothing, g_error))
    return 1;
  if (nothing) return 0;
  double weights[2 * MAX_WEIGHTS];
  const Window w = make_window(win_x, win_y, zero_x, zero_y, max_iter, eps, weights);
  if (dtype == DTYPE_U8)
    host_refine<Reducer>((const uint8_t*)images, H, W, n, corners, image_of_corner, w, refined, status, iterations, quality);
  else
    host_refine<Reducer>((const float*)images, H, W, n, corners, image_of_corner, w, refined, status, iterations, quality);
  return 0;
}

extern "C" {

const char* sph_last_error(void) { return g_error.c_str(); }

int32_t sph_refine_corners(const void* images, int32_t N, int32_t H, int32_t W, int32_t dtype, int32_t n, const double* corners,
                           const int32_t* image_of_corner, int32_t win_x, int32_t win_y, int32_t zero_x, int32_t zero_y,
                           int32_t max_iter, double eps, double* refined, uint8_t* status, int32_t* iterations, double* quality) {
  return refine<SerialReducer>(images, N, H, W, dtype, n, corners, image_of_corner, win_x, win_y, zero_x, zero_y, max_iter, eps, refined,
                               status, iterations, quality);
}

int32_t sph_refine_corners_wave_order(const void* images, int32_t N, int32_t H, int32_t W, int32_t dtype, int32_t n,
                                      const double* corners, const int32_t* image_of_corner, int32_t win_x, int32_t win_y,
                                      int32_t zero_x, int32_t zero_y, int32_t max_iter, double eps, double* refined, uint8_t* status,
                                      int32_t* iterations, double* quality) {
  return refine<WaveOrderReducer>(images, N, H, W, dtype, n, corners, image_of_corner, win_x, win_y, zero_x, zero_y, max_iter, eps,
                                  refined, status, iterations, quality);
}

}
