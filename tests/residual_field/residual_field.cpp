// TEST INFRASTRUCTURE: g++ build of the residual-field mathematics (multical_amd/csrc/mcba_residual_field.h): the spline cell, the
// cubic weights, the row of a pixel, and host_residual_gram -- the sequential specification of mcba_residual_gram over [C,F,B,P]
// arrays in the reference's order, which also returns the absolute-value Gram the tests scale their bound with.
#include <string>

#include "../../multical_amd/csrc/mcba_residual_field.h"

using namespace mcba::resfield;

static thread_local std::string g_error;

extern "C" {

const char* rfh_last_error() { return g_error.c_str(); }

int32_t rfh_cell(double u, double W, int32_t n, int32_t* interval, double* fraction) {
  const Cell c = spline_cell(u, W, n);
  *interval = c.i;
  *fraction = c.t;
  return 0;
}

int32_t rfh_weights(int64_t n, const double* t, double* w /*[n][4]*/) {
  for (int64_t i = 0; i < n; ++i) cubic_weights(t[i], w + 4 * i);
  return 0;
}

// rows of n pixels of one image: col [n][16], w [n][16], inside [n]
int32_t rfh_rows(int64_t n, const double* pixels, double W, double H, int32_t nx, int32_t ny, int32_t* col, double* w, uint8_t* inside) {
  for (int64_t i = 0; i < n; ++i) {
    const double u = pixels[2 * i], v = pixels[2 * i + 1];
    inside[i] = inside_image(u, v, W, H) ? 1 : 0;
    for (int k = 0; k < 16; ++k) {
      col[16 * i + k] = 0;
      w[16 * i + k] = 0.0;
    }
    if (inside[i]) field_row(u, v, W, H, nx, ny, col + 16 * i, w + 16 * i);
  }
  return 0;
}

int32_t rfh_residual_gram(int32_t C, int32_t F, int32_t B, int32_t P, const double* projected, const double* observed,
                          const uint8_t* valid, const uint8_t* inlier, const int32_t* image_size, int32_t nx, int32_t ny,
                          int32_t n_folds, int32_t inliers_only, double* gram, double* absgram, int64_t* count, int64_t* outside,
                          int32_t cov_w, int32_t cov_h, int32_t* coverage) {
  if (nx < 1 || ny < 1 || n_folds < 1 || n_folds > MAX_FOLDS || n_control(nx, ny) + 2 > MAX_NC) {
    g_error = "residual field: bad grid or fold count";
    return 1;
  }
  for (int c = 0; c < C; ++c)
    if (image_size[2 * c] <= 0 || image_size[2 * c + 1] <= 0) {
      g_error = "residual field: the image size of camera " + std::to_string(c) + " is not positive";
      return 1;
    }
  host_residual_gram(C, F, B, P, projected, observed, valid, inlier, image_size, nx, ny, n_folds, inliers_only, gram, absgram, count,
                     outside, cov_w, cov_h, coverage);
  return 0;
}

}  // extern "C"
