// mcba_subpix.h -- sub-pixel refinement of detected corners in a grey image (FP64 throughout).
//
// Restates board.subpix_corners (board/common.py:50-54: cv2.cornerSubPix) for a batch of independent corners.  One iteration at the
// position c, half window (wx, wy), pixel centres at integer coordinates:
//   samples    S(i, j) = bilinear sample of the image at c + (j, i), |i| <= wy + 1, |j| <= wx + 1: ONE fractional offset for all of
//              them, indices clamped to the image (replicate border);
//   gradients  gx = S(i, j+1) - S(i, j-1), gy = S(i+1, j) - S(i-1, j) on the window |i| <= wy, |j| <= wx;
//   weight     m(i, j) = e^-(i/wy)^2 e^-(j/wx)^2, zero inside the zero zone |i| <= zy and |j| <= zx when one is given;
//   sums       a = sum m gx^2, b = sum m gx gy, d = sum m gy^2, p = sum m (gx^2 j + gx gy i), q = sum m (gx gy j + gy^2 i);
//   singular   det = a d - b^2, |det| <= DBL_EPSILON^2: stop and keep c;
//   step       c <- c + (d p - b q, a q - b p) / det.
// The iteration stops when c leaves [0, W) x [0, H), after max_iter iterations or when |step|^2 <= eps^2; a result further than the
// window from the start is given up for the start.  cv2 keeps the patch in float32 and returns float32: parity is at formula level.
//
// Everything is MCBA_HD like mcba_pnp.h: k_refine_corners (mcba_subpix_kernels.h) runs one corner per wavefront, tests/subpix_host
// builds the same source with g++.  refine_corner is a template over the PATCH that holds the samples of an iteration (LDS written
// by the 64 lanes on the device, an array on the host) and the REDUCER of the five sums (lane partials + xor butterfly, a plain
// loop, or the host's emulation of the butterfly's order).  The argument checks, the weights and the status codes at the end of the file serve the driver and the host build alike.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include "mcba_math.h"

// the sample and term functions are lambdas: inlined into the loops of the patch and the reducer
#define MCBA_SUBPIX_INLINE __attribute__((always_inline))
// refine_corner rounds every product and sum on its own, on the device too (the library is built with -ffp-contract=on): with the
// sums taken in the same order the g++ build then returns the bits of the device.  A window too small for its corner has no stable
// fixed point, and an iteration that wanders turns one different rounding into another result.
#if defined(__clang__)
#define MCBA_SUBPIX_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define MCBA_SUBPIX_NO_CONTRACT
#endif

namespace mcba {
namespace subpix {

// status byte of a corner (mcba.h: MCBA_SUBPIX_*)
constexpr int ST_OK = 0, ST_MAX_ITER = 1, ST_SINGULAR = 2, ST_LEFT_IMAGE = 3, ST_REVERTED = 4, ST_INVALID = 5;
constexpr int MAX_WINDOW = 15;                        // half window
constexpr int MAX_ITERATIONS = 100;
constexpr int MAX_WEIGHTS = 2 * MAX_WINDOW + 1;       // values of one weight vector
constexpr int MAX_SAMPLES = (2 * MAX_WINDOW + 3) * (2 * MAX_WINDOW + 3);
constexpr int MAX_IMAGE_SIDE = 1 << 15;
constexpr int DTYPE_U8 = 0, DTYPE_F32 = 1;            // mcba.h: MCBA_PIXEL_*

// what one call fixes for all of its corners
struct Window {
  int wx, wy;              // half window
  int zx, zy;              // zero zone, (-1, -1) = none (normalised by make_window)
  int max_iter;
  double eps;
  double msum;             // sum of the weights over the window
  const double* mx;        // [2 wx + 1] e^-(j/wx)^2
  const double* my;        // [2 wy + 1] e^-(i/wy)^2
};

MCBA_HD int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the position of corner `start` in image img [H][W]: out = x, y; *iters = evaluations of the sums; *quality = smaller eigenvalue of
// [[a, b], [b, d]] / msum at the last evaluation (NaN without one).  Returns the status.  Every lane of a wavefront calls it with
// the same arguments and, the reducer returning the same bits to all of them, leaves it with the same results.
template <class Pixel, class Patch, class Reducer>
MCBA_HD int refine_corner(const Pixel* img, int H, int W, const Window& w, double x0, double y0, Patch& patch, const Reducer& red,
                          double* out, int* iters, double* quality) {
  MCBA_SUBPIX_NO_CONTRACT
  out[0] = x0;
  out[1] = y0;
  *iters = 0;
  *quality = NAN;
  if (!(x0 >= 0.0 && x0 < (double)W && y0 >= 0.0 && y0 < (double)H)) return ST_INVALID;   // (NaN fails every comparison)
  const int cols = 2 * w.wx + 3, rows = 2 * w.wy + 3, wcols = 2 * w.wx + 1, wrows = 2 * w.wy + 1;
  const double eps2 = w.eps * w.eps;
  double cx = x0, cy = y0;
  int status = ST_MAX_ITER, it = 0;
  for (;;) {
    const double flx = floor(cx), fly = floor(cy);
    const double fx = cx - flx, fy = cy - fly;
    const int bx = (int)flx - (w.wx + 1), by = (int)fly - (w.wy + 1);      // sample (0, 0) of the patch
    patch.fill(rows * cols, [&](int k) MCBA_SUBPIX_INLINE {
      MCBA_SUBPIX_NO_CONTRACT
      const int r = k / cols, c = k - r * cols;
      const int xa = clampi(bx + c, W - 1), xb = clampi(bx + c + 1, W - 1);
      const Pixel* ra = img + (size_t)clampi(by + r, H - 1) * W;
      const Pixel* rb = img + (size_t)clampi(by + r + 1, H - 1) * W;
      const double top = (1.0 - fx) * (double)ra[xa] + fx * (double)ra[xb];
      const double bot = (1.0 - fx) * (double)rb[xa] + fx * (double)rb[xb];
      return (1.0 - fy) * top + fy * bot;
    });
    double s[5];
    red.template sum<5>(wrows * wcols, [&](int k, double* t) MCBA_SUBPIX_INLINE {
      MCBA_SUBPIX_NO_CONTRACT
      const int r = k / wcols, c = k - r * wcols;
      const int i = r - w.wy, j = c - w.wx;
      const int at = (r + 1) * cols + (c + 1);
      const double gx = patch[at + 1] - patch[at - 1], gy = patch[at + cols] - patch[at - cols];
      const bool zero = (i <= w.zy && -i <= w.zy) && (j <= w.zx && -j <= w.zx);
      const double m = zero ? 0.0 : w.my[r] * w.mx[c];
      t[0] = m * gx * gx;
      t[1] = m * gx * gy;
      t[2] = m * gy * gy;
      t[3] = t[0] * (double)j + t[1] * (double)i;
      t[4] = t[1] * (double)j + t[2] * (double)i;
    }, s);
    ++it;
    const double a = s[0], b = s[1], d = s[2], p = s[3], q = s[4];
    const double half_gap = 0.5 * sqrt((a - d) * (a - d) + 4.0 * b * b);
    *quality = fmax(0.5 * (a + d) - half_gap, 0.0) / w.msum;
    const double det = a * d - b * b;
    if (fabs(det) <= DBL_EPSILON * DBL_EPSILON) { status = ST_SINGULAR; break; }
    const double sx = (d * p - b * q) / det, sy = (a * q - b * p) / det;
    cx += sx;
    cy += sy;
    if (!(cx >= 0.0 && cx < (double)W && cy >= 0.0 && cy < (double)H)) { status = ST_LEFT_IMAGE; break; }
    if (sx * sx + sy * sy <= eps2) { status = ST_OK; break; }
    if (it >= w.max_iter) break;
  }
  *iters = it;
  if (!(fabs(cx - x0) <= (double)w.wx && fabs(cy - y0) <= (double)w.wy)) return ST_REVERTED;   // (out still holds the start)
  out[0] = cx;
  out[1] = cy;
  return status;
}

// ---------------------------------------------------------------------------------------------------------
// host side: patch and reducer of the g++ build, the weights of a call and the argument checks
// ---------------------------------------------------------------------------------------------------------
struct HostPatch {
  double s[MAX_SAMPLES];
  template <class F>
  void fill(int n, F sample) {
    for (int k = 0; k < n; ++k) s[k] = sample(k);
  }
  double operator[](int k) const { return s[k]; }
};

struct SerialReducer {       // window pixels in row order
  template <int K, class F>
  void sum(int n, F f, double* out) const {
    for (int k = 0; k < K; ++k) out[k] = 0.0;
    for (int i = 0; i < n; ++i) {
      double t[K];
      f(i, t);
      for (int k = 0; k < K; ++k) out[k] += t[k];
    }
  }
};

struct WaveOrderReducer {    // the order of the device: 64 lane partials (term i in lane i % 64), then the xor butterfly
  template <int K, class F>
  void sum(int n, F f, double* out) const {
    double b[64][K], c[64][K];
    for (int l = 0; l < 64; ++l)
      for (int k = 0; k < K; ++k) b[l][k] = 0.0;
    for (int i = 0; i < n; ++i) {
      double t[K];
      f(i, t);
      for (int k = 0; k < K; ++k) b[i & 63][k] += t[k];
    }
    for (int off = 32; off > 0; off >>= 1) {
      for (int l = 0; l < 64; ++l)
        for (int k = 0; k < K; ++k) c[l][k] = b[l][k] + b[l ^ off][k];
      for (int l = 0; l < 64; ++l)
        for (int k = 0; k < K; ++k) b[l][k] = c[l][k];
    }
    for (int k = 0; k < K; ++k) out[k] = b[0][k];
  }
};

// the two weight vectors (weights [2][MAX_WEIGHTS]: mx | my), their sum over the window and the zero zone that applies: computed
// once per call on the host, so that the device and the g++ build work with the same bits
inline Window make_window(int wx, int wy, int zx, int zy, int max_iter, double eps, double* weights) {
  Window w{};
  w.wx = wx; w.wy = wy; w.max_iter = max_iter; w.eps = eps;
  const bool zone = zx >= 0 && zy >= 0 && 2 * zx + 1 < 2 * wx + 1 && 2 * zy + 1 < 2 * wy + 1;
  w.zx = zone ? zx : -1;
  w.zy = zone ? zy : -1;
  double* mx = weights;
  double* my = weights + MAX_WEIGHTS;
  for (int j = -wx; j <= wx; ++j) mx[j + wx] = exp(-((double)j / wx) * ((double)j / wx));
  for (int i = -wy; i <= wy; ++i) my[i + wy] = exp(-((double)i / wy) * ((double)i / wy));
  w.msum = 0.0;
  for (int i = -wy; i <= wy; ++i)
    for (int j = -wx; j <= wx; ++j)
      if (!(abs(i) <= w.zy && abs(j) <= w.zx)) w.msum += my[i + wy] * mx[j + wx];
  w.mx = mx;
  w.my = my;
  return w;
}

// everything mcba_refine_corners refuses before it looks at a corner; *nothing: a call with no corners, which returns at once
inline bool check_refine(int N, int H, int W, int dtype, int n, const void* images, const double* corners, const int32_t* image_of,
                         int wx, int wy, int max_iter, double eps, const double* refined, const uint8_t* status, const char* who,
                         bool* nothing, std::string& err) {
  const std::string s(who);
  char msg[200];
  *nothing = false;
  if (n < 0 || N < 0) { err = s + ": negative size"; return false; }
  if (wx < 1 || wx > MAX_WINDOW || wy < 1 || wy > MAX_WINDOW) {
    snprintf(msg, sizeof msg, "%s: the half window must be 1 .. %d on both axes, not (%d, %d)", who, MAX_WINDOW, wx, wy);
    err = msg;
    return false;
  }
  if (max_iter < 1 || max_iter > MAX_ITERATIONS) {
    snprintf(msg, sizeof msg, "%s: max_iter must be 1 .. %d, not %d", who, MAX_ITERATIONS, max_iter);
    err = msg;
    return false;
  }
  if (!(eps >= 0.0 && eps < 1e300)) { err = s + ": eps must be finite and not negative"; return false; }
  if (dtype != DTYPE_U8 && dtype != DTYPE_F32) {
    err = s + ": unsupported pixel type " + std::to_string(dtype) + " (uint8, float32)";
    return false;
  }
  if (n == 0) { *nothing = true; return true; }
  if (N == 0) { err = s + ": corners but no image"; return false; }
  if (H < 2 || W < 2 || H > MAX_IMAGE_SIDE || W > MAX_IMAGE_SIDE) {
    snprintf(msg, sizeof msg, "%s: image sizes must be 2 .. %d a side, not %d x %d", who, MAX_IMAGE_SIDE, H, W);
    err = msg;
    return false;
  }
  if (!images || !corners || !refined || !status) { err = s + ": null argument"; return false; }
  if (image_of)
    for (int i = 0; i < n; ++i)
      if (image_of[i] < 0 || image_of[i] >= N) {
        snprintf(msg, sizeof msg, "%s: corner %d names image %d of %d", who, i, (int)image_of[i], N);
        err = msg;
        return false;
      }
  return true;
}

}  // namespace subpix
}  // namespace mcba
