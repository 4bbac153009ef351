// mcba_residual_field.h -- the mathematics of the residual field (mcba_residual_gram), shared by the kernels
// (mcba_residual_field_kernels.h) and the g++ build the tests compare them with (tests/residual_field).
//
// Per camera a tensor-product UNIFORM CUBIC B-SPLINE field e(u, v) in R^2 over the image [0, W] x [0, H]: nx x ny intervals,
// K = (nx + 3)(ny + 3) control points, control point (a, b) (a along y, b along x) in column a (nx + 3) + b; both components share
// the grid.  A pixel in interval (ix, iy) with fractions (tx, ty) has the 16 non-zero weights wy[a] wx[b], a, b = 0 .. 3, on the
// control points (iy + a, ix + b); they are non-negative and sum to 1.  The row of an observation is
//     [ b(u, v)  (K entries) | r_x | r_y ],   r = projected - observed,   NC = K + 2 <= 64 columns,
// and what is accumulated per (camera, fold = frame mod n_folds) is the Gram matrix of these rows: B^T B, B^T r_x, B^T r_y,
// r_x^T r_x, r_x^T r_y, r_y^T r_y in one symmetric NC x NC block.
//
// Host and device evaluate a weight with the SAME roundings: every multiply-add below is an explicit fma, every other statement
// holds a single kind of operation, so neither -ffp-contract=on nor =off changes a bit.
#pragma once
#include <stdint.h>
#include "mcba_math.h"

#include <stddef.h>

namespace mcba {
namespace resfield {

constexpr int MAX_NC = 64;          // columns of a row: four 16-column MFMA tiles
constexpr int MAX_FOLDS = 16;
constexpr int MAX_COV_BINS = 512;   // cov_w * cov_h of the coverage maps (two planes of LDS counters per workgroup)

MCBA_HD int n_control(int nx, int ny) { return (nx + 3) * (ny + 3); }

struct Cell {
  int i;       // interval, 0 .. n - 1
  double t;    // fraction inside it, 0 .. 1 (1 only for a pixel exactly on the far edge)
};

// interval and fraction of coordinate u of an image of extent W cut into n intervals; 0 <= u <= W is the caller's business
MCBA_HD Cell spline_cell(double u, double W, int n) {
  const double un = u * (double)n;
  const double s = un / W;
  int i = (int)s;
  if (i > n - 1) i = n - 1;
  if (i < 0) i = 0;
  Cell c;
  c.i = i;
  c.t = s - (double)i;
  return c;
}

// the four cubic B-spline weights of fraction t on the control points i .. i + 3
MCBA_HD void cubic_weights(double t, double w[4]) {
  const double m = 1.0 - t;
  const double mm = m * m;
  const double tt = t * t;
  const double m3 = mm * m;
  const double t3 = tt * t;
  const double p1 = fma(fma(3.0, t, -6.0), tt, 4.0);                  // 3 t^3 - 6 t^2 + 4
  const double p2 = fma(fma(fma(-3.0, t, 3.0), t, 3.0), t, 1.0);      // -3 t^3 + 3 t^2 + 3 t + 1
  w[0] = m3 / 6.0;
  w[1] = p1 / 6.0;
  w[2] = p2 / 6.0;
  w[3] = t3 / 6.0;
}

// a slot whose observed pixel is not inside the closed image rectangle does not enter (NaN: not inside)
MCBA_HD bool inside_image(double u, double v, double W, double H) { return u >= 0.0 && u <= W && v >= 0.0 && v <= H; }

// coverage cell of coordinate u: n cells over [0, W], the far edge in the last one
MCBA_HD int coverage_bin(double u, double W, int n) {
  const double un = u * (double)n;
  int i = (int)(un / W);
  if (i > n - 1) i = n - 1;
  if (i < 0) i = 0;
  return i;
}

// the 16 non-zero entries of b(u, v): column col[4 a + b] carries w[4 a + b] = wy[a] wx[b]
MCBA_HD void field_row(double u, double v, double W, double H, int nx, int ny, int col[16], double w[16]) {
  const Cell cx = spline_cell(u, W, nx), cy = spline_cell(v, H, ny);
  double wx[4], wy[4];
  cubic_weights(cx.t, wx);
  cubic_weights(cy.t, wy);
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 4; ++b) {
      col[4 * a + b] = (cy.i + a) * (nx + 3) + cx.i + b;
      w[4 * a + b] = wy[a] * wx[b];
    }
}

#if !defined(__HIPCC__)
// The specification of mcba_residual_gram as one sequential loop over [C,F,B,P] arrays in the reference's order: projected and
// observed [C,F,B,P,2], valid and inlier [C,F,B,P], image_size [C][2] (W, H).  gram [C][n_folds][NC][NC] (full symmetric), count
// [C][n_folds], outside [C], coverage [C][2][cov_h][cov_w] or null -- and absgram (or null), the Gram matrix of the ABSOLUTE rows
// A = sum |row_i| |row_j|: the scale of the rounding error of any summation order of the same products.
inline void host_residual_gram(int C, int F, int B, int P, const double* projected, const double* observed, const uint8_t* valid,
                               const uint8_t* inlier, const int32_t* image_size, int nx, int ny, int n_folds, int inliers_only,
                               double* gram, double* absgram, int64_t* count, int64_t* outside, int cov_w, int cov_h,
                               int32_t* coverage) {
  const int K = n_control(nx, ny), NC = K + 2;
  const size_t blk = (size_t)NC * NC;
  for (size_t i = 0; i < (size_t)C * n_folds * blk; ++i) {
    gram[i] = 0.0;
    if (absgram) absgram[i] = 0.0;
  }
  for (int i = 0; i < C * n_folds; ++i) count[i] = 0;
  for (int c = 0; c < C; ++c) outside[c] = 0;
  if (coverage)
    for (size_t i = 0; i < (size_t)C * 2 * cov_w * cov_h; ++i) coverage[i] = 0;
  int col[16 + 2];
  double w[16 + 2];
  for (int c = 0; c < C; ++c) {
    const double W = (double)image_size[2 * c], H = (double)image_size[2 * c + 1];
    for (int f = 0; f < F; ++f) {
      const int fold = f % n_folds;
      double* G = gram + ((size_t)c * n_folds + fold) * blk;
      double* A = absgram ? absgram + ((size_t)c * n_folds + fold) * blk : nullptr;
      for (int q = 0; q < B * P; ++q) {
        const size_t s = ((size_t)c * F + f) * B * P + q;
        if (!valid[s]) continue;
        const bool in = inlier[s] != 0;
        const double u = observed[2 * s], v = observed[2 * s + 1];
        const bool ins = inside_image(u, v, W, H);
        if (ins && coverage)
          coverage[(((size_t)c * 2 + (in ? 0 : 1)) * cov_h + coverage_bin(v, H, cov_h)) * cov_w + coverage_bin(u, W, cov_w)] += 1;
        if (inliers_only && !in) continue;
        if (!ins) {
          outside[c] += 1;
          continue;
        }
        field_row(u, v, W, H, nx, ny, col, w);
        col[16] = K;
        col[17] = K + 1;
        w[16] = projected[2 * s] - u;
        w[17] = projected[2 * s + 1] - v;
        for (int i = 0; i < 18; ++i)
          for (int j = 0; j < 18; ++j) {
            const double p = w[i] * w[j];
            G[(size_t)col[i] * NC + col[j]] += p;
            if (A) A[(size_t)col[i] * NC + col[j]] += fabs(p);
          }
        count[c * n_folds + fold] += 1;
      }
    }
  }
}
#endif

}  // namespace resfield
}  // namespace mcba
