// mcba_guidance.h -- where to hold the board next: the information a candidate view adds to a camera's intrinsics, and what it does
// to the projection uncertainty over a focus region.
//
// A VIEW is a set of points seen by one camera c, with n_nuisance free parameters of its own:
//   board view   the P points of a board at the board-in-camera pose T (3 x 4); visible: in front, inside the image by `margin`
//                pixels, det d(u, v) / d(x, y) > 0 where the point lands (the test of mcba_uncertainty.h);
//   focus view   the unit rays n_c(q) of a grid or a list of pixels at inverse distance rho; visible: the exact inverse converges
//                and the same determinant test.
// The scaled point Y (Y = X for a board, rho = 1; Y = n for a focus) is carried as in mcba_uncertainty.h.  The two rows of a visible
// point, r + n_nuisance columns:
//   [0, r)             Kc_c W_c                            (W_c [KI, r]: M_c F of section 3.14, from the host)
//   [r, r + 3)         A (e_k x (Y - c))                   left rotation of the view's own pose about c: the camera (c = 0) with
//                                                          n_nuisance = 3; with 6 the centre of the view (the board's centroid,
//                                                          the optical axis of a focus) -- the same span with the translations,
//                                                          and a nuisance block whose pivots tell a degenerate view apart
//   [r + 3, r + 6)     rho A e_k                           its translation (n_nuisance = 6 only)
// An invisible point has zero rows.  G = Z^T Z (upper triangle, row stride GS) is summed over the points and
//   S = G_kk - G_ke G_ee^-1 G_ek
// is the Schur complement of the nuisance block: Cholesky of G_ee (a pivot at or below PD_EPS times its diagonal entry: DEGENERATE),
// Y = L^-1 G_ek, S = G_kk - Y^T Y.  Scoring against a base B (SPD): M = B + S / sigma^2 = L L^T,
//   gain = sum log L_ii - sum log (L_B)_ii,   focus_rms = sqrt(trace(L^-1 Q L^-T) / n_focus).
// MCBA_HD like mcba_uncertainty.h: k_view_schur / k_view_score (mcba_guidance_kernels.h) and tests/guidance compile this source.
#pragma once
#include <stdint.h>
#include "mcba_uncertainty.h"

namespace mcba {
namespace guidance {

using uncertainty::KI;
constexpr int ST_OK = 0, ST_TOO_FEW = 1, ST_DEGENERATE = 2, ST_UNCONSTRAINED = 3;   // mcba.h: MCBA_GUIDE_*
constexpr int CRIT_FOCUS = 0, CRIT_GAIN = 1;                                        // mcba.h: MCBA_GUIDE_BY_*
constexpr int MAX_R = KI;                 // columns of W_c: mcba.h: MCBA_GUIDE_MAX_R
constexpr int MAX_NN = 6, MAX_COLS = MAX_R + MAX_NN;
constexpr int GS = 32;                    // side of the Gram matrix: two MFMA tiles
constexpr double PD_EPS = 1e-9;

// the record of a camera: its entry (is_fisheye and the coefficient count in the spare slots, as in a job of mcba_uncertainty.h),
// image size, r, then W_c [KI][MAX_R] (rows past the camera's own count and columns past r are 0)
constexpr int CREC_W_IMG = CAM_STRIDE, CREC_H_IMG = CAM_STRIDE + 1, CREC_RANK = CAM_STRIDE + 2, CREC_MARGIN = CAM_STRIDE + 3,
              CREC_W = CAM_STRIDE + 8, CREC_STRIDE = CREC_W + KI * MAX_R;
// the record of a view
constexpr int KIND_BOARD = 0, KIND_GRID = 1, KIND_LIST = 2;
constexpr int V_CAMERA = 0, V_NN = 1, V_MIN = 2, V_KIND = 3, V_BOARD = 4, V_POSE = 5, V_RHO = 17, V_GW = 18, V_N = 19, V_U0 = 20,
              V_V0 = 21, V_DU = 22, V_DV = 23, V_FIRST = 24, V_CENTRE = 25, V_STRIDE = 32;

// point i of a view: the scaled point Y, rho; false: not visible (no projection is attempted)
MCBA_HD bool view_point(const double* crec, const double* vrec, const double* board_points, int board_stride, const double* uv_lists,
                        int i, double* Y, double& rho) {
  const int kind = (int)vrec[V_KIND];
  if (kind == KIND_BOARD) {
    const double* X = board_points + ((size_t)(int)vrec[V_BOARD] * board_stride + i) * 3;
    const double* T = vrec + V_POSE;
    MCBA_UNROLL
    for (int k = 0; k < 3; ++k) Y[k] = T[4 * k] * X[0] + T[4 * k + 1] * X[1] + T[4 * k + 2] * X[2] + T[4 * k + 3];
    rho = 1.0;
    return Y[2] > 0.0;
  }
  double u, v;
  if (kind == KIND_GRID) {
    uncertainty::grid_pixel(i, (int)vrec[V_GW], vrec[V_U0], vrec[V_V0], vrec[V_DU], vrec[V_DV], u, v);
  } else {
    const double* q = uv_lists + 2 * ((size_t)vrec[V_FIRST] + i);
    u = q[0];
    v = q[1];
  }
  double x, y;
  if (!pnp::undistort_point(crec, (int)crec[uncertainty::REC_ND], crec[CAM_ISFISH] != 0.0, u, v, x, y)) return false;
  const double inv = 1.0 / sqrt(x * x + y * y + 1.0);
  Y[0] = x * inv; Y[1] = y * inv; Y[2] = inv;
  rho = vrec[V_RHO];
  return true;
}

// point i of a view where a camera sees it: the scaled point Y, rho, A = d(u, v) / dY and Kc padded to 2 x KI; false: not visible
// (in front, the projection finite, det d(u, v) / d(x, y) > 0 where it lands, a board's point inside the image by the margin)
MCBA_HD bool visible_point(const double* crec, const double* vrec, const double* board_points, int board_stride, const double* uv_lists,
                           int i, double* Y, double& rho, double* A, double* K) {
  double uv[2];
  bool visible = view_point(crec, vrec, board_points, board_stride, uv_lists, i, Y, rho);
  if (visible) visible = uncertainty::project_padded(crec, Y, uv, A, K);
  if (visible) visible = undistort::finite_d(uv[0]) && undistort::finite_d(uv[1]) && A[0] * A[4] - A[1] * A[3] > 0.0;
  if (visible && (int)vrec[V_KIND] == KIND_BOARD) {
    const double m = crec[CREC_MARGIN];
    visible = uv[0] >= m && uv[1] >= m && uv[0] <= crec[CREC_W_IMG] - 1.0 - m && uv[1] <= crec[CREC_H_IMG] - 1.0 - m;
  }
  return visible;
}

// the columns of a left rotation and of a translation of the point: A (e_k x Y), rho A e_k (three entries of each row)
MCBA_HD void rotation_columns(const double* A, const double* Y, double* row_u, double* row_v) {
  // e_0 x Y = (0, -Y2, Y1), e_1 x Y = (Y2, 0, -Y0), e_2 x Y = (-Y1, Y0, 0)
  row_u[0] = A[2] * Y[1] - A[1] * Y[2];
  row_v[0] = A[5] * Y[1] - A[4] * Y[2];
  row_u[1] = A[0] * Y[2] - A[2] * Y[0];
  row_v[1] = A[3] * Y[2] - A[5] * Y[0];
  row_u[2] = A[1] * Y[0] - A[0] * Y[1];
  row_v[2] = A[4] * Y[0] - A[3] * Y[1];
}
MCBA_HD void translation_columns(const double* A, double rho, double* row_u, double* row_v) {
  MCBA_UNROLL
  for (int k = 0; k < 3; ++k) {
    row_u[k] = rho * A[k];
    row_v[k] = rho * A[3 + k];
  }
}

// the two rows of point i, r + nn entries each, written to row_u / row_v (LDS on the device); false: not visible, the rows are 0
MCBA_HD bool point_rows(const double* crec, const double* vrec, const double* board_points, int board_stride, const double* uv_lists,
                        int i, int r, int nn, double* row_u, double* row_v) {
  double Y[3], rho = 0.0, A[6], K[2 * KI];
  const bool visible = visible_point(crec, vrec, board_points, board_stride, uv_lists, i, Y, rho, A, K);
  if (!visible) {
    MCBA_NOUNROLL
    for (int j = 0; j < r + nn; ++j) row_u[j] = row_v[j] = 0.0;
    return false;
  }
  const double* W = crec + CREC_W;
  MCBA_NOUNROLL
  for (int j = 0; j < r; ++j) {
    double s0 = 0.0, s1 = 0.0;
    MCBA_UNROLL
    for (int k = 0; k < KI; ++k) {
      const double w = W[k * MAX_R + j];
      s0 += K[k] * w;
      s1 += K[KI + k] * w;
    }
    row_u[j] = s0;
    row_v[j] = s1;
  }
  if (nn == 6) {
    // (a rotation about the view's centre spans, with the translations, what a rotation about the camera does)
    MCBA_UNROLL
    for (int k = 0; k < 3; ++k) Y[k] -= vrec[V_CENTRE + k];
  }
  if (nn >= 3) rotation_columns(A, Y, row_u + r, row_v + r);
  if (nn == 6) translation_columns(A, rho, row_u + r + 3, row_v + r + 3);
  return true;
}

MCBA_HD double gsym(const double* G, int i, int j) { return i <= j ? G[i * GS + j] : G[j * GS + i]; }

// Cholesky of the nuisance block of G (rows and columns r .. r + nn - 1), L [MAX_NN][MAX_NN] lower; false: not positive definite
MCBA_HD bool nuisance_factor(const double* G, int r, int nn, double* L) {
  for (int j = 0; j < nn; ++j)
    for (int i = j; i < nn; ++i) {
      double s = gsym(G, r + i, r + j);
      for (int k = 0; k < j; ++k) s -= L[i * MAX_NN + k] * L[j * MAX_NN + k];
      if (i == j) {
        if (!(s > PD_EPS * G[(r + j) * GS + r + j])) return false;
        L[j * MAX_NN + j] = sqrt(s);
      } else {
        L[i * MAX_NN + j] = s / L[j * MAX_NN + j];
      }
    }
  return true;
}
// column c of Y = L^-1 G_ek: Y [MAX_NN][MAX_R]
MCBA_HD void nuisance_column(const double* G, int r, int nn, const double* L, int c, double* Y) {
  for (int i = 0; i < nn; ++i) {
    double s = G[c * GS + r + i];
    for (int k = 0; k < i; ++k) s -= L[i * MAX_NN + k] * Y[k * MAX_R + c];
    Y[i * MAX_R + c] = s / L[i * MAX_NN + i];
  }
}
MCBA_HD double schur_entry(const double* G, int nn, const double* Y, int i, int j) {
  double s = gsym(G, i, j);
  for (int k = 0; k < nn; ++k) s -= Y[k * MAX_R + i] * Y[k * MAX_R + j];
  return s;
}
MCBA_HD int view_status(int n_visible, int min_points, bool factored) {
  return n_visible < min_points ? ST_TOO_FEW : factored ? ST_OK : ST_DEGENERATE;
}

// ---- scoring ----------------------------------------------------------------------------------------------------------------
// A [MAX_R][MAX_R] holds a symmetric matrix in its lower triangle and is replaced by its Cholesky factor; false: not positive definite
MCBA_HD bool chol_lower(int r, double* A) {
  for (int j = 0; j < r; ++j)
    for (int i = j; i < r; ++i) {
      double s = A[i * MAX_R + j];
      for (int k = 0; k < j; ++k) s -= A[i * MAX_R + k] * A[j * MAX_R + k];
      if (i == j) {
        if (!(s > 0.0)) return false;
        A[j * MAX_R + j] = sqrt(s);
      } else {
        A[i * MAX_R + j] = s / A[j * MAX_R + j];
      }
    }
  return true;
}
MCBA_HD double half_log_det(int r, const double* L) {
  double s = 0.0;
  for (int i = 0; i < r; ++i) s += log(L[i * MAX_R + i]);
  return s;
}
// column j of X = L^-1 Q (Q symmetric, row stride ldq): X [MAX_R][MAX_R]
MCBA_HD void forward_column(int r, const double* L, const double* Q, int ldq, int j, double* X) {
  for (int i = 0; i < r; ++i) {
    double s = Q[i * ldq + j];
    for (int k = 0; k < i; ++k) s -= L[i * MAX_R + k] * X[k * MAX_R + j];
    X[i * MAX_R + j] = s / L[i * MAX_R + i];
  }
}
// entry (i, i) of L^-1 X^T: the solution of L y = (row i of X)^T up to its entry i; y is kept in column i of Yw [MAX_R][MAX_R]
MCBA_HD double diagonal_entry(const double* L, const double* X, int i, double* Yw) {
  for (int k = 0; k <= i; ++k) {
    double s = X[i * MAX_R + k];
    for (int m = 0; m < k; ++m) s -= L[k * MAX_R + m] * Yw[m * MAX_R + i];
    Yw[k * MAX_R + i] = s / L[k * MAX_R + k];
  }
  return Yw[i * MAX_R + i];
}
// column j of (L L^T)^-1 = L^-T (L^-1 e_j) into P (row stride ldp); Yw as above
MCBA_HD void inverse_column(int r, const double* L, int j, double* Yw, double* P, int ldp) {
  for (int i = 0; i < r; ++i) {
    double s = i == j ? 1.0 : 0.0;
    for (int k = 0; k < i; ++k) s -= L[i * MAX_R + k] * Yw[k * MAX_R + j];
    Yw[i * MAX_R + j] = s / L[i * MAX_R + i];
  }
  for (int i = r - 1; i >= 0; --i) {
    double s = Yw[i * MAX_R + j];
    for (int k = i + 1; k < r; ++k) s -= L[k * MAX_R + i] * Yw[k * MAX_R + j];
    Yw[i * MAX_R + j] = s / L[i * MAX_R + i];
    P[i * ldp + j] = Yw[i * MAX_R + j];
  }
}
// lower triangle of M = B + inv_s2 S into A (S null: the base alone)
MCBA_HD void form_lower(int r, const double* B, const double* S, int ld, double inv_s2, double* A) {
  for (int i = 0; i < r; ++i)
    for (int j = 0; j <= i; ++j) {
      const double b = B[i * ld + j];
      A[i * MAX_R + j] = S ? b + inv_s2 * S[i * ld + j] : b;
    }
}
MCBA_HD double focus_rms_of(double trace, double n_focus) { return sqrt(fmax(trace, 0.0) / n_focus); }

}  // namespace guidance
}  // namespace mcba
