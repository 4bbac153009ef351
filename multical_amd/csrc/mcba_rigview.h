// mcba_rigview.h -- where to hold the board next so that SEVERAL cameras see it: the information a candidate view adds to the
// intrinsics AND the poses of a camera group, and what it does to the transfer uncertainty between its cameras.
//
// A RIG VIEW is board b at the board-in-rig pose Z in a new frame whose rig pose is free, seen by every camera c of the group that
// it falls into.  A SLOT is (view, camera): the board at the board-in-camera pose T_c Z, with the visibility test of mcba_guidance.h.
// The two rows of a visible point in camera c, KC = 24 columns:
//   [0, KI)        Kc                               fx fy cx cy | 14 coefficients, padded
//   [KI, KI + 6)   P' = A [ -[Y - c_c]x | I ]       a left rotation of the point about c_c = T_c ctr, the board's centroid as camera c
//                                                   sees it, and a translation
// G_vc = [K | P']^T [K | P'] (KC x KC) is summed over the visible points of the slot.  The left perturbation of T_c (mcba_uncertainty.h:
// P = A [ -[Y]x | I ]) is P = P' M_c, M_c = [[I, 0], [-[c_c]x, I]], and the six columns of the free frame pose -- a rotation about ctr
// in the rig frame and a translation -- are E_c = P [[R_c, 0], [[c_c]x R_c, R_c]] = P' D_c with D_c = blockdiag(R_c, R_c): the G_vc
// carry everything, and no product cancels (rows about the camera's origin would leave the nuisance block of a far, small board with
// the rounding error of |Y|^2 where it holds |Y - c_c|^2; a single corner has rotation columns that are exactly 0).  With W_c [KC, r]
// the rows of the prior's factor in the columns of camera c and W'_c = blockdiag(I, M_c) W_c (centred_w),
//   S_v = sum_c W'_c^T G_vc W'_c - U^T G_xx^-1 U,   U = sum_c D_c^T G_vc[P', :] W'_c  [6, r],   G_xx = sum_c D_c^T G_vc[P', P'] D_c
// over the cameras that CONTRIBUTE (at least min_points visible points): Cholesky of G_xx with the pivot rule of mcba_guidance.h,
// Y = L^-1 U, S_v = sum - Y^T Y.  Scoring against the base B (SPD, r x r): M = B + S_v / sigma^2 = L L^T in place (row stride ld),
//   half log det = sum log L_ii,   X = L^-1 in place,   trace(M^-1 Q) = sum_i X[i, :] Q X[i, :]^T,   M^-1 = X^T X.
// Every sum below has one order, stated where it is formed; the kernels (mcba_rigview_kernels.h) and tests/rigview call the same
// functions entry by entry.
#pragma once
#include <stdint.h>
#include "mcba_guidance.h"

namespace mcba {
namespace rigview {

using guidance::CRIT_FOCUS;
using guidance::CRIT_GAIN;
using guidance::GS;
using guidance::ST_DEGENERATE;
using guidance::ST_OK;
using guidance::ST_TOO_FEW;
using guidance::ST_UNCONSTRAINED;
using uncertainty::KI;
using uncertainty::KP;

constexpr int MAX_R = 128;                 // columns of the factor: mcba.h: MCBA_RIG_MAX_R
constexpr int KC = KI + 6;                 // columns of a camera: intrinsics | pose
constexpr int NN = 6;                      // the free frame pose
// the record of a camera: that of mcba_guidance.h without its factor
constexpr int RC_STRIDE = guidance::CREC_W;
// the record of a slot: a board view of mcba_guidance.h (V_CAMERA, V_MIN, V_KIND, V_BOARD, V_POSE = T_c Z, V_N, V_CENTRE = c_c), then
// D_c [6][6]
constexpr int S_D = guidance::V_STRIDE, S_STRIDE = S_D + 40;
// the record of a focus pair (a, b): the head of a job record of mcba_uncertainty.h (no W)
constexpr int F_STRIDE = uncertainty::REC_W;

// the two rows of point i of a slot, KC entries each; false: not visible, the rows are 0
MCBA_HD bool point_rows(const double* crec, const double* srec, const double* board_points, int board_stride, int i, double* row_u,
                        double* row_v) {
  double Y[3], rho = 0.0, A[6], K[2 * KI];
  const bool visible = guidance::visible_point(crec, srec, board_points, board_stride, nullptr, i, Y, rho, A, K);
  if (!visible) {
    MCBA_UNROLL
    for (int j = 0; j < KC; ++j) row_u[j] = row_v[j] = 0.0;
    return false;
  }
  MCBA_UNROLL
  for (int k = 0; k < KI; ++k) {
    row_u[k] = K[k];
    row_v[k] = K[KI + k];
  }
  MCBA_UNROLL
  for (int k = 0; k < 3; ++k) Y[k] -= srec[guidance::V_CENTRE + k];
  guidance::rotation_columns(A, Y, row_u + KI, row_v + KI);
  guidance::translation_columns(A, rho, row_u + KI + 3, row_v + KI + 3);
  return true;
}
// the centroid of a board's points `mean` as the slot's camera sees it: the formula of guidance::view_point (a board of one corner has
// Y - c_c = 0 exactly)
MCBA_HD void slot_centre(const double* T, const double* mean, double* cc) {
  for (int k = 0; k < 3; ++k) cc[k] = T[4 * k] * mean[0] + T[4 * k + 1] * mean[1] + T[4 * k + 2] * mean[2] + T[4 * k + 3];
}
// entry (k, j) of W'_c = blockdiag(I, M_c) W_c: the translation rows take -c_c x (the rotation rows); W_c [KC][ld]
MCBA_HD double centred_w(const double* W, int ld, const double* cc, int k, int j) {
  const double w = W[k * ld + j];
  if (k < KI + 3) return w;
  const int a = k - KI - 3, b = a == 2 ? 0 : a + 1, c = a == 0 ? 2 : a - 1;          // (c x w)_a = c_b w_c - c_c w_b
  return w - (cc[b] * W[(KI + c) * ld + j] - cc[c] * W[(KI + b) * ld + j]);
}

MCBA_HD bool contributes(int n_visible, int min_points) { return n_visible > 0 && n_visible >= min_points; }

// ---- assembly of S_v: W and T = G W are [KC][ld], G [KC][KC] symmetric and full, D [6][6], U and Y [6][ld] -----------------------
// T[k][j] = sum_m G[k][m] W[m][j], m ascending
MCBA_HD double gw_entry(const double* G, const double* W, int ld, int k, int j) {
  double s = 0.0;
  for (int m = 0; m < KC; ++m) s += G[k * KC + m] * W[m * ld + j];
  return s;
}
// acc + sum_k W[k][i] T[k][j], k ascending, added one by one to the running sum
MCBA_HD double wtw_add(const double* W, const double* T, int ld, int i, int j, double acc) {
  for (int k = 0; k < KC; ++k) acc += W[k * ld + i] * T[k * ld + j];
  return acc;
}
// (D^T T[P, :])[q][j] = sum_p D[p][q] T[KI + p][j]
MCBA_HD double du_entry(const double* D, const double* T, int ld, int q, int j) {
  double s = 0.0;
  for (int p = 0; p < NN; ++p) s += D[p * NN + q] * T[(KI + p) * ld + j];
  return s;
}
// (D^T G[P, P] D)[q][s] = sum_p D[p][q] (sum_t G[KI + p][KI + t] D[t][s])
MCBA_HD double gxx_entry(const double* D, const double* G, int q, int s) {
  double out = 0.0;
  for (int p = 0; p < NN; ++p) {
    double in = 0.0;
    for (int t = 0; t < NN; ++t) in += G[(KI + p) * KC + KI + t] * D[t * NN + s];
    out += D[p * NN + q] * in;
  }
  return out;
}
// column c of Y = L^-1 U in place (L [MAX_NN][MAX_NN] of guidance::nuisance_factor)
MCBA_HD void nuisance_solve(const double* L, double* U, int ld, int c) {
  for (int i = 0; i < NN; ++i) {
    double s = U[i * ld + c];
    for (int k = 0; k < i; ++k) s -= L[i * guidance::MAX_NN + k] * U[k * ld + c];
    U[i * ld + c] = s / L[i * guidance::MAX_NN + i];
  }
}
MCBA_HD double yty_sub(const double* Y, int ld, int i, int j, double acc) {
  for (int k = 0; k < NN; ++k) acc -= Y[k * ld + i] * Y[k * ld + j];
  return acc;
}
// TOO_FEW before UNCONSTRAINED before DEGENERATE
MCBA_HD int view_status(int n_cameras, int min_cameras, bool loose, bool factored) {
  return n_cameras < min_cameras ? ST_TOO_FEW : loose ? ST_UNCONSTRAINED : factored ? ST_OK : ST_DEGENERATE;
}

// ---- scoring: M [r][ld], lower triangle, upper triangle 0 -----------------------------------------------------------------------
// one term of the Cholesky factorisation: M[i][k] -= L[i][j] L[k][j] (j ascending per entry in either loop order)
MCBA_HD void chol_term(double* M, int ld, int i, int k, int j) { M[i * ld + k] -= M[i * ld + j] * M[k * ld + j]; }
// host order of the same factorisation; false: a pivot is not positive
MCBA_HD bool chol_lower(int r, double* M, int ld) {
  for (int j = 0; j < r; ++j) {
    const double d = M[j * ld + j];
    if (!(d > 0.0)) return false;
    const double l = sqrt(d);
    M[j * ld + j] = l;
    for (int i = j + 1; i < r; ++i) M[i * ld + j] = M[i * ld + j] / l;
    for (int i = j + 1; i < r; ++i)
      for (int k = j + 1; k <= i; ++k) chol_term(M, ld, i, k, j);
  }
  return true;
}
MCBA_HD double half_log_det(int r, const double* L, int ld) {
  double s = 0.0;
  for (int i = 0; i < r; ++i) s += log(L[i * ld + i]);
  return s;
}
// entry (i, j), j <= i, of X = L^-1 when rows 0 .. i - 1 of M hold X already and row_l is row i of L: k ascending
MCBA_HD double inverse_entry(const double* M, int ld, const double* row_l, int i, int j) {
  double s = i == j ? 1.0 : 0.0;
  for (int k = j; k < i; ++k) s -= row_l[k] * M[k * ld + j];
  return s / row_l[i];
}
// X[i, :] Q X[i, :]^T = sum_a X[i][a] (sum_b Q[a][b] X[i][b]), a, b = 0 .. i ascending
MCBA_HD double trace_row(const double* X, int ld, const double* Q, int ldq, int i) {
  double out = 0.0;
  for (int a = 0; a <= i; ++a) {
    double in = 0.0;
    for (int b = 0; b <= i; ++b) in += Q[a * ldq + b] * X[i * ld + b];
    out += X[i * ld + a] * in;
  }
  return out;
}
// (X^T X)[a][b] = sum_i X[i][a] X[i][b], i = max(a, b) .. r - 1 ascending
MCBA_HD double posterior_entry(int r, const double* X, int ld, int a, int b) {
  double s = 0.0;
  for (int i = a > b ? a : b; i < r; ++i) s += X[i * ld + a] * X[i * ld + b];
  return s;
}
// row stride of M in LDS: odd, so that a column is read without bank conflicts
MCBA_HD int score_stride(int r) { return r | 1; }

}  // namespace rigview
}  // namespace mcba
