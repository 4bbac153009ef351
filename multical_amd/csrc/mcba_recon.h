// mcba_recon.h -- how well a calibrated rig measures 3-D: the 3 x 3 covariance of a triangulated point under the covariance of the
// calibration itself, beside the pixel noise of the point.
//
// A job is (camera group c_1 .. c_G, 2 <= G <= MAX_G; reference = the rig frame or a camera a of the group; per camera the factor
// W_c [KC][r] in the column order of mcba_rigview.h: fx fy cx cy | 14 coefficients | left perturbation (omega, tau) of T_c).  A query is
// a point X of the rig frame and a 64-bit mask of the group slots that may be used.  Per allowed slot c:
//   Y_c = R_c X + t_c,  (uv_c, A_c, Kc_c) = project_padded(Y_c);  c is a VIEW of the point when Y_c.z > 0, the family is served,
//   det d(u, v) / d(X, Y) > 0 (the monotone test of mcba_uncertainty.h) and uv_c lies in [-margin, W + margin) x [-margin, H + margin);
//   J_c = A_c R_c (2 x 3),  P_c = [Kc_c | A_c [-[Y_c]x | I]] (2 x KC),  B_c = J_c^T P_c (3 x KC),  H = sum_c J_c^T J_c.
// The point triangulated from the noise-free pixels q_c = uv_c solves sum_c J_c^T r_c = 0 with r_c = 0: the terms with second
// derivatives carry a factor r_c and vanish, so d X / d(parameters) = -H^-1 [B_1 .. B_G] exactly.  Per column j of the factor
//   u_j = sum_c B_c W_c[:, j]      the views in ascending slot order, k ascending inside a camera, one running sum per coordinate
//   z_j = -H^-1 u_j                H^-1 from the packed Cholesky factor of mcba_triangulate.h (chol3, chol3_solve of the unit vectors)
//   camera a as reference:         z_j <- R_a z_j + omega_aj x Y_a + tau_aj, (omega, tau) = W_a[KI .. KI + 6, j]: the point in a's frame.
//                                  A common motion of every camera pose cancels in it (the gauge-free form).
//   cov_cal = sum_j z_j z_j^T      in LANES = 16 interleaved partial sums (partial l takes the columns j = l, l + 16, .. ascending),
//                                  added in the order l = 0 .. 15: the order of the kernel, stated once for both builds
//   cov_noise = sigma2 H^-1        R_a (sigma2 H^-1) R_a^T with a reference camera
// Status: fewer than two views TOO_FEW; a Cholesky pivot of H at or below 1e-12 trace(H) DEGENERATE (the rule of mcba_triangulate.h);
// a view or the reference camera whose factor is flagged unconstrained UNCONSTRAINED; decided in this order.  Anything but OK: NaN.
// Pairs of points of a job -- the covariance of X_a - X_b, of the length |X_a - X_b| and cov(X_a, X_b) -- follow below (pair_query).
// MCBA_HD like mcba_uncertainty.h: k_reconstruction_uncertainty, k_reconstruction_pairs (mcba_recon_kernels.h), tests/recon_host and
// tests/length_host compile this source.
#pragma once
#include <stdint.h>
#include "mcba_triangulate.h"
#include "mcba_uncertainty.h"

namespace mcba {
namespace recon {

using uncertainty::KI;

constexpr int ST_OK = 0, ST_TOO_FEW = 1, ST_DEGENERATE = 2, ST_UNCONSTRAINED = 3;   // mcba.h: MCBA_RECON_*
constexpr int MAX_G = 8;                   // mcba.h: MCBA_RECON_MAX_CAMERAS
constexpr int MAX_R = 128;                 // mcba.h: MCBA_RIG_MAX_R
constexpr int KC = KI + 6;                 // columns of a camera: mcba.h: MCBA_RIG_COLUMNS
constexpr int LANES = 16;                  // interleaved partial sums of cov_cal
constexpr double PIVOT_FLOOR = triangulate::PIVOT_FLOOR;

// The record of a job: a head, then one record per slot: the camera_entry (spare slots as in mcba_uncertainty.h), R_c | t_c as the
// 3 x 4 row-major matrix, the image size and the unconstrained flag.
constexpr int SL_POSE = CAM_STRIDE, SL_W_IMG = SL_POSE + 12, SL_H_IMG = SL_W_IMG + 1, SL_LOOSE = SL_H_IMG + 1, SL_STRIDE = CAM_STRIDE + 16;
constexpr int JR_G = 0, JR_REF = 1, JR_R = 2, JR_LDW = 3, JR_MARGIN = 4, JR_SLOT = 8, JR_STRIDE = JR_SLOT + MAX_G * SL_STRIDE;
static_assert(SL_LOOSE < SL_STRIDE && JR_MARGIN < JR_SLOT, "the records of a job");

MCBA_HD int padded_columns(int r) { return (r + 15) / 16 * 16; }        // ldw: row stride of the job's factor [24 G][ldw], zero-padded
MCBA_HD const double* slot_of(const double* rec, int s) { return rec + JR_SLOT + s * SL_STRIDE; }

struct View {
  double Y[3], J[6], P[2 * KC];
};

MCBA_HD void to_camera(const double* T, const double* X, double* Y) {
  MCBA_UNROLL
  for (int i = 0; i < 3; ++i) Y[i] = T[4 * i] * X[0] + T[4 * i + 1] * X[1] + T[4 * i + 2] * X[2] + T[4 * i + 3];
}

// whether the camera of `slot` is a view of X, and its Y, J, P where it is
MCBA_HD bool view_of_point(const double* slot, double margin, const double* X, View& v) {
  const double* T = slot + SL_POSE;
  to_camera(T, X, v.Y);
  if (!(v.Y[2] > 0.0)) return false;
  double uv[2], A[6];
  if (!uncertainty::project_padded(slot, v.Y, uv, A, v.P)) return false;         // (Kc in rows of KI)
  if (!(A[0] * A[4] - A[1] * A[3] > 0.0)) return false;
  const double W = slot[SL_W_IMG], H = slot[SL_H_IMG];
  if (!(uv[0] >= -margin && uv[0] < W + margin && uv[1] >= -margin && uv[1] < H + margin)) return false;
  MCBA_UNROLL
  for (int k = 0; k < 2; ++k) {
    MCBA_UNROLL
    for (int j = 0; j < 3; ++j) v.J[3 * k + j] = A[3 * k] * T[j] + A[3 * k + 1] * T[4 + j] + A[3 * k + 2] * T[8 + j];
  }
  // rows of KI -> rows of KC, from the back: the second row first
  MCBA_UNROLL
  for (int k = KI - 1; k >= 0; --k) v.P[KC + k] = v.P[KI + k];
  base_row(A, v.Y, v.P + KI);
  base_row(A + 3, v.Y, v.P + KC + KI);
  return true;
}
// B_c[i][k] = J[0][i] P[0][k] + J[1][i] P[1][k]
MCBA_HD double b_entry(const View& v, int i, int k) { return v.J[i] * v.P[k] + v.J[3 + i] * v.P[KC + k]; }
MCBA_HD void view_B(const View& v, double* B) {
  MCBA_UNROLL
  for (int i = 0; i < 3; ++i) {
    MCBA_UNROLL
    for (int k = 0; k < KC; ++k) B[i * KC + k] = b_entry(v, i, k);
  }
}
// packed J^T J: [h00 h01 h02 h11 h12 h22]
MCBA_HD void view_H(const View& v, double* h) {
  const double* J = v.J;
  h[0] = J[0] * J[0] + J[3] * J[3]; h[1] = J[0] * J[1] + J[3] * J[4]; h[2] = J[0] * J[2] + J[3] * J[5];
  h[3] = J[1] * J[1] + J[4] * J[4]; h[4] = J[1] * J[2] + J[4] * J[5]; h[5] = J[2] * J[2] + J[5] * J[5];
}

// what the views of a point leave behind: H summed in slot order, then factored
struct Point {
  double Hi[6];            // H^-1, packed
  double Ya[3];            // the point in the reference camera
  int n_views, status;
  uint64_t views;
};

// packed inverse of H; false: a pivot at or below PIVOT_FLOOR trace(H)
MCBA_HD bool inverse3(const double* H, double* Hi) {
  double L[6];
  if (!triangulate::chol3(H, PIVOT_FLOOR * (H[0] + H[3] + H[5]), L)) return false;
  double c0[3], c1[3], c2[3];
  const double e0[3] = {1, 0, 0}, e1[3] = {0, 1, 0}, e2[3] = {0, 0, 1};
  triangulate::chol3_solve(L, e0, c0);
  triangulate::chol3_solve(L, e1, c1);
  triangulate::chol3_solve(L, e2, c2);
  Hi[0] = c0[0]; Hi[1] = c1[0]; Hi[2] = c2[0]; Hi[3] = c1[1]; Hi[4] = c2[1]; Hi[5] = c2[2];
  return true;
}
MCBA_HD int point_status(int n_views, bool factored, bool loose) {
  return n_views < 2 ? ST_TOO_FEW : !factored ? ST_DEGENERATE : loose ? ST_UNCONSTRAINED : ST_OK;
}
// from H (summed over the views in slot order), the views and whether one of them or the reference camera is unconstrained
MCBA_HD void point_H(const double* rec, const double* X, const double* H, int n_views, uint64_t views, bool loose, Point& p) {
  p.n_views = n_views;
  p.views = views;
  const int ref = (int)rec[JR_REF];
  if (ref >= 0) {
    loose = loose || slot_of(rec, ref)[SL_LOOSE] != 0.0;
    to_camera(slot_of(rec, ref) + SL_POSE, X, p.Ya);
  } else {
    p.Ya[0] = p.Ya[1] = p.Ya[2] = 0.0;
  }
  const bool factored = n_views >= 2 && inverse3(H, p.Hi);
  p.status = point_status(n_views, factored, loose);
}

MCBA_HD void sym3_times(const double* S, const double* x, double* y) {
  y[0] = S[0] * x[0] + S[1] * x[1] + S[2] * x[2];
  y[1] = S[1] * x[0] + S[3] * x[1] + S[4] * x[2];
  y[2] = S[2] * x[0] + S[4] * x[1] + S[5] * x[2];
}
// z of one column from its u; pose: (omega, tau) of the reference camera in that column (not read in the rig form)
MCBA_HD void response(const double* rec, const Point& p, const double* u, const double* pose, double* z) {
  double hu[3];
  sym3_times(p.Hi, u, hu);
  z[0] = -hu[0]; z[1] = -hu[1]; z[2] = -hu[2];
  const int ref = (int)rec[JR_REF];
  if (ref < 0) return;
  const double* T = slot_of(rec, ref) + SL_POSE;
  double rz[3], wy[3];
  MCBA_UNROLL
  for (int i = 0; i < 3; ++i) rz[i] = T[4 * i] * z[0] + T[4 * i + 1] * z[1] + T[4 * i + 2] * z[2];
  cross3(pose, p.Ya, wy);
  MCBA_UNROLL
  for (int i = 0; i < 3; ++i) z[i] = rz[i] + wy[i] + pose[3 + i];
}
MCBA_HD void add_outer(const double* z, double* c) {
  c[0] += z[0] * z[0]; c[1] += z[0] * z[1]; c[2] += z[0] * z[2];
  c[3] += z[1] * z[1]; c[4] += z[1] * z[2]; c[5] += z[2] * z[2];
}
// sigma2 H^-1, in the reference camera R_a (.) R_a^T
MCBA_HD void noise_covariance(const double* rec, const Point& p, double sigma2, double* c) {
  const int ref = (int)rec[JR_REF];
  if (ref < 0) {
    MCBA_UNROLL
    for (int i = 0; i < 6; ++i) c[i] = sigma2 * p.Hi[i];
    return;
  }
  const double* T = slot_of(rec, ref) + SL_POSE;
  double M[9];                      // H^-1 R_a^T, column i = H^-1 (row i of R_a)
  MCBA_UNROLL
  for (int i = 0; i < 3; ++i) {
    const double r[3] = {T[4 * i], T[4 * i + 1], T[4 * i + 2]};
    double y[3];
    sym3_times(p.Hi, r, y);
    M[i] = y[0]; M[3 + i] = y[1]; M[6 + i] = y[2];
  }
  int at = 0;
  MCBA_UNROLL
  for (int i = 0; i < 3; ++i) {
    MCBA_UNROLL
    for (int j = i; j < 3; ++j) c[at++] = sigma2 * (T[4 * i] * M[j] + T[4 * i + 1] * M[3 + j] + T[4 * i + 2] * M[6 + j]);
  }
}

struct Result {
  double cov_cal[6], cov_noise[6];
  int n_views, status;
  uint64_t views;
};

// the views of a point: B of every slot into Bs [3][KC G] (zero where the slot is no view), H in slot order
MCBA_HD void point_views(const double* rec, const double* X, uint64_t mask, double* Bs, Point& p) {
  const int G = (int)rec[JR_G];
  double H[6] = {0, 0, 0, 0, 0, 0};
  int n = 0;
  uint64_t views = 0;
  bool loose = false;
  for (int s = 0; s < G; ++s) {
    View v;
    const bool is_view = ((mask >> s) & 1) != 0 && view_of_point(slot_of(rec, s), rec[JR_MARGIN], X, v);
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < KC; ++k) Bs[i * KC * G + s * KC + k] = is_view ? b_entry(v, i, k) : 0.0;
    if (!is_view) continue;
    double h[6];
    view_H(v, h);
    for (int i = 0; i < 6; ++i) H[i] += h[i];
    ++n;
    views |= (uint64_t)1 << s;
    loose = loose || slot_of(rec, s)[SL_LOOSE] != 0.0;
  }
  point_H(rec, X, H, n, views, loose, p);
}

// one point, plain loops in the orders stated at the head.  Wj [KC G][ldw]: the job's factor, rows of slot s at KC s
MCBA_HD void query(const double* rec, const double* Wj, const double* X, uint64_t mask, double sigma2, Result& out) {
  const double nan = undistort::quiet_nan();
  const int G = (int)rec[JR_G], r = (int)rec[JR_R], ldw = (int)rec[JR_LDW], ref = (int)rec[JR_REF];
  double Bs[3 * KC * MAX_G];
  Point p;
  point_views(rec, X, mask, Bs, p);
  out.n_views = p.n_views; out.views = p.views; out.status = p.status;
  for (int i = 0; i < 6; ++i) out.cov_cal[i] = out.cov_noise[i] = nan;
  if (p.status != ST_OK) return;
  noise_covariance(rec, p, sigma2, out.cov_noise);
  double part[LANES][6];
  for (int l = 0; l < LANES; ++l)
    for (int i = 0; i < 6; ++i) part[l][i] = 0.0;
  for (int j = 0; j < r; ++j) {
    double u[3] = {0.0, 0.0, 0.0}, pose[6] = {0, 0, 0, 0, 0, 0}, z[3];
    for (int k = 0; k < KC * G; ++k) {
      const double w = Wj[(size_t)k * ldw + j];
      u[0] += Bs[k] * w;
      u[1] += Bs[KC * G + k] * w;
      u[2] += Bs[2 * KC * G + k] * w;
    }
    if (ref >= 0)
      for (int m = 0; m < 6; ++m) pose[m] = Wj[(size_t)(KC * ref + KI + m) * ldw + j];
    response(rec, p, u, pose, z);
    add_outer(z, part[j % LANES]);
  }
  for (int i = 0; i < 6; ++i) {
    double s = part[0][i];
    for (int l = 1; l < LANES; ++l) s += part[l][i];
    out.cov_cal[i] = s;
  }
}

// ---- pairs of points of one job: the covariance of X_a - X_b and of |X_a - X_b| ------------------------
// The calibration's error is common to all points, so per column j of the factor the two ends move by nearly the same vector:
//   d_j = z_j(X_a) - z_j(X_b)                the subtraction per column, BEFORE squaring -- never C_a + C_b - C_ab - C_ab^T
//   cov_diff_cal = sum_j d_j d_j^T           positive semi-definite by construction; a == b: exactly 0
//   cross_cal    = sum_j z_j(X_a) z_j(X_b)^T the full 3 x 3, row-major; cross(b, a) = cross(a, b)^T; a == b: the point's cov_cal
// both in the LANES interleaved partial sums of cov_cal, added in the same order; r = 0: exactly 0.
//   cov_diff_noise = cov_noise(a) + cov_noise(b)   (the pixel noise of two different points is independent); a == b: exactly 0
//   length = |X_a - X_b|,  u = (X_a - X_b) / length taken to the output frame,  length_var_* = u^T cov_diff_* u; length == 0: NaN.
// A common motion of the output frame moves both ends rigidly and its rotation term omega x (X_a - X_b) is perpendicular to u: to
// first order length_var_* does not depend on the reference, the rig frame or any camera pose being held.
// Each end keeps its own views (mask, margin).  Status: that of a unless it is OK, then that of b; anything but OK: NaN, the length
// and the view masks of both ends excepted.
struct PairResult {
  double cov_diff_cal[6], cross_cal[9], cov_diff_noise[6], length, length_var_cal, length_var_noise;
  int status;
  uint64_t views_a, views_b;
};
MCBA_HD int pair_status(int status_a, int status_b) { return status_a != ST_OK ? status_a : status_b; }
// d = za - zb into the pair's sums: diff [6] += d d^T, cross [9] += za zb^T
MCBA_HD void add_pair(const double* za, const double* zb, double* diff, double* cross) {
  const double d[3] = {za[0] - zb[0], za[1] - zb[1], za[2] - zb[2]};
  add_outer(d, diff);
  MCBA_UNROLL
  for (int i = 0; i < 3; ++i) {
    MCBA_UNROLL
    for (int k = 0; k < 3; ++k) cross[3 * i + k] += za[i] * zb[k];
  }
}
// what follows the sums: the noise of the difference, the length and the variances of the length; NaN where the pair is not OK
MCBA_HD void pair_finish(const double* rec, const double* Xa, const double* Xb, bool same, int status_a, int status_b,
                         const double* noise_a, const double* noise_b, const double* diff, const double* cross, PairResult& out) {
  const double nan = undistort::quiet_nan();
  out.status = pair_status(status_a, status_b);
  const double dX[3] = {Xa[0] - Xb[0], Xa[1] - Xb[1], Xa[2] - Xb[2]};
  out.length = sqrt(dX[0] * dX[0] + dX[1] * dX[1] + dX[2] * dX[2]);
  const bool ok = out.status == ST_OK;
  MCBA_UNROLL
  for (int i = 0; i < 6; ++i) {
    out.cov_diff_cal[i] = ok ? diff[i] : nan;
    out.cov_diff_noise[i] = !ok ? nan : same ? 0.0 : noise_a[i] + noise_b[i];
  }
  MCBA_UNROLL
  for (int i = 0; i < 9; ++i) out.cross_cal[i] = ok ? cross[i] : nan;
  out.length_var_cal = out.length_var_noise = nan;
  if (!ok || !(out.length > 0.0)) return;
  double u[3] = {dX[0] / out.length, dX[1] / out.length, dX[2] / out.length};
  const int ref = (int)rec[JR_REF];
  if (ref >= 0) {                    // the covariances are in the frame of the reference camera
    const double* T = slot_of(rec, ref) + SL_POSE;
    const double v[3] = {u[0], u[1], u[2]};
    MCBA_UNROLL
    for (int i = 0; i < 3; ++i) u[i] = T[4 * i] * v[0] + T[4 * i + 1] * v[1] + T[4 * i + 2] * v[2];
  }
  double cu[3];
  sym3_times(out.cov_diff_cal, u, cu);
  out.length_var_cal = u[0] * cu[0] + u[1] * cu[1] + u[2] * cu[2];
  sym3_times(out.cov_diff_noise, u, cu);
  out.length_var_noise = u[0] * cu[0] + u[1] * cu[1] + u[2] * cu[2];
}

// one pair, plain loops in the orders stated above; same: a and b are one index
MCBA_HD void pair_query(const double* rec, const double* Wj, const double* Xa, const double* Xb, uint64_t mask_a, uint64_t mask_b,
                        bool same, double sigma2, PairResult& out) {
  const int G = (int)rec[JR_G], r = (int)rec[JR_R], ldw = (int)rec[JR_LDW], ref = (int)rec[JR_REF];
  double Ba[3 * KC * MAX_G], Bb[3 * KC * MAX_G];
  Point pa, pb;
  point_views(rec, Xa, mask_a, Ba, pa);
  point_views(rec, Xb, mask_b, Bb, pb);
  out.views_a = pa.views; out.views_b = pb.views;
  double na[6] = {0, 0, 0, 0, 0, 0}, nb[6] = {0, 0, 0, 0, 0, 0};
  double diff[LANES][6], cross[LANES][9], sd[6], sc[9];
  for (int l = 0; l < LANES; ++l) {
    for (int i = 0; i < 6; ++i) diff[l][i] = 0.0;
    for (int i = 0; i < 9; ++i) cross[l][i] = 0.0;
  }
  if (pair_status(pa.status, pb.status) == ST_OK) {
    noise_covariance(rec, pa, sigma2, na);
    noise_covariance(rec, pb, sigma2, nb);
    for (int j = 0; j < r; ++j) {
      double ua[3] = {0.0, 0.0, 0.0}, ub[3] = {0.0, 0.0, 0.0}, pose[6] = {0, 0, 0, 0, 0, 0}, za[3], zb[3];
      for (int k = 0; k < KC * G; ++k) {
        const double w = Wj[(size_t)k * ldw + j];
        ua[0] += Ba[k] * w; ua[1] += Ba[KC * G + k] * w; ua[2] += Ba[2 * KC * G + k] * w;
        ub[0] += Bb[k] * w; ub[1] += Bb[KC * G + k] * w; ub[2] += Bb[2 * KC * G + k] * w;
      }
      if (ref >= 0)
        for (int m = 0; m < 6; ++m) pose[m] = Wj[(size_t)(KC * ref + KI + m) * ldw + j];
      response(rec, pa, ua, pose, za);
      response(rec, pb, ub, pose, zb);
      add_pair(za, zb, diff[j % LANES], cross[j % LANES]);
    }
  }
  for (int i = 0; i < 6; ++i) {
    sd[i] = diff[0][i];
    for (int l = 1; l < LANES; ++l) sd[i] += diff[l][i];
  }
  for (int i = 0; i < 9; ++i) {
    sc[i] = cross[0][i];
    for (int l = 1; l < LANES; ++l) sc[i] += cross[l][i];
  }
  pair_finish(rec, Xa, Xb, same, pa.status, pb.status, na, nb, sd, sc, out);
}

// tests: G = -H^-1 [B_1 .. B_G] [3][KC G] with the reference term included (the unit columns of every parameter); the status
MCBA_HD int query_rows(const double* rec, const double* X, uint64_t mask, double* Gm) {
  const int G = (int)rec[JR_G], ref = (int)rec[JR_REF];
  double Bs[3 * KC * MAX_G];
  Point p;
  point_views(rec, X, mask, Bs, p);
  for (int i = 0; i < 3 * KC * G; ++i) Gm[i] = 0.0;
  if (p.status != ST_OK && p.status != ST_UNCONSTRAINED) return p.status;
  for (int k = 0; k < KC * G; ++k) {
    const double u[3] = {Bs[k], Bs[KC * G + k], Bs[2 * KC * G + k]};
    double pose[6] = {0, 0, 0, 0, 0, 0}, z[3];
    if (ref >= 0 && k >= KC * ref + KI && k < KC * (ref + 1)) pose[k - KC * ref - KI] = 1.0;
    response(rec, p, u, pose, z);
    for (int i = 0; i < 3; ++i) Gm[i * KC * G + k] = z[i];
  }
  return p.status;
}

}  // namespace recon
}  // namespace mcba
