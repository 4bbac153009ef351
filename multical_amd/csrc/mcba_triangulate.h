// mcba_triangulate.h -- what a calibrated rig is used for second: the 3-D point behind the pixels several cameras saw at once.
//
// A view is a (camera c, frame f) pair with the row-major 3 x 4 matrix M[c,f] that takes a point of the rig's world frame into the
// camera frame (top three rows of camera_pose[c] @ rig_pose[f]).  Rolling shutter: the reference lerps the TRANSFORMED points
// (multical/motion/rolling_frames.py:21-41), which is linear in X, so one observation sees (1 - t) M + t M_end with t = v / image
// height -- the scan time of the bundle adjustment.  Per point (FP64 throughout):
//   usable views   the pixel goes back to its normalised ray through pnp::undistort_point (the exact Newton inverse of the
//                  project's projection); a view that is masked, not finite or does not invert is dropped, never fatal;
//   linear start   two planes a view (a1 = m1 - x m3, a2 = m2 - y m3, scaled to unit normals: point-to-plane distances in metres),
//                  N = sum n n^T, b = -sum d n in camera order, 3 x 3 Cholesky with a relative pivot floor;
//   refinement     Levenberg-Marquardt on the pixel residuals r_c = project(M_c X) - uv_c with the project's own projection and its
//                  analytic 2 x 3 derivative (project_point<ND, FISH, true>), damping schedule of pnp::lm_refine, stopped at an accepted
//                  step of whitened length sqrt(d^T H d) <= 1e-10 px;
//   covariance     sigma^2 H^-1 at the returned point.
// No per-view state is kept: every pass streams the observations again (a 64-bit mask remembers which views are usable), so the
// registers do not grow with the number of cameras.  Every loop has a constant upper bound.
// MCBA_HD like mcba_pnp.h: k_triangulate (mcba_triangulate_kernels.h) and tests/triangulate_host compile this source.
#pragma once
#include <stdint.h>
#include "mcba_undistort.h"

namespace mcba {
namespace triangulate {

constexpr int ST_OK = 0, ST_TOO_FEW = 1, ST_DEGENERATE = 2, ST_NOT_CONVERGED = 3, ST_BEHIND = 4;   // mcba.h: MCBA_TRI_*
constexpr int MAX_CAMERAS = 64;             // mcba.h: MCBA_TRI_MAX_CAMERAS (the usable-view mask is one 64-bit word; 40 KiB of LDS)
constexpr int DEFAULT_ITERATIONS = 20, MAX_ITERATIONS = 100;
constexpr double STOP_PX = 1e-10;           // whitened length of the last accepted step
constexpr double PIVOT_FLOOR = 1e-12;       // x trace(N): below it the planes do not fix a point
constexpr double RESIDUAL_ROUNDING = 1e-12; // px: rounding a residual carries (2^-52 x a coordinate of thousands of px x a few operations)
constexpr int SOLVE_RETRIES = 8;           // damped systems tried before a linearisation is given up

// The record of one camera in one frame, as the kernel stages it in LDS and the host build in a vector: the camera_entry (whose
// spare slots carry what the entry lacks), then the view matrix and the end matrix of the frame.
constexpr int REC_VIEW = CAM_STRIDE, REC_END = CAM_STRIDE + 12, REC_STRIDE = CAM_STRIDE + 24;
constexpr int REC_ND = 49, REC_VIEW_OK = 50;   // spare slots of a camera_entry: coefficient count, view_valid[c,f]
static_assert(REC_VIEW_OK < CAM_STRIDE && REC_ND > CAM_ISFISH, "the spare slots of a camera_entry");

struct Tables {                 // what the records are staged from
  int C, F;
  const double* cam;            // [C][CAM_STRIDE] camera_entry with CAM_HEIGHT, CAM_ISFISH and REC_ND filled in
  const double* views;          // [C,F,12]
  const double* views_end;      // [C,F,12] or null
  const uint8_t* view_valid;    // [C,F] or null
};

// entry i of the C * REC_STRIDE doubles of frame f
MCBA_HD double staged_value(const Tables& t, int f, int i) {
  const int c = i / REC_STRIDE, k = i - c * REC_STRIDE;
  const size_t view = (size_t)c * t.F + f;
  if (k == REC_VIEW_OK) return (t.view_valid == nullptr || t.view_valid[view] != 0) ? 1.0 : 0.0;
  if (k < REC_VIEW) return t.cam[(size_t)c * CAM_STRIDE + k];
  if (k < REC_END) return t.views[view * 12 + (k - REC_VIEW)];
  return t.views_end ? t.views_end[view * 12 + (k - REC_END)] : 0.0;
}

// the observations of one point: camera c at uv[c * uv_stride], valid[c * valid_stride]; err (or null) likewise
struct Observations {
  const double* uv;
  const uint8_t* valid;
  double* err;
  size_t uv_stride, valid_stride, err_stride;
};

// the matrix one observation sees: the frame's, or the lerp at the scan time of the observed row
MCBA_HD void view_matrix(const double* rec, bool rolling, double v, double* Mv) {
  const double* M = rec + REC_VIEW;
  if (!rolling) {
    MCBA_UNROLL
    for (int i = 0; i < 12; ++i) Mv[i] = M[i];
    return;
  }
  const double* E = rec + REC_END;
  const double t = v / rec[CAM_HEIGHT], s = 1.0 - t;
  MCBA_UNROLL
  for (int i = 0; i < 12; ++i) Mv[i] = s * M[i] + t * E[i];
}

MCBA_HD void transform(const double* Mv, const double* X, double* Xc) {
  MCBA_UNROLL
  for (int r = 0; r < 3; ++r) Xc[r] = Mv[4 * r] * X[0] + Mv[4 * r + 1] * X[1] + Mv[4 * r + 2] * X[2] + Mv[4 * r + 3];
}

// pixel of the camera-frame point Xc and d(u, v) / d Xc through the camera's own family (as undistort::project_any selects it)
MCBA_HD void project_jac(const double* rec, const double* Xc, double* uv, double* A) {
  const double* ext = rec + CAM_TILT;
  const int nd = (int)rec[REC_ND];
  double Kc[2 * (4 + MAX_DIST)];
  if (rec[CAM_ISFISH] != 0.0) { project_point<4, 1, true>(rec, ext, Xc, uv, A, Kc); return; }
  switch (nd) {
    case 4: project_point<4, 0, true>(rec, ext, Xc, uv, A, Kc); break;
    case 5: project_point<5, 0, true>(rec, ext, Xc, uv, A, Kc); break;
    case 8: project_point<8, 0, true>(rec, ext, Xc, uv, A, Kc); break;
    case 12: project_point<12, 0, true>(rec, ext, Xc, uv, A, Kc); break;
    case 14: project_point<14, 0, true>(rec, ext, Xc, uv, A, Kc); break;
    default:                     // (plan_cameras lets no other family through)
      uv[0] = uv[1] = undistort::quiet_nan();
      MCBA_UNROLL
      for (int i = 0; i < 6; ++i) A[i] = undistort::quiet_nan();
      break;
  }
}

// packed symmetric 3 x 3: S = [s00 s01 s02 s11 s12 s22];  L = [l00 l10 l11 l20 l21 l22]
MCBA_HD bool chol3(const double* S, double min_pivot, double* L) {
  if (!(S[0] > min_pivot)) return false;
  L[0] = sqrt(S[0]);
  L[1] = S[1] / L[0];
  L[3] = S[2] / L[0];
  const double d1 = S[3] - L[1] * L[1];
  if (!(d1 > min_pivot)) return false;
  L[2] = sqrt(d1);
  L[4] = (S[4] - L[3] * L[1]) / L[2];
  const double d2 = S[5] - L[3] * L[3] - L[4] * L[4];
  if (!(d2 > min_pivot)) return false;
  L[5] = sqrt(d2);
  return true;
}
MCBA_HD void chol3_solve(const double* L, const double* b, double* x) {
  const double z0 = b[0] / L[0];
  const double z1 = (b[1] - L[1] * z0) / L[2];
  const double z2 = (b[2] - L[3] * z0 - L[4] * z1) / L[5];
  x[2] = z2 / L[5];
  x[1] = (z1 - L[4] * x[2]) / L[2];
  x[0] = (z0 - L[1] * x[1] - L[3] * x[2]) / L[0];
}
MCBA_HD double quad3(const double* S, const double* d) {      // d^T S d
  return S[0] * d[0] * d[0] + S[3] * d[1] * d[1] + S[5] * d[2] * d[2] + 2.0 * (S[1] * d[0] * d[1] + S[2] * d[0] * d[2] + S[4] * d[1] * d[2]);
}

// the linear start; sets the mask of usable views and their number.  false: the planes do not fix a point
MCBA_HD bool linear_start(const double* recs, int C, bool rolling, const Observations& o, uint64_t& usable, int& n, double* X) {
  double N[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
  usable = 0;
  n = 0;
  MCBA_NOUNROLL
  for (int c = 0; c < C; ++c) {
    const double* rec = recs + (size_t)c * REC_STRIDE;
    if (o.valid[c * o.valid_stride] == 0 || rec[REC_VIEW_OK] == 0.0) continue;
    const double u = o.uv[c * o.uv_stride], v = o.uv[c * o.uv_stride + 1];
    if (!undistort::finite_d(u) || !undistort::finite_d(v)) continue;
    double x, y;
    if (!pnp::undistort_point(rec, (int)rec[REC_ND], rec[CAM_ISFISH] != 0.0, u, v, x, y)) continue;
    double Mv[12];
    view_matrix(rec, rolling, v, Mv);
    bool planes = true;
    double rows[8];
    MCBA_UNROLL
    for (int k = 0; k < 2; ++k) {
      const double w = k == 0 ? x : y;
      double a[4];
      MCBA_UNROLL
      for (int j = 0; j < 4; ++j) a[j] = Mv[4 * k + j] - w * Mv[8 + j];
      const double len = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
      if (!(len > 0.0) || !(len < 1e300)) planes = false;
      const double il = 1.0 / len;
      MCBA_UNROLL
      for (int j = 0; j < 4; ++j) rows[4 * k + j] = a[j] * il;
    }
    if (!planes) continue;
    usable |= (uint64_t)1 << c;
    ++n;
    MCBA_UNROLL
    for (int k = 0; k < 2; ++k) {
      const double* q = rows + 4 * k;
      N[0] += q[0] * q[0]; N[1] += q[0] * q[1]; N[2] += q[0] * q[2];
      N[3] += q[1] * q[1]; N[4] += q[1] * q[2]; N[5] += q[2] * q[2];
      b[0] -= q[3] * q[0]; b[1] -= q[3] * q[1]; b[2] -= q[3] * q[2];
    }
  }
  if (n < 2) return false;
  double L[6];
  if (!chol3(N, PIVOT_FLOOR * (N[0] + N[3] + N[5]), L)) return false;
  chol3_solve(L, b, X);
  return undistort::finite_d(X[0]) && undistort::finite_d(X[1]) && undistort::finite_d(X[2]);
}

// H = sum J^T J (packed), g = sum J^T r, cost = sum |r|^2 over the usable views at X
MCBA_HD void linearize(const double* recs, int C, bool rolling, const Observations& o, uint64_t usable, const double* X, double* H,
                       double* g, double* cost) {
  MCBA_UNROLL
  for (int i = 0; i < 6; ++i) H[i] = 0.0;
  g[0] = g[1] = g[2] = 0.0;
  double sse = 0.0;
  MCBA_NOUNROLL
  for (int c = 0; c < C; ++c) {
    if (!((usable >> c) & 1)) continue;
    const double* rec = recs + (size_t)c * REC_STRIDE;
    const double u = o.uv[c * o.uv_stride], v = o.uv[c * o.uv_stride + 1];
    double Mv[12], Xc[3], uv[2], A[6];
    view_matrix(rec, rolling, v, Mv);
    transform(Mv, X, Xc);
    project_jac(rec, Xc, uv, A);
    const double r0 = uv[0] - u, r1 = uv[1] - v;
    double J[6];                 // A (2 x 3) . rotation part of Mv
    MCBA_UNROLL
    for (int k = 0; k < 2; ++k) {
      MCBA_UNROLL
      for (int j = 0; j < 3; ++j) J[3 * k + j] = A[3 * k] * Mv[j] + A[3 * k + 1] * Mv[4 + j] + A[3 * k + 2] * Mv[8 + j];
    }
    H[0] += J[0] * J[0] + J[3] * J[3]; H[1] += J[0] * J[1] + J[3] * J[4]; H[2] += J[0] * J[2] + J[3] * J[5];
    H[3] += J[1] * J[1] + J[4] * J[4]; H[4] += J[1] * J[2] + J[4] * J[5]; H[5] += J[2] * J[2] + J[5] * J[5];
    g[0] += J[0] * r0 + J[3] * r1; g[1] += J[1] * r0 + J[4] * r1; g[2] += J[2] * r0 + J[5] * r1;
    sse += r0 * r0 + r1 * r1;
  }
  *cost = sse;
}

// per-view errors |r_c| (0 where the view did not enter) and whether any usable view has the point at or behind its plane
MCBA_HD bool final_errors(const double* recs, int C, bool rolling, const Observations& o, uint64_t usable, const double* X) {
  bool behind = false;
  MCBA_NOUNROLL
  for (int c = 0; c < C; ++c) {
    double e = 0.0;
    if ((usable >> c) & 1) {
      const double* rec = recs + (size_t)c * REC_STRIDE;
      const double u = o.uv[c * o.uv_stride], v = o.uv[c * o.uv_stride + 1];
      double Mv[12], Xc[3], uv[2];
      view_matrix(rec, rolling, v, Mv);
      transform(Mv, X, Xc);
      undistort::project_any(rec, (int)rec[REC_ND], rec[CAM_ISFISH] != 0.0, Xc, uv);
      e = sqrt((uv[0] - u) * (uv[0] - u) + (uv[1] - v) * (uv[1] - v));
      behind = behind || !(Xc[2] > 0.0);
    }
    if (o.err) o.err[c * o.err_stride] = e;
  }
  return behind;
}

struct PointResult {
  double X[3], cov[6], sse;
  int n_views, status;
};

MCBA_HD int clamp_iterations(int max_iterations) {
  return max_iterations <= 0 ? DEFAULT_ITERATIONS : max_iterations > MAX_ITERATIONS ? MAX_ITERATIONS : max_iterations;
}

// one point.  recs: the C records of its frame; max_iter: linearisations, already clamped.  Without a result: NaN in X and cov,
// sse 0, err 0.  BEHIND is decided last and replaces OK and NOT_CONVERGED alike.
MCBA_HD void triangulate_point(const double* recs, int C, bool rolling, const Observations& o, double sigma_px, int max_iter,
                               PointResult& out) {
  const double nan = undistort::quiet_nan();
  out.X[0] = out.X[1] = out.X[2] = nan;
  MCBA_UNROLL
  for (int i = 0; i < 6; ++i) out.cov[i] = nan;
  out.sse = 0.0;
  uint64_t usable;
  double X[3];
  const bool started = linear_start(recs, C, rolling, o, usable, out.n_views, X);
  double H[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0}, cost = 0.0;
  bool have = false, converged = false;
  if (started) {
    double Q[3] = {X[0], X[1], X[2]}, d[3] = {0, 0, 0};
    double lambda = 1e-3;
    MCBA_NOUNROLL
    for (int used = 0; used < max_iter; ++used) {        // ONE linearisation per round, at the trial point Q
      double Hq[6], gq[3], cq;
      linearize(recs, C, rolling, o, usable, Q, Hq, gq, &cq);
      bool accept;
      if (!have) {
        if (!(cq < 1e300)) break;                          // (non-finite at the start: no result)
        accept = have = true;
      } else {
        // a trial within rounding of the current cost counts as a descent.  Rounding here is not relative to the cost: each of
        // the 2 n residuals carries RESIDUAL_ROUNDING px of the projection's own rounding whatever its size, so the cost carries
        // 2 |r| |e| <= 2 sqrt(cost 2 n) RESIDUAL_ROUNDING -- at a small cost far more than pnp::LM_ACCEPT_SLACK x cost, and a
        // trial rejected for it would raise the damping and let a shrunken step pass the stop rule.  STOP_PX^2: what the stop rule
        // itself resolves (noise-free observations end at a cost of rounding errors alone).
        accept = cq <= cost * (1.0 + pnp::LM_ACCEPT_SLACK) + 2.0 * sqrt(cost * (double)(2 * out.n_views)) * RESIDUAL_ROUNDING +
                           STOP_PX * STOP_PX;
      }
      if (accept) {
        const double whitened = sqrt(fmax(quad3(H, d), 0.0));   // (H of the point the step left; 0 in the first round)
        const bool step = used > 0;
        MCBA_UNROLL
        for (int i = 0; i < 3; ++i) { X[i] = Q[i]; g[i] = gq[i]; }
        MCBA_UNROLL
        for (int i = 0; i < 6; ++i) H[i] = Hq[i];
        cost = cq;
        if (step) {
          lambda = fmax(lambda * 0.1, 1e-15);
          if (whitened <= STOP_PX) { converged = true; break; }
        }
      } else {
        lambda = fmin(lambda * 10.0, 1e30);
      }
      bool solved = false;
      MCBA_NOUNROLL
      for (int k = 0; k < SOLVE_RETRIES && !solved; ++k) {
        const double Hd[6] = {H[0] * (1.0 + lambda), H[1], H[2], H[3] * (1.0 + lambda), H[4], H[5] * (1.0 + lambda)};
        const double rhs[3] = {-g[0], -g[1], -g[2]};
        double L[6];
        solved = chol3(Hd, 0.0, L);
        if (solved) chol3_solve(L, rhs, d);
        else lambda = lambda * 10.0 + 1e-12;
      }
      if (!solved) break;
      MCBA_UNROLL
      for (int i = 0; i < 3; ++i) Q[i] = X[i] + d[i];
    }
  }
  // errors are written for every point (zeros without a result); the mask is empty unless the start stood
  const bool behind = final_errors(recs, C, rolling, o, have ? usable : 0, X);
  if (!started || !have) {
    out.status = out.n_views < 2 ? ST_TOO_FEW : ST_DEGENERATE;
    return;
  }
  out.X[0] = X[0]; out.X[1] = X[1]; out.X[2] = X[2];
  out.sse = cost;
  const double sigma2 = sigma_px > 0.0 ? sigma_px * sigma_px : cost / (double)(2 * out.n_views - 3);
  double L[6];
  if (chol3(H, 0.0, L)) {
    double c0[3], c1[3], c2[3];
    const double e0[3] = {1, 0, 0}, e1[3] = {0, 1, 0}, e2[3] = {0, 0, 1};
    chol3_solve(L, e0, c0);
    chol3_solve(L, e1, c1);
    chol3_solve(L, e2, c2);
    out.cov[0] = sigma2 * c0[0]; out.cov[1] = sigma2 * c1[0]; out.cov[2] = sigma2 * c2[0];
    out.cov[3] = sigma2 * c1[1]; out.cov[4] = sigma2 * c2[1]; out.cov[5] = sigma2 * c2[2];
  }
  out.status = behind ? ST_BEHIND : converged ? ST_OK : ST_NOT_CONVERGED;
}

}  // namespace triangulate
}  // namespace mcba
