// mcba_projdiff.h -- comparing two calibrations of one rig: the projection difference of a pixel, the
// twin of mcba_uncertainty.h (which predicts the covariance this difference is supposed to stay within).
//
// Two calibrations 0 and 1 of the same cameras.  A job is (camera b, reference, inverse distance rho, fit mode); a query is a pixel q.
// n_c^k(q) is the UNIT ray of the pixel through the exact Newton inverse (pnp::undistort_point) of camera c under calibration k, and
// the scaled point Y = rho X is what is carried, as in mcba_uncertainty.h: rho = 0 is no special case.
//   reference = the camera itself   Y = n_b^0(q),  q' = project_b^1(R(omega) Y + rho tau),  diff = q' - q.  (omega, tau) is the
//                                   IMPLIED TRANSFORM of the job, fitted once before the map: it minimises sum |diff_i|^2 over the
//                                   job's fit pixels (a grid or a list of their own, restricted to a focus disc).
//   reference = camera a            Y_a^k = n_a^k(q),  Y_b^k = R_ba^k Y_a^k + rho t_ba^k,  q_b^k = project_b^k(Y_b^k),
//                                   diff = q_b^1 - q_b^0, landing = q_b^0.  Gauge-free: no fit.  a == b returns exactly 0.
// The fit is localize::solve_frame (Levenberg-Marquardt, Marquardt scaling, stopped at an accepted step of whitened length
// sqrt(d^T J^T J d) <= 1e-10 px: no fit pixel moves further) over 3 (ROTATION) or 6 (RIGID) unknowns from the identity, through a
// BACK-END as there: one workgroup per job on the device (mcba_projdiff_kernels.h), a plain loop in SerialBackend below.  The
// unknowns are the rotation vector and the translation themselves; the row pair of a fit pixel is base_rows' pair at the rotated
// ray, its rotation columns times L(omega), its translation columns times rho (localize::obs_rows without a camera pose).
// A fit pixel takes part if it lies in the focus disc, its inverse under calibration 0 converges and its projection under
// calibration 1 is valid (in front of the camera, det d(u, v) / d(X, Y) > 0) AT THE IDENTITY: the set is decided once, in the first
// pass, and does not change while the transform moves.
// MCBA_HD like mcba_uncertainty.h: the kernels and tests/projdiff_host compile this source.
#pragma once
#include <stdint.h>
#include "mcba_localize.h"
#include "mcba_uncertainty.h"

namespace mcba {
namespace projdiff {

constexpr int ST_OK = 0, ST_NOT_CONVERGED = 1, ST_BEHIND = 2, ST_NO_FIT = 3;                    // mcba.h: MCBA_PDIFF_*
constexpr int FIT_OK = 0, FIT_TOO_FEW = 1, FIT_NOT_CONVERGED = 2, FIT_DEGENERATE = 3;           // mcba.h: MCBA_PDIFF_FIT_*
constexpr int MODE_NONE = 0, MODE_ROTATION = 1, MODE_RIGID = 2;                                 // mcba.h: MCBA_PDIFF_MODE_*
constexpr int MAX_FIT_PIXELS = 65536;            // mcba.h: MCBA_PDIFF_MAX_FIT (the rays stay L2 resident: 3 MiB)
// linearisations of a fit.  Calibrations that agree to a few pixels take 5 .. 11; a rigid fit that leaves tens of pixels behind
// (a rolling-shutter rig whose second focal length is off by 12 %) converges linearly and was measured at 86 .. 176
constexpr int MAX_ITERATIONS = 400;
using triangulate::REC_ND;
using localize::GS;
using localize::MAX_K;

// the record of a job: camera b under calibration 0 and 1, camera a under 0 and 1, R_ba | t_ba of 0 and 1, the scalars
constexpr int REC_B0 = 0, REC_B1 = CAM_STRIDE, REC_A0 = 2 * CAM_STRIDE, REC_A1 = 3 * CAM_STRIDE, REC_RT0 = 4 * CAM_STRIDE,
              REC_RT1 = REC_RT0 + 12, REC_RHO = REC_RT1 + 12, REC_HAS_A = REC_RHO + 1, REC_MODE = REC_HAS_A + 1,
              REC_SAME = REC_MODE + 1, REC_STRIDE = 256;
static_assert(REC_SAME < REC_STRIDE, "the record of a job");
// what a fit leaves behind for the map: omega | tau | n_fit iterations rms_before rms_after status
constexpr int FIT_NFIT = 6, FIT_ITERS = 7, FIT_RMS0 = 8, FIT_RMS1 = 9, FIT_STATUS = 10, FIT_STRIDE = 12;
// a fit pixel in the scratch buffer: the ray under calibration 0 | the pixel | takes part
constexpr int RAY_N = 0, RAY_UV = 3, RAY_OK = 5, RAY_STRIDE = 6;
// the transform as a query reads it: R | rho tau | the job has a transform
constexpr int XF_R = 0, XF_T = 9, XF_OK = 12, XF_STRIDE = 16;

MCBA_HD int n_unknowns(int mode) { return mode == MODE_RIGID ? 6 : 3; }
MCBA_HD int min_pixels(int mode) { return mode == MODE_RIGID ? 3 : 2; }

struct Result {
  double du, dv, mag, lu, lv;
  int status;
};

MCBA_HD bool unit_ray(const double* cam, double u, double v, double* n) {
  double x, y;
  if (!pnp::undistort_point(cam, (int)cam[REC_ND], cam[CAM_ISFISH] != 0.0, u, v, x, y)) return false;
  const double inv = 1.0 / sqrt(x * x + y * y + 1.0);
  n[0] = x * inv; n[1] = y * inv; n[2] = inv;
  return true;
}

// pixel of the scaled point Y through camera `cam`; status: BEHIND, or NOT_CONVERGED outside the model's monotone range
MCBA_HD int project_checked(const double* cam, const double* Y, double* uv) {
  if (!(Y[2] > 0.0)) return ST_BEHIND;
  double A[6];
  triangulate::project_jac(cam, Y, uv, A);
  if (!(A[0] * A[4] - A[1] * A[3] > 0.0)) return ST_NOT_CONVERGED;
  return ST_OK;
}

// xf of a job from what its fit left behind (a job that does not fit has the identity and FIT_OK there)
MCBA_HD void stage_transform(const double* rec, const double* fit, double* xf) {
  double L[9];
  rodrigues(fit, xf + XF_R, L);
  const double rho = rec[REC_RHO];
  MCBA_UNROLL
  for (int i = 0; i < 3; ++i) xf[XF_T + i] = rho * fit[3 + i];
  xf[XF_OK] = fit[FIT_STATUS] == (double)FIT_OK ? 1.0 : 0.0;
  xf[13] = xf[14] = xf[15] = 0.0;
}

// one query
MCBA_HD void query(const double* rec, const double* xf, double u, double v, Result& out) {
  const double nan = undistort::quiet_nan();
  out.du = out.dv = out.mag = out.lu = out.lv = nan;
  double n[3], Y[3], q1[2];
  if (rec[REC_HAS_A] == 0.0) {
    if (xf[XF_OK] == 0.0) { out.status = ST_NO_FIT; return; }
    if (!unit_ray(rec + REC_B0, u, v, n)) { out.status = ST_NOT_CONVERGED; return; }
    mat3_vec(xf + XF_R, n, Y);
    MCBA_UNROLL
    for (int i = 0; i < 3; ++i) Y[i] += xf[XF_T + i];
    out.status = project_checked(rec + REC_B1, Y, q1);
    if (out.status != ST_OK) return;
    out.du = q1[0] - u;
    out.dv = q1[1] - v;
  } else {
    const double rho = rec[REC_RHO];
    double q0[2];
    if (!unit_ray(rec + REC_A0, u, v, n)) { out.status = ST_NOT_CONVERGED; return; }
    mat3_vec(rec + REC_RT0, n, Y);
    MCBA_UNROLL
    for (int i = 0; i < 3; ++i) Y[i] += rho * rec[REC_RT0 + 9 + i];
    out.status = project_checked(rec + REC_B0, Y, q0);
    if (out.status != ST_OK) return;
    if (!unit_ray(rec + REC_A1, u, v, n)) { out.status = ST_NOT_CONVERGED; return; }
    mat3_vec(rec + REC_RT1, n, Y);
    MCBA_UNROLL
    for (int i = 0; i < 3; ++i) Y[i] += rho * rec[REC_RT1 + 9 + i];
    out.status = project_checked(rec + REC_B1, Y, q1);
    if (out.status != ST_OK) return;
    if (rec[REC_SAME] != 0.0) {          // the point is where the camera itself sees it under either calibration: exactly 0
      out.du = out.dv = 0.0;
      out.lu = u;
      out.lv = v;
    } else {
      out.du = q1[0] - q0[0];
      out.dv = q1[1] - q0[1];
      out.lu = q0[0];
      out.lv = q0[1];
    }
  }
  const double a = out.du * out.du;
  const double b = out.dv * out.dv;
  out.mag = sqrt(a + b);
}

// ---------------------------------------------------------------------------------------------------------
// the fit.  A fit pixel is RAY_STRIDE doubles of the scratch buffer; pe: pose entry (R | t | L) of the transform
// ---------------------------------------------------------------------------------------------------------
struct Focus {
  double u, v, radius;          // radius <= 0: the whole image
};

// first pass: the ray of fit pixel (u, v) and whether it takes part
MCBA_HD void fit_ray(const double* rec, const Focus& f, double u, double v, double* ray) {
  double n[3] = {0.0, 0.0, 0.0}, q[2];
  bool ok = true;
  if (f.radius > 0.0) {
    const double du = u - f.u, dv = v - f.v;
    ok = du * du + dv * dv <= f.radius * f.radius;
  }
  ok = ok && unit_ray(rec + REC_B0, u, v, n);
  ok = ok && project_checked(rec + REC_B1, n, q) == ST_OK;
  ray[RAY_N] = n[0]; ray[RAY_N + 1] = n[1]; ray[RAY_N + 2] = n[2];
  ray[RAY_UV] = u; ray[RAY_UV + 1] = v;
  ray[RAY_OK] = ok ? 1.0 : 0.0;
}

// the two rows [J | r] of a fit pixel that takes part: K + 1 entries each
template <int K>
MCBA_HD void fit_rows(const double* rec, const double* pe, const double* ray, double* ru, double* rv) {
  const double rho = rec[REC_RHO];
  double RY[3], X[3], uv[2], A[6], E[12];
  mat3_vec(pe + POSE_R, ray + RAY_N, RY);
  MCBA_UNROLL
  for (int i = 0; i < 3; ++i) X[i] = RY[i] + rho * pe[POSE_T + i];
  triangulate::project_jac(rec + REC_B1, X, uv, A);
  base_rows(A, RY, E);
  const double* L = pe + POSE_L;
  MCBA_UNROLL
  for (int c = 0; c < 3; ++c) {
    ru[c] = E[0] * L[c] + E[1] * L[3 + c] + E[2] * L[6 + c];
    rv[c] = E[6] * L[c] + E[7] * L[3 + c] + E[8] * L[6 + c];
    if constexpr (K == 6) {
      ru[3 + c] = rho * E[3 + c];
      rv[3 + c] = rho * E[9 + c];
    }
  }
  ru[K] = uv[0] - ray[RAY_UV];
  rv[K] = uv[1] - ray[RAY_UV + 1];
}

// squared difference of a fit pixel that takes part
MCBA_HD double fit_sq(const double* rec, const double* pe, const double* ray) {
  const double rho = rec[REC_RHO];
  double X[3], uv[2];
  mat3_vec(pe + POSE_R, ray + RAY_N, X);
  MCBA_UNROLL
  for (int i = 0; i < 3; ++i) X[i] += rho * pe[POSE_T + i];
  const double* cam = rec + REC_B1;
  undistort::project_any(cam, (int)cam[REC_ND], cam[CAM_ISFISH] != 0.0, X, uv);
  const double du = uv[0] - ray[RAY_UV], dv = uv[1] - ray[RAY_UV + 1];
  return du * du + dv * dv;
}

// what a job leaves behind: status from the run of localize::solve_frame
MCBA_HD void fit_record(const double* p, int K, int n_fit, int iters, double cost0, double cost1, int status, double* fit) {
  const double nan = undistort::quiet_nan();
  for (int i = 0; i < 6; ++i) fit[i] = status == FIT_OK ? (i < K ? p[i] : 0.0) : nan;
  fit[FIT_NFIT] = (double)n_fit;
  fit[FIT_ITERS] = (double)iters;
  fit[FIT_RMS0] = n_fit > 0 && cost0 >= 0.0 ? sqrt(cost0 / (double)n_fit) : nan;
  fit[FIT_RMS1] = status == FIT_OK ? sqrt(cost1 / (double)n_fit) : nan;
  fit[FIT_STATUS] = (double)status;
  fit[11] = 0.0;
}

// the record of a job that does not fit: the identity
MCBA_HD void fit_identity(double* fit) {
  for (int i = 0; i < FIT_STRIDE; ++i) fit[i] = 0.0;
  fit[FIT_RMS0] = fit[FIT_RMS1] = undistort::quiet_nan();
}

// the plain-loop back-end of localize::solve_frame: fit pixels in order
template <int K>
struct SerialBackend {
  const double* rec;
  const double* rays;
  int n;
  double p[6], q[6], pe[POSE_STRIDE], qe[POSE_STRIDE], G[GS * GS], A[MAX_K * MAX_K], cost0 = -1.0;

  void entries(const double* x, double* e) {
    double x6[6] = {x[0], x[1], x[2], 0.0, 0.0, 0.0};
    for (int i = 3; i < K; ++i) x6[i] = x[i];
    pose_entry(x6, e);
  }
  void start() {
    for (int i = 0; i < 6; ++i) p[i] = 0.0;
    entries(p, pe);
  }
  double linearize() {
    for (int i = 0; i < GS * GS; ++i) G[i] = 0.0;
    for (int i = 0; i < n; ++i) {
      const double* ray = rays + (size_t)i * RAY_STRIDE;
      if (ray[RAY_OK] == 0.0) continue;
      double ru[K + 1], rv[K + 1];
      fit_rows<K>(rec, pe, ray, ru, rv);
      for (int a = 0; a <= K; ++a)
        for (int b = a; b <= K; ++b) G[a * GS + b] += ru[a] * ru[b] + rv[a] * rv[b];
    }
    if (cost0 < 0.0) cost0 = G[K * GS + K];
    return G[K * GS + K];
  }
  bool well_posed() { return localize::well_posed(K, G, A); }
  bool solve(double lambda, double* whitened) {
    double d[MAX_K];
    if (!localize::damped_step(K, G, lambda, A, d, whitened)) return false;
    for (int i = 0; i < K; ++i) q[i] = p[i] + d[i];
    entries(q, qe);
    return true;
  }
  double cost_at(const double* e) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) {
      const double* ray = rays + (size_t)i * RAY_STRIDE;
      if (ray[RAY_OK] != 0.0) s += fit_sq(rec, e, ray);
    }
    return s;
  }
  double trial_cost() { return cost_at(qe); }
  void accept() {
    for (int i = 0; i < K; ++i) p[i] = q[i];
    for (int i = 0; i < POSE_STRIDE; ++i) pe[i] = qe[i];
  }
};

// status of a finished run of localize::solve_frame
MCBA_HD int fit_status(bool have, bool converged) { return !have ? FIT_DEGENERATE : converged ? FIT_OK : FIT_NOT_CONVERGED; }

// one job on the host.  rays [n][RAY_STRIDE]: the first pass, already made
template <int K>
inline void fit_job_as(const double* rec, const double* rays, int n, double* fit) {
  int n_fit = 0;
  for (int i = 0; i < n; ++i) n_fit += rays[(size_t)i * RAY_STRIDE + RAY_OK] != 0.0 ? 1 : 0;
  const double zero[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (n_fit < min_pixels(K == 6 ? MODE_RIGID : MODE_ROTATION)) return fit_record(zero, K, n_fit, 0, -1.0, 0.0, FIT_TOO_FEW, fit);
  SerialBackend<K> be;
  be.rec = rec; be.rays = rays; be.n = n;
  be.start();
  bool have = false;
  int iters = 0;
  double cost = 0.0;
  const bool converged = localize::solve_frame(be, n_fit, MAX_ITERATIONS, &have, &iters, &cost);
  fit_record(be.p, K, n_fit, iters, be.cost0, have ? be.cost_at(be.pe) : 0.0, fit_status(have, converged), fit);
}
inline void fit_job(const double* rec, const double* rays, int n, double* fit) {
  if ((int)rec[REC_MODE] == MODE_RIGID) fit_job_as<6>(rec, rays, n, fit);
  else fit_job_as<3>(rec, rays, n, fit);
}

// pixel i of a job's queries or fit set: a grid (uncertainty::grid_pixel: the one definition) or a list
struct PixelSet {
  long long list;               // first pixel in `uv`, -1: a grid
  int grid_w;
  double u0, v0, du, dv;
};
MCBA_HD void pixel_of(const PixelSet& s, const double* uv, long long i, double& u, double& v) {
  if (s.list < 0) {
    uncertainty::grid_pixel(i, s.grid_w, s.u0, s.v0, s.du, s.dv, u, v);
  } else {
    u = uv[2 * (s.list + i)];
    v = uv[2 * (s.list + i) + 1];
  }
}

}  // namespace projdiff
}  // namespace mcba
