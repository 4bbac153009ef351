// mcba_localize.h -- what a calibrated rig is used for third: where the rig was in a frame that was not part of the calibration.
//
// The dual of mcba_triangulate.h (rig known, point unknown): cameras, camera poses, boards and board poses are held, and every frame
// is one small dense least-squares problem over its own rig pose (FP64 throughout):
//   cost          sum over the frame's usable observations (camera c, world point W = board_pose[b] X[b,p]) of
//                 |project_c(camera_pose[c] rig W) - uv|^2 in pixels; rolling shutter as in the bundle adjustment and in
//                 mcba_triangulate.h: X_cam = (1 - t) cam start W + t cam end W, t = v_observed / image_height[c] (constant in the
//                 parameters), 12 unknowns: start, then end;
//   unknowns      the project's parameterisation of a motion block: GLOBAL rotation vector, then translation (rx ry rz tx ty tz),
//                 with d(R(w) y)/dw = -[R y]x L(w) (rodrigues of mcba_math.h) -- so the covariance returned is the conditional
//                 covariance of the frame's block of Calibration.covariance();
//   rows          [J | r] of an observation: A (2 x 3, triangulate::project_jac: the project's own projection and derivative) times
//                 the camera rotation, times (-[R W]x L | I) (base_rows), times the lerp weight; K + 1 = 7 or 13 columns;
//   start         the frame's own `init` pose, or the best of up to four candidates camera_pose[c]^-1 T_view board_pose[b]^-1 from
//                 pnp::view_pose of its largest views, scored over ALL the frame's observations (a point at or behind its camera
//                 counts as the squared image diagonal): the planar flip of one view is outvoted by the other cameras;
//   refinement    Levenberg-Marquardt with Marquardt scaling and the damping schedule of triangulate_point; a trial point costs one
//                 residual-only pass, an accepted one is linearised again; stopped at an accepted step of whitened length
//                 sqrt(d^T J^T J d) <= 1e-10 px;
//   covariance    sigma^2 (J^T J)^-1 of the last linearisation (at most one accepted step of 1e-10 px from the returned pose).
// The loop (solve_frame) is written against a BACK-END like intr::lm_loop: who walks the observations, in which order the sums are
// formed and where the barriers are is the back-end's business -- one workgroup per frame on the device (mcba_localize_kernels.h),
// a plain loop in SerialBackend below (tests/localize_host).  Every value a back-end method returns is the same in every thread.
#pragma once
#include <stdint.h>
#include "mcba_intrinsic.h"
#include "mcba_triangulate.h"

namespace mcba {
namespace localize {

constexpr int ST_OK = 0, ST_TOO_FEW = 1, ST_DEGENERATE = 2, ST_NOT_CONVERGED = 3, ST_BEHIND = 4;   // mcba.h: MCBA_RIG_*
constexpr int MAX_CAMERAS = 64;             // mcba.h: MCBA_RIG_MAX_CAMERAS (the camera records are staged in LDS)
constexpr int DEFAULT_ITERATIONS = 20, MAX_ITERATIONS = 100;
constexpr double STOP_PX = 1e-10;           // whitened length of the last accepted step
constexpr double PIVOT_FLOOR = 1e-12;       // squared pivot of the Cholesky factor of D^-1/2 H D^-1/2, D = diag(H)
constexpr double RESIDUAL_ROUNDING = 1e-12; // px: see triangulate_point
constexpr int SOLVE_RETRIES = 8;
constexpr int MAX_K = 12;                   // unknowns of a rolling-shutter frame
constexpr int GS = 16;                      // row stride of the Gram matrix of [J | r]: one 16 x 16 tile
constexpr int MAX_CANDIDATES = 4;
constexpr int MIN_STATIC = 3, MIN_ROLLING = 6;   // usable observations below which a frame is TOO_FEW

// the record of one camera: camera_entry (spare slots as in mcba_triangulate.h: CAM_HEIGHT, CAM_ISFISH, REC_ND) | camera pose 3 x 4
constexpr int REC_POSE = CAM_STRIDE, REC_STRIDE = CAM_STRIDE + 12;
using triangulate::REC_ND;

MCBA_HD constexpr int n_unknowns(bool rolling) { return rolling ? 12 : 6; }
MCBA_HD constexpr int n_cov(int K) { return K * (K + 1) / 2; }
MCBA_HD int min_observations(bool rolling) { return rolling ? MIN_ROLLING : MIN_STATIC; }
MCBA_HD int clamp_iterations(int max_iterations) { return triangulate::clamp_iterations(max_iterations); }

// the usable observations of one frame, compacted: pixel, camera and world point of each
struct FrameObs {
  const double* uv;        // [n][2]
  const int32_t* cam;      // [n]
  const int32_t* wpt;      // [n] index into W
  const double* W;         // [B P][3] board_pose[b] X[b,p]
  int n;
};

// ---------------------------------------------------------------------------------------------------------
// rigid 3 x 4 helpers (row-major [R | t])
// ---------------------------------------------------------------------------------------------------------
MCBA_HD void rigid_inverse(const double* M, double* out) {
  MCBA_UNROLL
  for (int r = 0; r < 3; ++r) {
    MCBA_UNROLL
    for (int c = 0; c < 3; ++c) out[4 * r + c] = M[4 * c + r];
    out[4 * r + 3] = -(M[r] * M[3] + M[4 + r] * M[7] + M[8 + r] * M[11]);
  }
}
MCBA_HD void rigid_mul(const double* A, const double* B, double* out) {
  MCBA_UNROLL
  for (int r = 0; r < 3; ++r) {
    MCBA_UNROLL
    for (int c = 0; c < 4; ++c)
      out[4 * r + c] = A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c] + A[4 * r + 2] * B[8 + c] + (c == 3 ? A[4 * r + 3] : 0.0);
  }
}
// rig candidate of one view: camera_pose^-1 . T_view . board_pose^-1 as a row-major 4 x 4 (cam_inv, board_inv: the inverses, 3 x 4)
MCBA_HD void view_candidate(const double* cam_inv, const double* view_pose16, const double* board_inv, double* pose16) {
  double T[12], U[12];
  rigid_mul(cam_inv, view_pose16, T);     // (the top three rows of a row-major 4 x 4 are a row-major 3 x 4)
  rigid_mul(T, board_inv, U);
  MCBA_UNROLL
  for (int i = 0; i < 12; ++i) pose16[i] = U[i];
  pose16[12] = pose16[13] = pose16[14] = 0.0;
  pose16[15] = 1.0;
}

// up to MAX_CANDIDATES views of a frame: status OK, most corners first, ties to the earlier view (the list is in (c, b) order)
MCBA_HD int select_views(int n_views, const uint8_t* status, const int32_t* n_used, int* picks) {
  int n = 0;
  MCBA_NOUNROLL
  for (int k = 0; k < MAX_CANDIDATES; ++k) {
    int best = -1;
    MCBA_NOUNROLL
    for (int v = 0; v < n_views; ++v) {
      if (status[v] != (uint8_t)pnp::ST_OK) continue;
      bool taken = false;
      for (int j = 0; j < n; ++j) taken = taken || picks[j] == v;
      if (taken) continue;
      if (best < 0 || n_used[v] > n_used[best]) best = v;
    }
    if (best < 0) break;
    picks[n++] = best;
  }
  return n;
}

// ---------------------------------------------------------------------------------------------------------
// per observation.  pe: the frame's pose entries (mcba_math.h: pose_entry, R | t | L), start and -- rolling -- end
// ---------------------------------------------------------------------------------------------------------
// camera-frame point; Xr0, Xr1 = R_start W, R_end W; s = lerp weights (1 - t, t)
template <bool ROLLING>
MCBA_HD void obs_point(const double* rec, const double* pe, const double* W, double v, double* Xr0, double* Xr1, double* s, double* Xc) {
  mat3_vec(pe + POSE_R, W, Xr0);
  double Xg[3] = {Xr0[0] + pe[POSE_T], Xr0[1] + pe[POSE_T + 1], Xr0[2] + pe[POSE_T + 2]};
  s[0] = 1.0;
  s[1] = 0.0;
  if constexpr (ROLLING) {
    const double* pq = pe + POSE_STRIDE;
    const double t = v / rec[CAM_HEIGHT];
    s[0] = 1.0 - t;
    s[1] = t;
    mat3_vec(pq + POSE_R, W, Xr1);
    MCBA_UNROLL
    for (int i = 0; i < 3; ++i) Xg[i] = s[0] * Xg[i] + s[1] * (Xr1[i] + pq[POSE_T + i]);
  }
  triangulate::transform(rec + REC_POSE, Xg, Xc);
}

// the two rows [J | r] of one observation: K + 1 entries each
template <bool ROLLING>
MCBA_HD void obs_rows(const double* rec, const double* pe, const double* W, double u, double v, double* ru, double* rv) {
  constexpr int K = ROLLING ? 12 : 6;
  double Xr0[3], Xr1[3], s[2], Xc[3], uv[2], A[6], Ar[6], E[12];
  obs_point<ROLLING>(rec, pe, W, v, Xr0, Xr1, s, Xc);
  triangulate::project_jac(rec, Xc, uv, A);
  const double* M = rec + REC_POSE;
  MCBA_UNROLL
  for (int k = 0; k < 2; ++k) {
    MCBA_UNROLL
    for (int j = 0; j < 3; ++j) Ar[3 * k + j] = A[3 * k] * M[j] + A[3 * k + 1] * M[4 + j] + A[3 * k + 2] * M[8 + j];
  }
  MCBA_UNROLL
  for (int e = 0; e < (ROLLING ? 2 : 1); ++e) {
    const double* L = pe + e * POSE_STRIDE + POSE_L;
    const double w = s[e];
    base_rows(Ar, e == 0 ? Xr0 : Xr1, E);
    MCBA_UNROLL
    for (int c = 0; c < 3; ++c) {
      ru[6 * e + c] = w * (E[0] * L[c] + E[1] * L[3 + c] + E[2] * L[6 + c]);
      rv[6 * e + c] = w * (E[6] * L[c] + E[7] * L[3 + c] + E[8] * L[6 + c]);
      ru[6 * e + 3 + c] = w * E[3 + c];
      rv[6 * e + 3 + c] = w * E[9 + c];
    }
  }
  ru[K] = uv[0] - u;
  rv[K] = uv[1] - v;
}

// squared pixel error of one observation; *behind: the point is at or behind its camera
template <bool ROLLING>
MCBA_HD double obs_sq(const double* rec, const double* pe, const double* W, double u, double v, bool* behind) {
  double Xr0[3], Xr1[3], s[2], Xc[3], uv[2];
  obs_point<ROLLING>(rec, pe, W, v, Xr0, Xr1, s, Xc);
  undistort::project_any(rec, (int)rec[REC_ND], rec[CAM_ISFISH] != 0.0, Xc, uv);
  *behind = !(Xc[2] > 0.0);
  return (uv[0] - u) * (uv[0] - u) + (uv[1] - v) * (uv[1] - v);
}

// what a start candidate pays for one observation: the squared error, or the squared image diagonal (as the principal point states
// it: 4 (cx^2 + cy^2)) for a point at or behind its camera or an error that is not finite
MCBA_HD double candidate_term(const double* rec, const double* pe, const double* W, double u, double v) {
  bool behind;
  const double e = obs_sq<false>(rec, pe, W, u, v, &behind);
  const double diag2 = 4.0 * (rec[CAM_CX] * rec[CAM_CX] + rec[CAM_CY] * rec[CAM_CY]);
  return (behind || !(e < 1e300)) ? diag2 : e;
}

// pose entry of a row-major 4 x 4 (and its six parameters)
MCBA_HD void pose_to_entry(const double* pose16, double* p6, double* entry) {
  intr::pose_to_params(pose16, p6);
  pose_entry(p6, entry);
}

// score of one candidate pose over a whole frame, observations in record order (the host's order; the device's is its own)
MCBA_HD double candidate_score(const double* recs, const FrameObs& o, const double* pose16) {
  double p[6], pe[POSE_STRIDE], s = 0.0;
  pose_to_entry(pose16, p, pe);
  MCBA_NOUNROLL
  for (int i = 0; i < o.n; ++i)
    s += candidate_term(recs + (size_t)o.cam[i] * REC_STRIDE, pe, o.W + 3 * (size_t)o.wpt[i], o.uv[2 * i], o.uv[2 * i + 1]);
  return s;
}
// the candidate a frame starts from: lowest score, ties to the earlier one; -1: none has a finite score
MCBA_HD int pick_candidate(const double* scores, int n) {
  int best = -1;
  for (int k = 0; k < n; ++k)
    if (scores[k] < 1e300 && (best < 0 || scores[k] < scores[best])) best = k;
  return best;
}

// ---------------------------------------------------------------------------------------------------------
// small dense algebra of one frame: G = Gram matrix of [J | r] (stride GS, upper triangle read), A = K x K scratch (stride MAX_K)
// ---------------------------------------------------------------------------------------------------------
MCBA_HD double gsym(const double* G, int i, int j) { return i <= j ? G[i * GS + j] : G[j * GS + i]; }

// Cholesky factor in place (lower triangle of A); a squared pivot at or below min_pivot counts as vanished
MCBA_HD bool chol_factor(int K, double* A, double min_pivot) {
  for (int j = 0; j < K; ++j) {
    double d = A[j * MAX_K + j];
    for (int k = 0; k < j; ++k) d -= A[j * MAX_K + k] * A[j * MAX_K + k];
    if (!(d > min_pivot)) return false;
    const double l = sqrt(d);
    A[j * MAX_K + j] = l;
    for (int i = j + 1; i < K; ++i) {
      double s = A[i * MAX_K + j];
      for (int k = 0; k < j; ++k) s -= A[i * MAX_K + k] * A[j * MAX_K + k];
      A[i * MAX_K + j] = s / l;
    }
  }
  return true;
}
MCBA_HD void chol_solve(int K, const double* A, double* b) {
  for (int i = 0; i < K; ++i) {
    double s = b[i];
    for (int k = 0; k < i; ++k) s -= A[i * MAX_K + k] * b[k];
    b[i] = s / A[i * MAX_K + i];
  }
  for (int i = K - 1; i >= 0; --i) {
    double s = b[i];
    for (int k = i + 1; k < K; ++k) s -= A[k * MAX_K + i] * b[k];
    b[i] = s / A[i * MAX_K + i];
  }
}

// the frame is well posed at this linearisation: every pivot of the factor of the scaled matrix D^-1/2 H D^-1/2 stands clear of 0
MCBA_HD bool well_posed(int K, const double* G, double* A) {
  double is[MAX_K];
  for (int i = 0; i < K; ++i) {
    const double d = G[i * GS + i];
    if (!(d > 0.0) || !(d < 1e300)) return false;
    is[i] = 1.0 / sqrt(d);
  }
  for (int i = 0; i < K; ++i)
    for (int j = 0; j <= i; ++j) A[i * MAX_K + j] = gsym(G, i, j) * is[i] * is[j];
  return chol_factor(K, A, PIVOT_FLOOR);
}

// step of (H + lambda diag H) d = -g; *whitened = sqrt(d^T H d).  false: the damped matrix is not positive definite
MCBA_HD bool damped_step(int K, const double* G, double lambda, double* A, double* d, double* whitened) {
  for (int i = 0; i < K; ++i) {
    for (int j = 0; j < i; ++j) A[i * MAX_K + j] = gsym(G, i, j);
    A[i * MAX_K + i] = G[i * GS + i] * (1.0 + lambda);
    d[i] = -G[i * GS + K];
  }
  if (!chol_factor(K, A, 0.0)) return false;
  chol_solve(K, A, d);
  double q = 0.0;
  for (int i = 0; i < K; ++i)
    for (int j = 0; j < K; ++j) q += d[i] * gsym(G, i, j) * d[j];
  *whitened = sqrt(fmax(q, 0.0));
  return *whitened < 1e300;
}

// cov [K (K + 1) / 2] = upper triangle by rows of sigma2 H^-1; false (cov untouched): H is not positive definite
MCBA_HD bool covariance(int K, const double* G, double sigma2, double* A, double* cov) {
  for (int i = 0; i < K; ++i)
    for (int j = 0; j <= i; ++j) A[i * MAX_K + j] = gsym(G, i, j);
  if (!chol_factor(K, A, 0.0)) return false;
  double x[MAX_K];
  for (int j = 0; j < K; ++j) {
    for (int i = 0; i < K; ++i) x[i] = i == j ? 1.0 : 0.0;
    chol_solve(K, A, x);
    for (int i = 0; i <= j; ++i) cov[i * K - i * (i - 1) / 2 + (j - i)] = sigma2 * x[i];
  }
  return true;
}

// variance of a pixel coordinate behind the covariance: the given one, or the frame's own sse / (2 n - K) (NaN without a surplus)
MCBA_HD double pixel_variance(double sigma_px, double sse, int n, int K) {
  if (sigma_px > 0.0) return sigma_px * sigma_px;
  return 2 * n > K ? sse / (double)(2 * n - K) : undistort::quiet_nan();
}

// ---------------------------------------------------------------------------------------------------------
// Levenberg-Marquardt over one frame through a back-end BE.  The current point is set by the caller (be.start).
//   double linearize()                    Gram matrix at the current point; returns the cost
//   bool   well_posed()                   the scaled factor of that matrix has no vanishing pivot
//   bool   solve(lambda, *whitened)       trial point = current + step; false: not positive definite
//   double trial_cost()                   cost at the trial point (residual-only pass)
//   void   accept()                       current point <- trial point
// max_iter: linearisations, already clamped.  *have: the start had a finite cost and was well posed; *iters: linearisations used.
// ---------------------------------------------------------------------------------------------------------
template <class BE>
MCBA_HD bool solve_frame(BE& be, int n, int max_iter, bool* have, int* iters, double* cost_out) {
  double cost = be.linearize();
  int used = 1;
  *iters = used;
  *cost_out = 0.0;
  *have = cost < 1e300 && be.well_posed();
  if (!*have) return false;
  bool converged = false;
  double lambda = 1e-3;
  const int max_rounds = 2 * max_iter + SOLVE_RETRIES;   // (a run of rejected trials costs no linearisation: bounded on its own)
  MCBA_NOUNROLL
  for (int round = 0; round < max_rounds; ++round) {
    double whitened = 0.0;
    bool solved = false;
    MCBA_NOUNROLL
    for (int k = 0; k < SOLVE_RETRIES && !solved; ++k) {
      solved = be.solve(lambda, &whitened);
      if (!solved) lambda = lambda * 10.0 + 1e-12;
    }
    if (!solved) break;
    const double cq = be.trial_cost();
    // (the slack of triangulate_point: a trial within the rounding of the residuals counts as a descent)
    const bool accept = cq <= cost * (1.0 + pnp::LM_ACCEPT_SLACK) + 2.0 * sqrt(cost * (double)(2 * n)) * RESIDUAL_ROUNDING + STOP_PX * STOP_PX;
    if (!accept) {
      lambda = fmin(lambda * 10.0, 1e30);
      continue;
    }
    be.accept();
    cost = cq;
    lambda = fmax(lambda * 0.1, 1e-15);
    if (whitened <= STOP_PX) { converged = true; break; }
    if (used >= max_iter) break;
    const double cl = be.linearize();
    ++used;
    if (!(cl < 1e300) || !be.well_posed()) { *have = false; break; }
    cost = cl;
  }
  *iters = used;
  *cost_out = cost;
  return converged;
}

struct FrameResult {
  double pose[16], pose_end[16], cov[MAX_K * (MAX_K + 1) / 2], sse;
  int iters, status;
};

// what a frame without a result returns: identity poses, sse 0, NaN covariance
MCBA_HD void no_result(int K, int status, int iters, FrameResult& out) {
  pnp::identity_pose(out.pose);
  pnp::identity_pose(out.pose_end);
  for (int i = 0; i < n_cov(K); ++i) out.cov[i] = undistort::quiet_nan();
  out.sse = 0.0;
  out.iters = iters;
  out.status = status;
}

// ---------------------------------------------------------------------------------------------------------
// the plain-loop back-end: observations in record order
// ---------------------------------------------------------------------------------------------------------
template <bool ROLLING>
struct SerialBackend {
  static constexpr int K = ROLLING ? 12 : 6;
  const double* recs;
  FrameObs o;
  double p[MAX_K], q[MAX_K], pe[2 * POSE_STRIDE], qe[2 * POSE_STRIDE], G[GS * GS], A[MAX_K * MAX_K];

  void entries(const double* x, double* e) {
    pose_entry(x, e);
    if (ROLLING) pose_entry(x + 6, e + POSE_STRIDE);
  }
  void start(const double* x) {
    for (int i = 0; i < K; ++i) p[i] = x[i];
    entries(p, pe);
  }
  double linearize() {
    for (int i = 0; i < GS * GS; ++i) G[i] = 0.0;
    for (int i = 0; i < o.n; ++i) {
      double ru[K + 1], rv[K + 1];
      obs_rows<ROLLING>(recs + (size_t)o.cam[i] * REC_STRIDE, pe, o.W + 3 * (size_t)o.wpt[i], o.uv[2 * i], o.uv[2 * i + 1], ru, rv);
      for (int a = 0; a <= K; ++a)
        for (int b = a; b <= K; ++b) G[a * GS + b] += ru[a] * ru[b] + rv[a] * rv[b];
    }
    return G[K * GS + K];
  }
  bool well_posed() { return localize::well_posed(K, G, A); }
  bool solve(double lambda, double* whitened) {
    double d[MAX_K];
    if (!damped_step(K, G, lambda, A, d, whitened)) return false;
    for (int i = 0; i < K; ++i) q[i] = p[i] + d[i];
    entries(q, qe);
    return true;
  }
  double cost_at(const double* e, bool* behind, double* err) {
    double s = 0.0;
    *behind = false;
    for (int i = 0; i < o.n; ++i) {
      bool b;
      const double t = obs_sq<ROLLING>(recs + (size_t)o.cam[i] * REC_STRIDE, e, o.W + 3 * (size_t)o.wpt[i], o.uv[2 * i], o.uv[2 * i + 1], &b);
      s += t;
      *behind = *behind || b;
      if (err) err[i] = sqrt(t);
    }
    return s;
  }
  double trial_cost() {
    bool b;
    return cost_at(qe, &b, nullptr);
  }
  void accept() {
    for (int i = 0; i < K; ++i) p[i] = q[i];
    for (int i = 0; i < 2 * POSE_STRIDE; ++i) pe[i] = qe[i];
  }
};

// one frame on the host.  start16 / start_end16: the start poses (row-major 4 x 4; the end is read for rolling shutter only), or
// null: the frame has no start.  err [n] (or null): per-record reprojection error, 0 without a result.
template <bool ROLLING>
inline void localize_frame(const double* recs, const FrameObs& o, const double* start16, const double* start_end16, double sigma_px,
                           int max_iter, double* err, FrameResult& out) {
  constexpr int K = ROLLING ? 12 : 6;
  if (err)
    for (int i = 0; i < o.n; ++i) err[i] = 0.0;
  if (o.n < min_observations(ROLLING)) return no_result(K, ST_TOO_FEW, 0, out);
  if (!start16) return no_result(K, ST_DEGENERATE, 0, out);
  SerialBackend<ROLLING> be;
  be.recs = recs;
  be.o = o;
  double x[MAX_K];
  intr::pose_to_params(start16, x);
  if (ROLLING) intr::pose_to_params(start_end16, x + 6);
  be.start(x);
  bool have = false;
  int iters = 0;
  double cost = 0.0;
  const bool converged = solve_frame(be, o.n, max_iter, &have, &iters, &cost);
  if (!have) return no_result(K, ST_DEGENERATE, iters, out);
  bool behind = false;
  out.sse = be.cost_at(be.pe, &behind, err);
  intr::params_to_pose(be.p, out.pose);
  if (ROLLING) intr::params_to_pose(be.p + 6, out.pose_end);
  else pnp::identity_pose(out.pose_end);
  for (int i = 0; i < n_cov(K); ++i) out.cov[i] = undistort::quiet_nan();
  covariance(K, be.G, pixel_variance(sigma_px, out.sse, o.n, K), be.A, out.cov);
  out.iters = iters;
  out.status = behind ? ST_BEHIND : converged ? ST_OK : ST_NOT_CONVERGED;
}

}  // namespace localize
}  // namespace mcba
