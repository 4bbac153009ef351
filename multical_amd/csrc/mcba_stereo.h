// mcba_stereo.h -- stereo calibration of camera pairs with the cameras held (FP64 throughout).
//
// Restates stereo_calibrate / stereo_calibrate_fisheye (camera.py:261-286, camera_fisheye.py:180-200: cv2.stereoCalibrate with
// CALIB_FIX_INTRINSIC) for a batch of independent pairs (l, r) of one detection table.  Unknowns of a pair: T_rel (left-camera
// frame -> right-camera frame, X_r = R X_l + T) and one board pose T_v (board -> left camera) per usable view; all of them in the
// project's parameterisation of a pose block: GLOBAL rotation vector, then translation, d(R(w) y)/dw = -[R y]x L(w).
//   view         a (frame, board) slot in which both cameras have a valid start pose and at least min_common corners are valid in
//                both cameras and in board_valid; only those common corners enter (tables.matching_points' rule).  A slot whose
//                common corners lie on one line (the overlap of two images can be one column of a board) leaves the rotation
//                about that line free: the driver drops it (mcba_stereo_driver.h: collinear_view); a pair that has nothing
//                else is DEGENERATE;
//   cost         sum |project_l(T_v X) - p_l|^2 + |project_r(T_rel T_v X) - p_r|^2 in pixels, the runtime-dispatched projection of
//                mcba_triangulate.h: a pair may mix camera families;
//   rows         four per corner, 13 columns [rel (6) | view (6) | r]; the left rows have zeros in the rel columns;
//                dX_r/drel = (-[R_rel X_l]x L_rel | I), dX_r/dview = R_rel (-[R_v X]x L_v | I);
//   start        T_v = the left camera's start pose of the view; T_rel = the best of up to four candidates T_{r,v} T_{l,v}^-1 from
//                the views with the most common corners, scored by the residual-only cost over ALL the pair's views, a point at or
//                behind a camera counting as the squared image diagonal (mcba_localize.h's rule: one planar flip is outvoted);
//   refinement   intr::lm_loop (accept / reject policy, Marquardt scaling, LM_STEP_TOL).  One linearisation = per view the 16 x 16
//                Gram matrix of the rows, the view eliminated by its damped 6 x 6 block (Schur complement), the reduced 6 x 6
//                system solved by Cholesky, the views back-substituted, the trial cost from a residual-only pass;
//   results      cov = sigma^2 (H_rr - sum_v S_v)^-1 at lambda = 0, linearised again at the returned point; sigma^2 = sse /
//                (4 n_points - 6 - 6 n_views), or sigma_px^2 when given; a non-positive degree of freedom: NaN;
//   degenerate   at lambda = 0 every pivot of the factor of the scaled blocks D^-1/2 H_vv D^-1/2 and of the scaled reduced matrix must
//                stand clear of 0 (PIVOT_FLOOR): what the drop of collinear views lets through (corners that are nearly on a line).
// Rolling shutter and free intrinsics are out of scope: the model is cv2's static one with the cameras held.
// Everything is MCBA_HD: k_stereo_pair (mcba_stereo_kernels.h) runs one pair per workgroup, tests/stereo_host builds the same
// source with g++.  The loop is written against a BACK-END as in mcba_intrinsic.h and mcba_localize.h; SerialBackend below is the
// plain-loop one, with a switch for the device's summation order.
#pragma once
#include <stdint.h>
#include "mcba_localize.h"

namespace mcba {
namespace stereo {

constexpr int ST_OK = 0, ST_TOO_FEW = 1, ST_DEGENERATE = 2, ST_NOT_CONVERGED = 3;   // mcba.h: MCBA_STEREO_*
constexpr int DEFAULT_MIN_COMMON = pnp::MIN_CORNERS, MIN_MIN_COMMON = 3;
constexpr int DEFAULT_ITERATIONS = 100, MAX_ITERATIONS = 1000;   // passes of intr::lm_loop
constexpr int NV = 13;                      // columns of a row: rel | view | r
constexpr int GS = localize::GS;            // row stride of a view's Gram matrix: one 16 x 16 tile
constexpr int MAX_CANDIDATES = localize::MAX_CANDIDATES;
constexpr double PIVOT_FLOOR = localize::PIVOT_FLOOR;
constexpr int WAVES = 4;                    // wave partials of the device's summation order

// per-view block of the workspace (doubles)
constexpr int VB_HVV = 0;                   // [6][6] J_v^T J_v
constexpr int VB_HVR = 36;                  // [6][6] J_v^T J_rel
constexpr int VB_GV = 72;                   // [6]    J_v^T r
constexpr int VB_W = 78;                    // [6][7] (H_vv + lambda D_v)^-1 [H_vr | g_v]
constexpr int VB_P = 120;                   // [6] pose
constexpr int VB_Q = 126;                   // [6] trial pose
constexpr int VB_SSE = 132;                 // [2] cost of the view at the trial point: left | right
constexpr int VB_STRIDE = 134;
constexpr int WS = 7;                       // row stride of W
constexpr int N_PAIR_SUMS = 43;             // H_rr [36] | g_r [6] | cost
constexpr int N_SCHUR = 42;                 // [6][7]: S_v | its right-hand side
constexpr int N_VIEW_ENTRIES = 78;          // H_vv, H_vr, g_v
constexpr int PART = 44;                    // a wave partial of either

MCBA_HD int clamp_iterations(int max_iterations) {
  return max_iterations <= 0 ? DEFAULT_ITERATIONS : (max_iterations > MAX_ITERATIONS ? MAX_ITERATIONS : max_iterations);
}

// what the back-ends read: the call's tables (camera records: camera_entry with CAM_ISFISH and triangulate::REC_ND filled in)
struct Tables {
  int F, B, P;
  const double* recs;          // [C][CAM_STRIDE]
  const double* board;         // [B][P][3]
  const uint8_t* board_valid;  // [B][P] or null
  const double* points;        // [C,F,B,P,2]
  const uint8_t* valid;        // [C,F,B,P]
  const double* view_poses;    // [C,F,B,16] start poses board -> camera
};
// one pair: its cameras and its views ((frame, board) slots f B + b, table order) with their common-corner counts and blocks
struct PairViews {
  int l, r, nv;
  const int32_t* slot;         // [nv]
  const int32_t* n_common;     // [nv]
  double* ws;                  // [nv][VB_STRIDE]
};

MCBA_HD bool finite2(const double* p) { return p[0] - p[0] == 0.0 && p[1] - p[1] == 0.0; }
// corner j of slot (f, b) enters the pair: valid in both cameras and on the board, both pixels finite.  rowl / rowr: index of
// the slot's first corner in [C,F,B,P]
MCBA_HD bool common_corner(const Tables& t, size_t rowl, size_t rowr, int b, int j) {
  if (!t.valid[rowl + j] || !t.valid[rowr + j]) return false;
  if (t.board_valid && !t.board_valid[(size_t)b * t.P + j]) return false;
  return finite2(t.points + 2 * (rowl + j)) && finite2(t.points + 2 * (rowr + j));
}
MCBA_HD size_t slot_row(const Tables& t, int c, int slot) { return ((size_t)c * t.F * t.B + (size_t)slot) * t.P; }

// ---------------------------------------------------------------------------------------------------------
// per corner.  ve, re: pose entries (mcba_math.h: pose_entry, R | t | L) of the view and of T_rel
// ---------------------------------------------------------------------------------------------------------
// camera-frame point of side s (0: left, 1: right); Xr = R_v X, Y = R_rel X_l (right only)
MCBA_HD void corner_point(int side, const double* ve, const double* re, const double* X, double* Xr, double* Y, double* Xc) {
  mat3_vec(ve + POSE_R, X, Xr);
  MCBA_UNROLL
  for (int i = 0; i < 3; ++i) Xc[i] = Xr[i] + ve[POSE_T + i];
  if (side != 0) {
    mat3_vec(re + POSE_R, Xc, Y);
    MCBA_UNROLL
    for (int i = 0; i < 3; ++i) Xc[i] = Y[i] + re[POSE_T + i];
  }
}

// the two rows [rel | view | r] of one corner in the camera of side s (rec: that camera's record): NV entries each
MCBA_HD void corner_rows(int side, const double* rec, const double* ve, const double* re, const double* X, double u, double v,
                         double* ru, double* rv) {
  double Xr[3], Y[3], Xc[3], uv[2], A[6], E[12];
  corner_point(side, ve, re, X, Xr, Y, Xc);
  triangulate::project_jac(rec, Xc, uv, A);
  const double* L = ve + POSE_L;
  if (side == 0) {
    MCBA_UNROLL
    for (int c = 0; c < 6; ++c) ru[c] = rv[c] = 0.0;
  } else {
    const double* Lr = re + POSE_L;
    const double* R = re + POSE_R;
    base_rows(A, Y, E);
    MCBA_UNROLL
    for (int c = 0; c < 3; ++c) {
      ru[c] = E[0] * Lr[c] + E[1] * Lr[3 + c] + E[2] * Lr[6 + c];
      rv[c] = E[6] * Lr[c] + E[7] * Lr[3 + c] + E[8] * Lr[6 + c];
      ru[3 + c] = E[3 + c];
      rv[3 + c] = E[9 + c];
    }
    double Ar[6];
    MCBA_UNROLL
    for (int k = 0; k < 2; ++k) {
      MCBA_UNROLL
      for (int j = 0; j < 3; ++j) Ar[3 * k + j] = A[3 * k] * R[j] + A[3 * k + 1] * R[3 + j] + A[3 * k + 2] * R[6 + j];
    }
    MCBA_UNROLL
    for (int i = 0; i < 6; ++i) A[i] = Ar[i];
  }
  base_rows(A, Xr, E);
  MCBA_UNROLL
  for (int c = 0; c < 3; ++c) {
    ru[6 + c] = E[0] * L[c] + E[1] * L[3 + c] + E[2] * L[6 + c];
    rv[6 + c] = E[6] * L[c] + E[7] * L[3 + c] + E[8] * L[6 + c];
    ru[9 + c] = E[3 + c];
    rv[9 + c] = E[9 + c];
  }
  ru[12] = uv[0] - u;
  rv[12] = uv[1] - v;
}

// squared pixel error of one corner in the camera of side s.  SCORE: what a start candidate pays -- the squared image diagonal
// (as the principal point states it: 4 (cx^2 + cy^2)) for a point at or behind the camera or an error that is not finite
template <bool SCORE>
MCBA_HD double corner_sq(int side, const double* rec, const double* ve, const double* re, const double* X, double u, double v) {
  double Xr[3], Y[3], Xc[3], uv[2];
  corner_point(side, ve, re, X, Xr, Y, Xc);
  undistort::project_any(rec, (int)rec[triangulate::REC_ND], rec[CAM_ISFISH] != 0.0, Xc, uv);
  const double e = (uv[0] - u) * (uv[0] - u) + (uv[1] - v) * (uv[1] - v);
  if (SCORE) {
    const double diag2 = 4.0 * (rec[CAM_CX] * rec[CAM_CX] + rec[CAM_CY] * rec[CAM_CY]);
    return (!(Xc[2] > 0.0) || !(e < 1e300)) ? diag2 : e;
  }
  return e;
}

// ---------------------------------------------------------------------------------------------------------
// per view, entry by entry (the back-end spreads the entries over its lanes).  G: the view's Gram matrix, upper triangle
// ---------------------------------------------------------------------------------------------------------
using localize::gsym;
// entries of the pair's sums a view contributes: H_rr, then g_r, then the cost
MCBA_HD double pair_sum_entry(const double* G, int e) {
  if (e < 36) return gsym(G, e / 6, e % 6);
  if (e < 42) return gsym(G, e - 36, 12);
  return G[12 * GS + 12];
}
// entries of the view's own blocks
MCBA_HD void view_entry(const double* G, int e, double* vb) {
  if (e < 36) vb[VB_HVV + e] = gsym(G, 6 + e / 6, 6 + e % 6);
  else if (e < 72) vb[VB_HVR + (e - 36)] = gsym(G, (e - 36) % 6, 6 + (e - 36) / 6);
  else vb[VB_GV + (e - 72)] = gsym(G, 6 + (e - 72), 12);
}
// column j <= 6 of W = (H_vv + lambda D_v)^-1 [H_vr | g_v], through the factor of the scaled block D^-1/2 (.) D^-1/2 whose squared
// pivots must exceed `floor`; false: they do not (at lambda = 0: the view does not fix its own pose)
MCBA_HD bool view_w_column(double* vb, double lambda, int j, double floor) {
  double M[36], is[6], rhs[6], out[6];
  bool ok = true;
  MCBA_UNROLL
  for (int k = 0; k < 6; ++k) {
    const double d = vb[VB_HVV + 7 * k];
    ok = ok && d > 0.0 && d < 1e300;
    is[k] = ok ? 1.0 / sqrt(d) : 1.0;
  }
  if (!ok) return false;
  MCBA_UNROLL
  for (int a = 0; a < 6; ++a) {
    MCBA_UNROLL
    for (int b = 0; b < 6; ++b) M[6 * a + b] = a == b ? 1.0 + lambda : vb[VB_HVV + 6 * a + b] * is[a] * is[b];
    rhs[a] = (j < 6 ? vb[VB_HVR + 6 * a + (j < 6 ? j : 0)] : vb[VB_GV + a]) * is[a];
  }
  if (!pnp::chol6_solve(M, rhs, out, floor)) return false;
  MCBA_UNROLL
  for (int k = 0; k < 6; ++k) vb[VB_W + k * WS + j] = out[k] * is[k];
  return true;
}
// entry e = i 7 + j of H_rv W: columns j < 6 the Schur complement S_v, column 6 its right-hand side
MCBA_HD double view_schur_entry(const double* vb, int e) {
  const int i = e / WS, j = e % WS;
  double s = 0.0;
  MCBA_UNROLL
  for (int k = 0; k < 6; ++k) s += vb[VB_HVR + 6 * k + i] * vb[VB_W + k * WS + j];
  return s;
}
// back-substitution: q = p - W [delta_rel ; 1]; adds the view's part of the scaled step and parameter norms
MCBA_HD void view_backsub(double* vb, const double* di, double* dn, double* pn) {
  MCBA_NOUNROLL
  for (int k = 0; k < 6; ++k) {
    double s = vb[VB_W + k * WS + 6];
    for (int i = 0; i < 6; ++i) s += vb[VB_W + k * WS + i] * di[i];
    const double p = vb[VB_P + k], d = vb[VB_HVV + 7 * k];
    vb[VB_Q + k] = p - s;
    *dn += d * s * s;
    *pn += d * p * p;
  }
}

// ---------------------------------------------------------------------------------------------------------
// per pair.  hs [N_PAIR_SUMS]: the pair's sums; ss [N_SCHUR]: the Schur sums
// ---------------------------------------------------------------------------------------------------------
// the scaled reduced matrix D^-1/2 (H_rr + lambda D - S) D^-1/2 and the scale; false: a diagonal entry of H_rr is not positive
MCBA_HD bool reduced_matrix(const double* hs, const double* ss, double lambda, double* M, double* is) {
  for (int i = 0; i < 6; ++i) {
    const double d = hs[7 * i];
    if (!(d > 0.0) || !(d < 1e300)) return false;
    is[i] = 1.0 / sqrt(d);
  }
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      // (S is summed entry by entry: its two triangles agree to rounding only; the factor reads the lower one)
      const double h = (i == j ? hs[7 * i] * (1.0 + lambda) : hs[6 * i + j]) - ss[i * WS + j];
      M[6 * i + j] = h * is[i] * is[j];
    }
  return true;
}
// reduced system (H_rr + lambda D - S) delta = -(g_r - s): p -> trial q; the pair's part of the step norms
MCBA_HD bool reduced_solve(const double* hs, const double* ss, double lambda, double* di, const double* p, double* q, double* dn,
                           double* pn) {
  double M[36], is[6], rhs[6], out[6];
  if (!reduced_matrix(hs, ss, lambda, M, is)) return false;
  for (int i = 0; i < 6; ++i) rhs[i] = -(hs[36 + i] - ss[i * WS + 6]) * is[i];
  if (!pnp::chol6_solve(M, rhs, out, 0.0)) return false;
  for (int i = 0; i < 6; ++i) {
    di[i] = out[i] * is[i];
    q[i] = p[i] + di[i];
    *dn += hs[7 * i] * di[i] * di[i];
    *pn += hs[7 * i] * p[i] * p[i];
  }
  return true;
}
// inv [36] = (H_rr - S)^-1 from the sums at lambda = 0; false: a pivot of the scaled factor does not stand clear of 0
MCBA_HD bool reduced_inverse(const double* hs, const double* ss, double* inv) {
  double M[36], is[6], rhs[6], out[6];
  if (!reduced_matrix(hs, ss, 0.0, M, is)) return false;
  for (int j = 0; j < 6; ++j) {
    for (int i = 0; i < 6; ++i) rhs[i] = i == j ? 1.0 : 0.0;
    if (!pnp::chol6_solve(M, rhs, out, PIVOT_FLOOR)) return false;
    for (int i = 0; i < 6; ++i) inv[6 * i + j] = out[i] * is[i] * is[j];
  }
  return true;
}

// variance of a pixel coordinate behind the covariance: the given one, or the pair's own sse / (4 n_points - 6 - 6 n_views)
MCBA_HD double pixel_variance(double sigma_px, double sse, int n_points, int n_views) {
  if (sigma_px > 0.0) return sigma_px * sigma_px;
  const int dof = 4 * n_points - 6 - 6 * n_views;
  return dof > 0 ? sse / (double)dof : undistort::quiet_nan();
}

// up to MAX_CANDIDATES views of a pair: most common corners first, ties to the earlier view
MCBA_HD int select_views(int nv, const int32_t* n_common, int* picks) {
  int n = 0;
  MCBA_NOUNROLL
  for (int k = 0; k < MAX_CANDIDATES; ++k) {
    int best = -1;
    MCBA_NOUNROLL
    for (int v = 0; v < nv; ++v) {
      bool taken = false;
      for (int j = 0; j < n; ++j) taken = taken || picks[j] == v;
      if (taken) continue;
      if (best < 0 || n_common[v] > n_common[best]) best = v;
    }
    if (best < 0) break;
    picks[n++] = best;
  }
  return n;
}
// the six parameters of the candidate T_{r,v} T_{l,v}^-1 of one view (row-major 4 x 4 start poses)
MCBA_HD void candidate_params(const double* pose_l, const double* pose_r, double* p6) {
  double inv[12], T[12], pose[16];
  localize::rigid_inverse(pose_l, inv);
  localize::rigid_mul(pose_r, inv, T);
  MCBA_UNROLL
  for (int i = 0; i < 12; ++i) pose[i] = T[i];
  pose[12] = pose[13] = pose[14] = 0.0;
  pose[15] = 1.0;
  intr::pose_to_params(pose, p6);
}

// ---------------------------------------------------------------------------------------------------------
// one pair through a back-end BE.  On top of what intr::lm_loop asks for:
//   bool start()            view poses <- the left camera's start poses, T_rel <- the best candidate; false: none has a finite score
//   bool information()      the sums at lambda = 0 with the pivot floors; leaves (H_rr - S)^-1; false: the pair is degenerate
//   double final_costs()    cost of every view (left | right) at the current point; returns the sum
// Returns the status; *have: the pair has a result; *sse: its cost.
// ---------------------------------------------------------------------------------------------------------
template <class BE>
MCBA_HD int solve_pair(BE& be, int max_iter, int* iters, bool* have, double* sse) {
  *have = false;
  *iters = 0;
  *sse = 0.0;
  if (!be.start()) return ST_DEGENERATE;
  bool finite = false;
  const bool converged = intr::lm_loop(be, max_iter, iters, &finite);
  if (!finite) return ST_DEGENERATE;
  const double cost = be.linearize();   // (at the returned point: the covariance is stated there)
  if (!(cost < 1e300) || !be.information()) return ST_DEGENERATE;
  *sse = be.final_costs();
  *have = true;
  return converged ? ST_OK : ST_NOT_CONVERGED;
}

// ---------------------------------------------------------------------------------------------------------
// the plain-loop back-end.  DEVICE_ORDER: the sums in the order of k_stereo_pair (the rows of a view chunk by chunk of 64 corners,
// left rows before right rows; the corner sums of a residual pass, and the step norms of a wave's views, as 64 lane partials folded
// by the xor butterfly; the views dealt round-robin to four wave partials that are added in wave order) instead of table order
// ---------------------------------------------------------------------------------------------------------
template <bool DEVICE_ORDER>
struct SerialBackend {
  static constexpr int NW = DEVICE_ORDER ? WAVES : 1;
  Tables t;
  PairViews v;
  double p[6], q[6], pe[POSE_STRIDE], qe[POSE_STRIDE], hs[PART], ss[PART], di[6], inv[36];

  const double* rec(int side) const { return t.recs + (size_t)(side ? v.r : v.l) * CAM_STRIDE; }
  double* block(int k) const { return v.ws + (size_t)k * VB_STRIDE; }

  void add_rows(int side, int k, int j, const double* ve, const double* e, double* G) const {
    const size_t row = slot_row(t, side ? v.r : v.l, v.slot[k]) + j;
    const int b = v.slot[k] % t.B;
    double ru[NV], rv[NV];
    corner_rows(side, rec(side), ve, e, t.board + ((size_t)b * t.P + j) * 3, t.points[2 * row], t.points[2 * row + 1], ru, rv);
    for (int a = 0; a < NV; ++a)
      for (int c = a; c < NV; ++c) { G[a * GS + c] += ru[a] * ru[c]; G[a * GS + c] += rv[a] * rv[c]; }
  }

  double linearize() {
    double part[NW][PART], G[GS * GS];
    for (int w = 0; w < NW; ++w)
      for (int e = 0; e < PART; ++e) part[w][e] = 0.0;
    for (int k = 0; k < v.nv; ++k) {
      const size_t rowl = slot_row(t, v.l, v.slot[k]), rowr = slot_row(t, v.r, v.slot[k]);
      const int b = v.slot[k] % t.B;
      double ve[POSE_STRIDE];
      pose_entry(block(k) + VB_P, ve);
      for (int i = 0; i < GS * GS; ++i) G[i] = 0.0;
      if (DEVICE_ORDER) {
        for (int base = 0; base < t.P; base += 64)
          for (int side = 0; side < 2; ++side)
            for (int j = base; j < t.P && j < base + 64; ++j)
              if (common_corner(t, rowl, rowr, b, j)) add_rows(side, k, j, ve, pe, G);
      } else {
        for (int j = 0; j < t.P; ++j)
          if (common_corner(t, rowl, rowr, b, j))
            for (int side = 0; side < 2; ++side) add_rows(side, k, j, ve, pe, G);
      }
      for (int e = 0; e < N_PAIR_SUMS; ++e) part[k % NW][e] += pair_sum_entry(G, e);
      for (int e = 0; e < N_VIEW_ENTRIES; ++e) view_entry(G, e, block(k));
    }
    fold(part, N_PAIR_SUMS, hs);
    return hs[42];
  }

  // the xor butterfly over 64 lane partials: every lane ends with the same bits
  static void xor_fold(double* lanes) {
    for (int off = 32; off > 0; off >>= 1) {
      double c[64];
      for (int l = 0; l < 64; ++l) c[l] = lanes[l] + lanes[l ^ off];
      for (int l = 0; l < 64; ++l) lanes[l] = c[l];
    }
  }

  static void fold(const double (*part)[PART], int n, double* out) {
    for (int e = 0; e < n; ++e) {
      double s = part[0][e];
      for (int w = 1; w < NW; ++w) s += part[w][e];
      out[e] = s;
    }
  }

  // W and the Schur sums of every view; false: a block did not factor
  bool eliminate(double lambda, double floor) {
    double part[NW][PART];
    for (int w = 0; w < NW; ++w)
      for (int e = 0; e < PART; ++e) part[w][e] = 0.0;
    bool ok = true;
    for (int k = 0; k < v.nv; ++k) {
      for (int j = 0; j <= 6; ++j) ok = view_w_column(block(k), lambda, j, floor) && ok;
      for (int e = 0; e < N_SCHUR; ++e) part[k % NW][e] += view_schur_entry(block(k), e);
    }
    fold(part, N_SCHUR, ss);
    return ok;
  }

  bool solve(double lambda, bool* small) {
    if (!eliminate(lambda, 0.0)) return false;
    double dn = 0.0, pn = 0.0;
    if (!reduced_solve(hs, ss, lambda, di, p, q, &dn, &pn)) return false;
    pose_entry(q, qe);
    double wd[NW], wp[NW];
    for (int w = 0; w < NW; ++w) wd[w] = wp[w] = 0.0;
    if (DEVICE_ORDER) {   // lane l of wave w takes the wave's views l, l + 64, ...; lane partials folded by the xor butterfly
      double ld[NW][64], lp[NW][64];
      for (int w = 0; w < NW; ++w)
        for (int l = 0; l < 64; ++l) ld[w][l] = lp[w][l] = 0.0;
      for (int k = 0; k < v.nv; ++k) view_backsub(block(k), di, &ld[k % NW][(k / NW) & 63], &lp[k % NW][(k / NW) & 63]);
      for (int w = 0; w < NW; ++w) {
        xor_fold(ld[w]);
        xor_fold(lp[w]);
        wd[w] = ld[w][0];
        wp[w] = lp[w][0];
      }
    } else {
      for (int k = 0; k < v.nv; ++k) view_backsub(block(k), di, &wd[0], &wp[0]);
    }
    for (int w = 0; w < NW; ++w) { dn += wd[w]; pn += wp[w]; }
    *small = sqrt(dn) <= pnp::LM_STEP_TOL * (sqrt(pn) + pnp::LM_STEP_TOL);
    return true;
  }

  // cost of the views at their trial poses with the relative pose e; SCORE: as a start candidate pays it
  template <bool SCORE>
  double costs(const double* e) {
    double wc[NW];
    for (int w = 0; w < NW; ++w) wc[w] = 0.0;
    for (int k = 0; k < v.nv; ++k) {
      const size_t rowl = slot_row(t, v.l, v.slot[k]), rowr = slot_row(t, v.r, v.slot[k]);
      const int b = v.slot[k] % t.B;
      double ve[POSE_STRIDE], lanes[2][64];
      pose_entry(block(k) + VB_Q, ve);
      for (int l = 0; l < 64; ++l) lanes[0][l] = lanes[1][l] = 0.0;
      for (int j = 0; j < t.P; ++j) {
        if (!common_corner(t, rowl, rowr, b, j)) continue;
        const double* X = t.board + ((size_t)b * t.P + j) * 3;
        lanes[0][DEVICE_ORDER ? j & 63 : 0] += corner_sq<SCORE>(0, rec(0), ve, e, X, t.points[2 * (rowl + j)], t.points[2 * (rowl + j) + 1]);
        lanes[1][DEVICE_ORDER ? j & 63 : 0] += corner_sq<SCORE>(1, rec(1), ve, e, X, t.points[2 * (rowr + j)], t.points[2 * (rowr + j) + 1]);
      }
      if (DEVICE_ORDER)
        for (int side = 0; side < 2; ++side) xor_fold(lanes[side]);
      if (!SCORE) { block(k)[VB_SSE] = lanes[0][0]; block(k)[VB_SSE + 1] = lanes[1][0]; }
      wc[k % NW] += lanes[0][0] + lanes[1][0];
    }
    double s = wc[0];
    for (int w = 1; w < NW; ++w) s += wc[w];
    return s;
  }
  double trial() { return costs<false>(qe); }

  void copy_views(int from, int to) {
    for (int k = 0; k < v.nv; ++k)
      for (int i = 0; i < 6; ++i) block(k)[to + i] = block(k)[from + i];
  }
  void accept() {
    for (int i = 0; i < 6; ++i) p[i] = q[i];
    for (int i = 0; i < POSE_STRIDE; ++i) pe[i] = qe[i];
    copy_views(VB_Q, VB_P);
  }

  bool start() {
    for (int k = 0; k < v.nv; ++k) {
      const size_t view = (size_t)v.l * t.F * t.B + (size_t)v.slot[k];
      intr::pose_to_params(t.view_poses + 16 * view, block(k) + VB_P);
    }
    copy_views(VB_P, VB_Q);
    int picks[MAX_CANDIDATES];
    const int nc = select_views(v.nv, v.n_common, picks);
    double cand[MAX_CANDIDATES][6], scores[MAX_CANDIDATES];
    for (int c = 0; c < nc; ++c) {
      const size_t s = (size_t)v.slot[picks[c]], fb = (size_t)t.F * t.B;
      candidate_params(t.view_poses + 16 * ((size_t)v.l * fb + s), t.view_poses + 16 * ((size_t)v.r * fb + s), cand[c]);
      pose_entry(cand[c], qe);
      scores[c] = costs<true>(qe);
    }
    const int best = localize::pick_candidate(scores, nc);
    if (best < 0) return false;
    for (int i = 0; i < 6; ++i) p[i] = cand[best][i];
    pose_entry(p, pe);
    return true;
  }

  bool information() { return eliminate(0.0, PIVOT_FLOOR) && reduced_inverse(hs, ss, inv); }

  double final_costs() {
    copy_views(VB_P, VB_Q);
    return costs<false>(pe);
  }
};

}  // namespace stereo
}  // namespace mcba
