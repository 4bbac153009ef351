// mcba_intrinsic.h -- single-camera intrinsic calibration from the detections of one camera (FP64 throughout).
//
// Restates Camera.calibrate / CameraFisheye.calibrate (camera.py:69-105, camera_fisheye.py:71-94: cv2.calibrateCameraExtended,
// cv2.fisheye.calibrate) for a batch of independent cameras.  Unknowns of a camera: fx fy cx cy | dist[nd] and one pose (rotation
// vector | translation) per view; cost: sum over views and corners of |project(K, dist, R_v X + t_v) - observed|^2 in pixels,
// the projection being project_point of mcba_math.h (every family bundle_adjust serves).
//   start        homography board plane -> pixels per view (the DLT of mcba_pnp.h on raw pixels); pinhole: principal point at the
//                image centre and (1/fx^2, 1/fy^2) by least squares over the two orthogonality constraints of every view
//                (OpenCV's initIntrinsicParams2D in substance); fisheye: the same, with f = max(w, h) / pi as the fall-back
//                (camera_start says why); distortion 0; the view poses come
//                from pnp::view_pose with that camera.  The start only has to lie in the basin of attraction.
//   refinement   Levenberg-Marquardt with Marquardt scaling (lambda diag(H)) and the accept / reject policy of pnp::lm_refine.
//                One linearisation = per view the Gram matrix G_v of the rows [J_i | J_v | r] (<= 18 + 6 + 1 columns), the view
//                eliminated by its 6x6 block (Schur complement), the reduced k_i x k_i system solved by Cholesky, the views
//                back-substituted, and the trial cost from a residual-only pass.  Iterated to convergence (scaled step below
//                LM_STEP_TOL), not to cv2's (10, 1e-3) criterion.
//   held         a column whose mask entry is 0 (free_dist, and fy under fix_aspect through project_point) is a zero column:
//                unit diagonal, zero step -- the project's convention.  Skew is never estimated.
// Everything is MCBA_HD: k_calibrate_camera (mcba_intrinsic_kernels.h) runs one camera per workgroup, tests/intrinsic_host
// builds the same source with g++.  What differs between the two -- who walks the corners and the views, in which order the
// sums are formed, where the barriers are -- is the BACK-END the loop below is written against.
#pragma once
#include "mcba_pnp.h"

namespace mcba {
namespace intr {

// status byte of a camera (mcba.h: MCBA_CAMERA_*)
constexpr int CAM_OK = 0, CAM_TOO_FEW_VIEWS = 1, CAM_DEGENERATE = 2, CAM_NOT_CONVERGED = 3, CAM_MASKED = 4;
constexpr int MIN_VIEWS = 3;
constexpr int MAX_KI = 4 + MAX_DIST;            // intrinsic columns: fx fy cx cy | dist
constexpr int BLK = 5 + MAX_DIST;               // parameter block [fx fy cx cy skew dist...]
constexpr int GS = 32;                          // row stride of a view's Gram matrix (two 16-column tiles)
constexpr double FOCAL_RANK_TOL = 1e-10;        // relative determinant of the focal start's 2x2 normal matrix

// per-view block of the workspace (doubles)
constexpr int VB_HVV = 0;                        // [6][6]      J_v^T J_v
constexpr int VB_HVI = 36;                       // [6][MAX_KI] J_v^T J_i
constexpr int VB_GV = VB_HVI + 6 * MAX_KI;       // [6]         J_v^T r
constexpr int VB_W = VB_GV + 6;                  // [6][MAX_KI + 1] (H_vv + lambda D_v)^-1 [H_vi | g_v]
constexpr int VB_P = VB_W + 6 * (MAX_KI + 1);    // [6] pose
constexpr int VB_Q = VB_P + 6;                   // [6] trial pose
constexpr int VB_SSE = VB_Q + 6;                 // cost of the view at the trial point
constexpr int VB_STRIDE = VB_SSE + 2;
constexpr int WS = MAX_KI + 1;                   // row stride of W

// column of the parameter block that intrinsic column j (skew omitted) lives in
MCBA_HD constexpr int blk_index(int j) { return j < 4 ? j : j + 1; }

MCBA_HD double gsym(const double* G, int i, int j) { return i <= j ? G[i * GS + j] : G[j * GS + i]; }

// ---------------------------------------------------------------------------------------------------------
// per corner
// ---------------------------------------------------------------------------------------------------------
// the two Jacobian rows [Kc * mask | A (-[R X]x | I) diag(L, I) | r] of one corner: KI + 7 entries each
template <int ND, bool FISH>
MCBA_HD void corner_rows(const double* e, const double* R, const double* L, const double* t, const double* mask, const double* X,
                         double u, double v, double* ru, double* rv) {
  constexpr int KI = 4 + ND;
  double Xr[3], Xc[3], uv[2], A[6], Kc[2 * KI], E[12];
  mat3_vec(R, X, Xr);
  Xc[0] = Xr[0] + t[0]; Xc[1] = Xr[1] + t[1]; Xc[2] = Xr[2] + t[2];
  project_point<ND, FISH ? 1 : 0, true>(e, e + CAM_TILT, Xc, uv, A, Kc);
  MCBA_UNROLL
  for (int i = 0; i < KI; ++i) { ru[i] = Kc[i] * mask[i]; rv[i] = Kc[KI + i] * mask[i]; }
  base_rows(A, Xr, E);
  MCBA_UNROLL
  for (int c = 0; c < 3; ++c) {
    ru[KI + c] = E[0] * L[c] + E[1] * L[3 + c] + E[2] * L[6 + c];
    rv[KI + c] = E[6] * L[c] + E[7] * L[3 + c] + E[8] * L[6 + c];
    ru[KI + 3 + c] = E[3 + c];
    rv[KI + 3 + c] = E[9 + c];
  }
  ru[KI + 6] = uv[0] - u;
  rv[KI + 6] = uv[1] - v;
}

template <int ND, bool FISH>
MCBA_HD double corner_sse(const double* e, const double* R, const double* t, const double* X, double u, double v) {
  double Xr[3], Xc[3], uv[2];
  mat3_vec(R, X, Xr);
  Xc[0] = Xr[0] + t[0]; Xc[1] = Xr[1] + t[1]; Xc[2] = Xr[2] + t[2];
  project_point<ND, FISH ? 1 : 0, false>(e, e + CAM_TILT, Xc, uv, nullptr, nullptr);
  return (uv[0] - u) * (uv[0] - u) + (uv[1] - v) * (uv[1] - v);
}

// ---------------------------------------------------------------------------------------------------------
// per view, entry by entry (the back-end spreads the entries over its lanes)
// ---------------------------------------------------------------------------------------------------------
// entries of the camera's sums a view contributes: e < KI KI -> H_ii, then KI of g_i, then the cost
MCBA_HD constexpr int n_cam_sums(int KI) { return KI * KI + KI + 1; }
MCBA_HD double cam_sum_entry(const double* G, int KI, int e) {
  if (e < KI * KI) return gsym(G, e / KI, e % KI);
  if (e < KI * KI + KI) return gsym(G, e - KI * KI, KI + 6);
  return G[(KI + 6) * GS + KI + 6];
}
// entries of the view's own blocks: H_vv, H_vi, g_v
MCBA_HD constexpr int n_view_entries(int KI) { return 36 + 6 * KI + 6; }
MCBA_HD void view_entry(const double* G, int KI, int e, double* vb) {
  if (e < 36) vb[VB_HVV + e] = gsym(G, KI + e / 6, KI + e % 6);
  else if (e < 36 + 6 * KI) { const int a = (e - 36) / KI, i = (e - 36) % KI; vb[VB_HVI + a * MAX_KI + i] = gsym(G, i, KI + a); }
  else vb[VB_GV + (e - 36 - 6 * KI)] = gsym(G, KI + (e - 36 - 6 * KI), KI + 6);
}
// column j <= KI of W = (H_vv + lambda D_v)^-1 [H_vi | g_v]; false: the damped block is not positive definite
MCBA_HD bool view_w_column(double* vb, int KI, double lambda, int j) {
  double M[36], rhs[6], out[6];
  MCBA_UNROLL
  for (int i = 0; i < 36; ++i) M[i] = vb[VB_HVV + i];
  MCBA_UNROLL
  for (int k = 0; k < 6; ++k) {
    M[7 * k] = M[7 * k] > 0.0 ? M[7 * k] * (1.0 + lambda) : 1.0;
    rhs[k] = j < KI ? vb[VB_HVI + k * MAX_KI + j] : vb[VB_GV + k];
  }
  if (!pnp::chol6_solve(M, rhs, out)) return false;
  MCBA_UNROLL
  for (int k = 0; k < 6; ++k) vb[VB_W + k * WS + j] = out[k];
  return true;
}
// entry e = i (KI + 1) + j of H_iv W: columns j < KI the Schur complement S_v, column KI its right-hand side
MCBA_HD double view_schur_entry(const double* vb, int KI, int e) {
  const int i = e / (KI + 1), j = e % (KI + 1);
  double s = 0.0;
  MCBA_UNROLL
  for (int k = 0; k < 6; ++k) s += vb[VB_HVI + k * MAX_KI + i] * vb[VB_W + k * WS + j];
  return s;
}
// back-substitution: q = p - W [delta_i ; 1]; adds the view's part of the scaled step and parameter norms
MCBA_HD void view_backsub(double* vb, int KI, const double* di, double* dn, double* pn) {
  MCBA_NOUNROLL
  for (int k = 0; k < 6; ++k) {
    double s = vb[VB_W + k * WS + KI];
    for (int i = 0; i < KI; ++i) s += vb[VB_W + k * WS + i] * di[i];
    const double p = vb[VB_P + k], d = vb[VB_HVV + 7 * k] > 0.0 ? vb[VB_HVV + 7 * k] : 1.0;
    vb[VB_Q + k] = p - s;
    *dn += d * s * s;
    *pn += d * p * p;
  }
}

// ---------------------------------------------------------------------------------------------------------
// per camera
// ---------------------------------------------------------------------------------------------------------
// reduced system (H_ii + lambda D_i - S) delta = -(g_i - s) from the camera's sums hs [n_cam_sums] and the Schur sums
// ss [KI (KI + 1)]; A [KI KI] is scratch.  blk -> trial block; adds the camera's part of the step norms.
MCBA_HD bool reduced_solve(int KI, const double* hs, const double* ss, double lambda, double* A, double* di, const double* blk,
                           double* qblk, double* dn, double* pn) {
  for (int i = 0; i < KI; ++i) {
    const double d = hs[i * KI + i];
    for (int j = 0; j < KI; ++j) A[i * KI + j] = hs[i * KI + j] - ss[i * (KI + 1) + j];
    A[i * KI + i] = d > 0.0 ? d * (1.0 + lambda) - ss[i * (KI + 1) + i] : 1.0;
    di[i] = d > 0.0 ? -(hs[KI * KI + i] - ss[i * (KI + 1) + KI]) : 0.0;
  }
  for (int j = 0; j < KI; ++j) {              // Cholesky in place (lower triangle), forward and backward substitution
    double d = A[j * KI + j];
    for (int k = 0; k < j; ++k) d -= A[j * KI + k] * A[j * KI + k];
    if (!(d > 0.0)) return false;
    const double l = sqrt(d);
    A[j * KI + j] = l;
    for (int i = j + 1; i < KI; ++i) {
      double s = A[i * KI + j];
      for (int k = 0; k < j; ++k) s -= A[i * KI + k] * A[j * KI + k];
      A[i * KI + j] = s / l;
    }
  }
  for (int i = 0; i < KI; ++i) {
    double s = di[i];
    for (int k = 0; k < i; ++k) s -= A[i * KI + k] * di[k];
    di[i] = s / A[i * KI + i];
  }
  for (int i = KI - 1; i >= 0; --i) {
    double s = di[i];
    for (int k = i + 1; k < KI; ++k) s -= A[k * KI + i] * di[k];
    di[i] = s / A[i * KI + i];
  }
  for (int i = 0; i < BLK; ++i) qblk[i] = blk[i];
  for (int i = 0; i < KI; ++i) {
    const double d = hs[i * KI + i] > 0.0 ? hs[i * KI + i] : 1.0, p = blk[blk_index(i)];
    qblk[blk_index(i)] = p + di[i];
    *dn += d * di[i] * di[i];
    *pn += d * p * p;
  }
  return true;
}

// focal start of a pinhole camera from the homographies Hv [n][10] (H [9] row-major plane -> pixels, then a usable flag)
MCBA_HD bool focal_start(const double* Hv, int n, double w, double h, bool fix_aspect, double* blk) {
  const double cx = 0.5 * (w - 1.0), cy = 0.5 * (h - 1.0);
  double n00 = 0.0, n01 = 0.0, n11 = 0.0, b0 = 0.0, b1 = 0.0;
  MCBA_NOUNROLL
  for (int v = 0; v < n; ++v) {
    const double* H = Hv + 10 * v;
    if (!(H[9] != 0.0)) continue;
    // principal point shifted out, columns scaled to |h1| |h2| = 1 (H is only known up to scale)
    double h1[3] = {H[0] - cx * H[6], H[3] - cy * H[6], H[6]}, h2[3] = {H[1] - cx * H[7], H[4] - cy * H[7], H[7]};
    const double s = 1.0 / sqrt(sqrt(h1[0] * h1[0] + h1[1] * h1[1] + h1[2] * h1[2]) * sqrt(h2[0] * h2[0] + h2[1] * h2[1] + h2[2] * h2[2]));
    MCBA_UNROLL
    for (int k = 0; k < 3; ++k) { h1[k] *= s; h2[k] *= s; }
    // h1^T w h2 = 0,  h1^T w h1 = h2^T w h2,  w = diag(a, b, 1)
    const double c[2][3] = {{h1[0] * h2[0], h1[1] * h2[1], -h1[2] * h2[2]},
                            {h1[0] * h1[0] - h2[0] * h2[0], h1[1] * h1[1] - h2[1] * h2[1], -(h1[2] * h1[2] - h2[2] * h2[2])}};
    MCBA_UNROLL
    for (int r = 0; r < 2; ++r) {
      n00 += c[r][0] * c[r][0]; n01 += c[r][0] * c[r][1]; n11 += c[r][1] * c[r][1];
      b0 += c[r][0] * c[r][2]; b1 += c[r][1] * c[r][2];
    }
  }
  double a, b;
  if (fix_aspect) {
    const double m = n00 + 2.0 * n01 + n11;
    if (!(m > FOCAL_RANK_TOL * (n00 + n11))) return false;
    a = b = (b0 + b1) / m;
  } else {
    const double det = n00 * n11 - n01 * n01;
    if (!(det > FOCAL_RANK_TOL * n00 * n11)) return false;
    a = (n11 * b0 - n01 * b1) / det;
    b = (n00 * b1 - n01 * b0) / det;
  }
  if (!(a > 0.0) || !(b > 0.0) || !(a < 1e300) || !(b < 1e300)) return false;
  for (int i = 0; i < BLK; ++i) blk[i] = 0.0;
  blk[0] = 1.0 / sqrt(a);
  blk[1] = 1.0 / sqrt(b);
  blk[2] = cx;
  blk[3] = cy;
  return blk[0] < 1e300 && blk[1] < 1e300;
}
MCBA_HD void fisheye_start(double w, double h, double* blk) {
  for (int i = 0; i < BLK; ++i) blk[i] = 0.0;
  blk[0] = blk[1] = fmax(w, h) / 3.14159265358979323846;
  blk[2] = 0.5 * w - 0.5;
  blk[3] = 0.5 * h - 0.5;
}

// start block of a camera.  A fisheye camera takes the pinhole estimate too when there is one: near the image centre the two
// projections agree, and max(w, h) / pi alone (OpenCV's fisheye start) leaves the ring rigs of this project outside the basin
// of attraction (views end in the mirrored planar pose).  It remains the fall-back, so a fisheye camera is never DEGENERATE here.
MCBA_HD bool camera_start(const double* Hv, int n, double w, double h, bool fix_aspect, bool fisheye, double* blk) {
  if (focal_start(Hv, n, w, h, fix_aspect, blk)) return true;
  if (fisheye) fisheye_start(w, h, blk);
  return fisheye;
}

// homography H [9] (row-major: plane coordinates (a, b, 1) -> (x, y, 1) of the container) of one view: the Hartley-normalised DLT
// of pnp::planar_init, said again here up to the point where that function goes on to the pose -- k_view_pose is an existing
// kernel and stays as it is, instruction for instruction
template <class Pts, class Red>
MCBA_HD bool planar_homography(const Pts& pts, const Red& red, const double* plane, double n, double* H) {
  const double ox = plane[0], oy = plane[1], oz = plane[2];
  const double e1x = plane[3], e1y = plane[4], e1z = plane[5], e2x = plane[6], e2y = plane[7], e2z = plane[8];
  auto plane_ab = [&](int i, double& a, double& b) MCBA_TERMS {
    const double dx = pts.X[i] - ox, dy = pts.Y[i] - oy, dz = pts.Z[i] - oz;
    a = e1x * dx + e1y * dy + e1z * dz;
    b = e2x * dx + e2y * dy + e2z * dz;
  };
  // Hartley normalisation of both sides: centroid to the origin, mean distance sqrt(2)
  double m[4];
  red.template sum<4>(pts, [&](int i, double* q) MCBA_TERMS { plane_ab(i, q[0], q[1]); q[2] = pts.x[i]; q[3] = pts.y[i]; }, m);
  const double ma = m[0] / n, mb = m[1] / n, mx = m[2] / n, my = m[3] / n;
  double d[2];
  red.template sum<2>(pts, [&](int i, double* q) MCBA_TERMS {
    double a, b;
    plane_ab(i, a, b);
    q[0] = sqrt((a - ma) * (a - ma) + (b - mb) * (b - mb));
    q[1] = sqrt((pts.x[i] - mx) * (pts.x[i] - mx) + (pts.y[i] - my) * (pts.y[i] - my));
  }, d);
  if (!(d[0] > 0.0) || !(d[1] > 0.0)) return false;
  const double sp = 1.4142135623730951 * n / d[0], sx = 1.4142135623730951 * n / d[1];
  // normal matrix of the DLT rows  [-p 0 x p] and [0 -p y p],  p = (a', b', 1): upper triangle, 45 sums
  double tri[45];
  red.template sum<45>(pts, [&](int i, double* q) MCBA_TERMS {
    double a, b;
    plane_ab(i, a, b);
    a = sp * (a - ma);
    b = sp * (b - mb);
    const double x = sx * (pts.x[i] - mx), y = sx * (pts.y[i] - my);
    const double r1[9] = {-a, -b, -1.0, 0.0, 0.0, 0.0, x * a, x * b, x};
    const double r2[9] = {0.0, 0.0, 0.0, -a, -b, -1.0, y * a, y * b, y};
    int idx = 0;
    MCBA_UNROLL
    for (int r = 0; r < 9; ++r) {
      MCBA_UNROLL
      for (int c = r; c < 9; ++c) q[idx++] = r1[r] * r1[c] + r2[r] * r2[c];
    }
  }, tri);
  double V[81];
  pnp::jacobi_eig<9>(tri, V);
  // smallest eigenvalue's vector; the second smallest must stand clear of it (collinear corners: a null space of 2 or more)
  double l0 = tri[0], l1 = 1e300, lmax = tri[0];
  double h[9];
  MCBA_UNROLL
  for (int r = 0; r < 9; ++r) h[r] = V[r * 9];
  MCBA_UNROLL
  for (int k = 1; k < 9; ++k) {
    const double l = tri[pnp::tri_index(9, k, k)];
    lmax = fmax(lmax, l);
    if (l < l0) {
      l1 = l0;
      l0 = l;
      MCBA_UNROLL
      for (int r = 0; r < 9; ++r) h[r] = V[r * 9 + k];
    } else if (l < l1) {
      l1 = l;
    }
  }
  if (!(l1 > 1e-12 * lmax) || !(lmax > 0.0)) return false;
  // undo the normalisations: H = Tx^-1 Hn Tp
  double G[9];
  MCBA_UNROLL
  for (int r = 0; r < 3; ++r) {
    G[3 * r] = sp * h[3 * r];
    G[3 * r + 1] = sp * h[3 * r + 1];
    G[3 * r + 2] = h[3 * r + 2] - sp * (ma * h[3 * r] + mb * h[3 * r + 1]);
  }
  MCBA_UNROLL
  for (int c = 0; c < 3; ++c) {
    H[c] = G[c] / sx + mx * G[6 + c];
    H[3 + c] = G[3 + c] / sx + my * G[6 + c];
    H[6 + c] = G[6 + c];
  }
  return true;
}

// container fill for the homography on RAW pixels: x, y = the detection itself
template <class Pts>
MCBA_HD void load_view_raw(Pts& pts, int lane, int lanes, int P, const double* pixel, const uint8_t* valid, const double* board) {
  pts.clear();
  MCBA_NOUNROLL
  for (int i = 0; i < pts.size(); ++i) {
    const int j = lane + lanes * i;
    const bool good = j < P && valid[j] != 0;
    double x = 0.0, y = 0.0, X = 0.0, Y = 0.0, Z = 0.0;
    if (good) { x = pixel[2 * j]; y = pixel[2 * j + 1]; X = board[3 * j]; Y = board[3 * j + 1]; Z = board[3 * j + 2]; }
    pts.set(i, good, x, y, X, Y, Z);
  }
}
// homography of one view into Hv [10]
template <class Pts, class Red>
MCBA_HD void view_homography(const Pts& pts, const Red& red, const double* plane, double* Hv) {
  double cnt[1];
  red.template sum<1>(pts, [&](int, double* q) MCBA_TERMS { q[0] = 1.0; }, cnt);
  bool ok = cnt[0] + 0.5 >= (double)pnp::MIN_CORNERS;
  MCBA_UNROLL
  for (int i = 0; i < 9; ++i) Hv[i] = 0.0;
  if (ok) ok = planar_homography(pts, red, plane, (double)(int)(cnt[0] + 0.5), Hv);
  Hv[9] = ok ? 1.0 : 0.0;
}

// ---------------------------------------------------------------------------------------------------------
// Levenberg-Marquardt loop over a back-end BE.  Every value a back-end method returns is the same in every thread that runs
// the loop, so the control flow is uniform (the device back-end has barriers inside its methods).
//   double linearize()                       blocks and sums at the current point; returns the cost
//   bool   solve(lambda, bool* small)        step and trial point; false: a damped block is not positive definite;
//                                            *small: the scaled step meets LM_STEP_TOL
//   double trial()                           cost at the trial point (residual-only pass)
//   void   accept()                          current point <- trial point
// Returns true when the step test was met; *iters = passes of the loop + 1 (every pass holds at most one linearisation).
// ---------------------------------------------------------------------------------------------------------
template <class BE>
MCBA_HD bool lm_loop(BE& be, int max_iter, int* iters, bool* finite) {
  double cost = be.linearize();
  int used = 1;
  double lambda = 1e-3;
  bool converged = false;
  *finite = cost < 1e300;
  if (!*finite) { *iters = used; return false; }
  MCBA_NOUNROLL
  while (used < max_iter) {
    ++used;   // (every pass is counted so that a run of rejected steps cannot spin)
    bool small = false;
    if (!be.solve(lambda, &small)) {
      lambda = lambda * 10.0 + 1e-12;
      if (!(lambda < 1e30)) break;
      continue;
    }
    if (small) {
      be.accept();
      converged = true;
      break;
    }
    const double cq = be.trial();
    if (cq <= cost * (1.0 + pnp::LM_ACCEPT_SLACK)) {
      be.accept();
      cost = be.linearize();
      lambda = fmax(lambda * 0.1, 1e-15);
    } else {
      lambda = fmin(lambda * 10.0, 1e30);
    }
  }
  *iters = used;
  return converged;
}

// start pose of the refinement from a row-major 4x4
MCBA_HD void pose_to_params(const double* pose, double* p) {
  double R[9];
  MCBA_UNROLL
  for (int r = 0; r < 3; ++r) {
    MCBA_UNROLL
    for (int c = 0; c < 3; ++c) R[3 * r + c] = pose[4 * r + c];
    p[3 + r] = pose[4 * r + 3];
  }
  pnp::rotvec_of_matrix(R, p);
}
MCBA_HD void params_to_pose(const double* p, double* pose) {
  double R[9], L[9];
  rodrigues(p, R, L);
  MCBA_UNROLL
  for (int i = 0; i < 16; ++i) pose[i] = (i % 5 == 0) ? 1.0 : 0.0;
  MCBA_UNROLL
  for (int r = 0; r < 3; ++r) {
    MCBA_UNROLL
    for (int c = 0; c < 3; ++c) pose[4 * r + c] = R[3 * r + c];
    pose[4 * r + 3] = p[3 + r];
  }
}

}  // namespace intr
}  // namespace mcba
