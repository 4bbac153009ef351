// mcba_pnp.h -- per-view board pose from the detections of one (camera, frame, board) table slot (FP64 throughout).
//
// Restates board.estimate_pose_points (board/common.py:36-47: camera.undistort_points + cv2.solvePnPGeneric with K and no
// distortion) for a batch of independent views.  Three steps per view:
//   undistort     exact inverse of the project's own distortion (distort_pinhole / distort_fisheye of mcba_math.h) by Newton's
//                 method on the 2x2 Jacobian those functions return -- NOT cv2's five fixed-point sweeps -- and kept in FP64
//                 (the reference hands cv2 float32 points: <= 2^-24 x image width);
//   initialise    Hartley-normalised DLT homography board plane -> normalised image, smallest eigenvector of the 9x9 normal
//                 matrix by cyclic Jacobi sweeps, [r1 r2 t] -> nearest rotation by polar iteration, board in front of the camera;
//   refine        Levenberg-Marquardt on (rotation vector | translation) of  sum |K pi(R X + t) - K (x, y, 1)|^2  (pixels),
//                 iterated to convergence (relative step < 1e-13), not to cv2's loose stop.
// Everything is MCBA_HD like mcba_math.h: k_view_pose (mcba_pnp_kernels.h) runs one view per wavefront, tests/pnp_host builds
// the same source with g++.  The sums over the corners of a view go through a REDUCER type: a wave butterfly on the device, a
// plain loop (or its 64-bucket emulation of the butterfly) on the host.  The corner container is a template parameter too:
// fixed-size register arrays per lane on the device, pointers on the host.
#pragma once
#include <stdint.h>
#include "mcba_math.h"

#if defined(__HIPCC__)
#define MCBA_UNROLL _Pragma("unroll")
#define MCBA_NOUNROLL _Pragma("nounroll")
#else
#define MCBA_UNROLL
#define MCBA_NOUNROLL
#endif
// per-corner term functions are lambdas: they must be inlined into the reducer's loop for the register arrays to stay registers
#define MCBA_TERMS __attribute__((always_inline))

namespace mcba {
namespace pnp {

// status byte of a view (mcba.h: MCBA_VIEW_*)
constexpr int ST_OK = 0, ST_TOO_FEW = 1, ST_MASKED = 2, ST_DEGENERATE = 3, ST_NOT_CONVERGED = 4;
constexpr int MIN_CORNERS = 4;
constexpr int UNDISTORT_MAX_ITER = 25;
constexpr double UNDISTORT_TOL = 1e-14;     // Newton step, normalised units
constexpr double LM_STEP_TOL = 1e-13;       // |step| <= tol (|p| + tol)
constexpr double LM_ACCEPT_SLACK = 1e-12;   // a trial whose cost is within rounding of the current one counts as a descent
constexpr int PLANE_STRIDE = 12;            // o[3] | e1[3] e2[3] e3[3]  (rows of E^T): plane coordinates (a, b, c) = E^T (X - o)
constexpr double PLANAR_TOL = 1e-9;         // largest |c| over the board's extent

// ---------------------------------------------------------------------------------------------------------
// undistortion of one pixel: solve distort(x, y) = ((u - cx) / fx, (v - cy) / fy), start at the distorted point
// ---------------------------------------------------------------------------------------------------------
template <int ND, bool FISH>
MCBA_HD bool undistort_newton(const double* cam, double u, double v, double& x, double& y) {
  const double* k = cam + CAM_K;
  const double xt = (u - cam[CAM_CX]) / cam[CAM_FX], yt = (v - cam[CAM_CY]) / cam[CAM_FY];
  x = xt;
  y = yt;
  MCBA_NOUNROLL
  for (int it = 0; it < UNDISTORT_MAX_ITER; ++it) {
    double xd, yd, dxx = 0, dxy = 0, dyx = 0, dyy = 0;
    double dk[2 * ND];
    if constexpr (FISH) distort_fisheye<ND, true>(k, x, y, xd, yd, dxx, dxy, dyx, dyy, dk);
    else distort_pinhole<ND, true>(k, cam + CAM_TILT, x, y, xd, yd, dxx, dxy, dyx, dyy, dk);
    const double det = dxx * dyy - dxy * dyx;
    if (!(det > 0.0)) return false;          // folded over: outside the model's monotone range
    const double rx = xd - xt, ry = yd - yt;
    const double sx = (dyy * rx - dxy * ry) / det, sy = (dxx * ry - dyx * rx) / det;
    x -= sx;
    y -= sy;
    const double s = fmax(fabs(sx), fabs(sy));
    if (!(s < 1e300)) return false;          // (NaN / inf)
    if (s < UNDISTORT_TOL) return true;
  }
  return false;
}

// cam: a camera_entry (under fix_aspect its CAM_FY already holds fx); nd: the camera's own coefficient count
MCBA_HD bool undistort_point(const double* cam, int nd, bool fisheye, double u, double v, double& x, double& y) {
  if (fisheye) return undistort_newton<4, true>(cam, u, v, x, y);
  switch (nd) {
    case 4: return undistort_newton<4, false>(cam, u, v, x, y);
    case 5: return undistort_newton<5, false>(cam, u, v, x, y);
    case 8: return undistort_newton<8, false>(cam, u, v, x, y);
    case 12: return undistort_newton<12, false>(cam, u, v, x, y);
    case 14: return undistort_newton<14, false>(cam, u, v, x, y);
    default: return false;
  }
}
MCBA_HD bool supported_model(int nd, bool fisheye) {
  return fisheye ? nd >= 4 : (nd == 4 || nd == 5 || nd == 8 || nd == 12 || nd == 14);
}

// the pose of everything that has no result: row-major 4x4 identity
MCBA_HD void identity_pose(double* T) {
  MCBA_UNROLL
  for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
}

// ---------------------------------------------------------------------------------------------------------
// corner containers.  size() slots per "lane"; slot i of lane l holds corner l + lanes * i of the table slot.
//   x, y      undistorted normalised image point          X, Y, Z   board point (board frame)
// ---------------------------------------------------------------------------------------------------------
template <int N>
struct LanePoints {          // registers: every loop over it has a constant trip count
  double x[N], y[N], X[N], Y[N], Z[N];
  unsigned okmask;
  MCBA_HD static constexpr int size() { return N; }
  MCBA_HD bool ok(int i) const { return (okmask >> i) & 1u; }
  MCBA_HD void clear() { okmask = 0u; }
  // (i is a loop counter of a rolled loop: select chains instead of a dynamically indexed store, which would go to scratch)
  MCBA_HD void set(int i, bool good, double x_, double y_, double X_, double Y_, double Z_) {
    MCBA_UNROLL
    for (int k = 0; k < N; ++k)
      if (k == i) { x[k] = x_; y[k] = y_; X[k] = X_; Y[k] = Y_; Z[k] = Z_; }
    okmask |= (good ? 1u : 0u) << i;
  }
};
struct HostPoints {          // one lane that holds every corner (host builds)
  double *x, *y, *X, *Y, *Z;
  uint8_t* good;
  int n;
  MCBA_HD int size() const { return n; }
  MCBA_HD bool ok(int i) const { return good[i] != 0; }
  MCBA_HD void clear() {}
  MCBA_HD void set(int i, bool g, double x_, double y_, double X_, double Y_, double Z_) {
    x[i] = x_; y[i] = y_; X[i] = X_; Y[i] = Y_; Z[i] = Z_; good[i] = g ? 1 : 0;
  }
};

// fill the container from one table slot: pixel [P][2], valid [P], board points [P][3]; corners that fail to undistort are dropped
template <class Pts>
MCBA_HD void load_view(Pts& pts, int lane, int lanes, int P, const double* pixel, const uint8_t* valid, const double* board,
                       const double* cam, int nd, bool fisheye) {
  pts.clear();
  MCBA_NOUNROLL
  for (int i = 0; i < pts.size(); ++i) {
    const int j = lane + lanes * i;
    bool good = j < P && valid[j] != 0;
    double x = 0.0, y = 0.0, X = 0.0, Y = 0.0, Z = 0.0;
    if (good) {
      good = undistort_point(cam, nd, fisheye, pixel[2 * j], pixel[2 * j + 1], x, y);
      X = board[3 * j]; Y = board[3 * j + 1]; Z = board[3 * j + 2];
    }
    pts.set(i, good, x, y, X, Y, Z);
  }
}

// ---------------------------------------------------------------------------------------------------------
// host reducers (the device's is WaveReducer in mcba_pnp_kernels.h).  sum<K>(pts, f, out): out[k] = sum over the valid corners
// of t[k], f(i, t) filling the K terms of corner i.
// ---------------------------------------------------------------------------------------------------------
struct SerialReducer {       // corners in table order
  template <int K, class Pts, class F>
  void sum(const Pts& pts, F f, double* out) const {
    for (int k = 0; k < K; ++k) out[k] = 0.0;
    for (int i = 0; i < pts.size(); ++i)
      if (pts.ok(i)) {
        double t[K];
        f(i, t);
        for (int k = 0; k < K; ++k) out[k] += t[k];
      }
  }
};
struct PairwiseReducer {     // the order of the device: 64 lane partials (corner j in lane j % 64), then the xor butterfly
  template <int K, class Pts, class F>
  void sum(const Pts& pts, F f, double* out) const {
    double b[64][K], c[64][K];
    for (int l = 0; l < 64; ++l)
      for (int k = 0; k < K; ++k) b[l][k] = 0.0;
    for (int i = 0; i < pts.size(); ++i)
      if (pts.ok(i)) {
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

// ---------------------------------------------------------------------------------------------------------
// small dense algebra with constant indices only (registers on the device)
// ---------------------------------------------------------------------------------------------------------
// index of (i, j), i <= j, in the upper triangle of a symmetric N x N matrix stored by rows
MCBA_HD constexpr int tri_index(int N, int i, int j) { return i * N - i * (i - 1) / 2 + (j - i); }

// cyclic Jacobi on a symmetric N x N matrix held as its upper triangle S (destroyed: the eigenvalues end on its diagonal
// entries tri_index(N, i, i)); V [N x N, row-major] = eigenvectors (columns).  Constant indices only.
template <int N>
MCBA_HD void jacobi_eig(double* S, double* V, int max_sweeps = 30) {
  MCBA_UNROLL
  for (int i = 0; i < N * N; ++i) V[i] = 0.0;
  MCBA_UNROLL
  for (int i = 0; i < N; ++i) V[i * N + i] = 1.0;
  MCBA_NOUNROLL
  for (int sweep = 0; sweep < max_sweeps; ++sweep) {
    double off = 0.0, dia = 0.0;
    MCBA_UNROLL
    for (int p = 0; p < N; ++p) {
      dia += S[tri_index(N, p, p)] * S[tri_index(N, p, p)];
      MCBA_UNROLL
      for (int q = p + 1; q < N; ++q) off += S[tri_index(N, p, q)] * S[tri_index(N, p, q)];
    }
    if (!(off > 1e-30 * dia)) break;         // (also ends on NaN)
    MCBA_UNROLL
    for (int p = 0; p < N - 1; ++p) {
      MCBA_UNROLL
      for (int q = p + 1; q < N; ++q) {
        const double apq = S[tri_index(N, p, q)];
        double c = 1.0, s = 0.0, t = 0.0;
        if (fabs(apq) > 1e-300) {
          const double theta = (S[tri_index(N, q, q)] - S[tri_index(N, p, p)]) / (2.0 * apq);
          t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          c = 1.0 / sqrt(t * t + 1.0);
          s = t * c;
        }
        S[tri_index(N, p, p)] -= t * apq;
        S[tri_index(N, q, q)] += t * apq;
        S[tri_index(N, p, q)] = 0.0;
        MCBA_UNROLL
        for (int k = 0; k < N; ++k) {
          if (k != p && k != q) {
            const int kp = k < p ? tri_index(N, k, p) : tri_index(N, p, k), kq = k < q ? tri_index(N, k, q) : tri_index(N, q, k);
            const double akp = S[kp], akq = S[kq];
            S[kp] = c * akp - s * akq;
            S[kq] = s * akp + c * akq;
          }
        }
        MCBA_UNROLL
        for (int k = 0; k < N; ++k) {
          const double vkp = V[k * N + p], vkq = V[k * N + q];
          V[k * N + p] = c * vkp - s * vkq;
          V[k * N + q] = s * vkp + c * vkq;
        }
      }
    }
  }
}

MCBA_HD bool mat3_inv_transpose(const double* M, double* out, double* det_out) {
  const double c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
  const double c10 = M[2] * M[7] - M[1] * M[8], c11 = M[0] * M[8] - M[2] * M[6], c12 = M[1] * M[6] - M[0] * M[7];
  const double c20 = M[1] * M[5] - M[2] * M[4], c21 = M[2] * M[3] - M[0] * M[5], c22 = M[0] * M[4] - M[1] * M[3];
  const double det = M[0] * c00 + M[1] * c01 + M[2] * c02;
  *det_out = det;
  if (!(fabs(det) > 1e-300)) return false;
  const double id = 1.0 / det;   // M^-T = cofactor matrix / det
  out[0] = c00 * id; out[1] = c01 * id; out[2] = c02 * id;
  out[3] = c10 * id; out[4] = c11 * id; out[5] = c12 * id;
  out[6] = c20 * id; out[7] = c21 * id; out[8] = c22 * id;
  return true;
}

// nearest rotation of M (det > 0) by the Newton polar iteration R <- (R + R^-T) / 2
MCBA_HD bool nearest_rotation(double* M) {
  MCBA_NOUNROLL
  for (int it = 0; it < 40; ++it) {
    double T[9], det;
    if (!mat3_inv_transpose(M, T, &det) || !(det > 0.0)) return false;
    double change = 0.0;
    MCBA_UNROLL
    for (int i = 0; i < 9; ++i) {
      const double r = 0.5 * (M[i] + T[i]);
      change = fmax(change, fabs(r - M[i]));
      M[i] = r;
    }
    if (change < 1e-15) return true;
  }
  return true;   // (quadratic: 40 rounds only run out on a matrix that is singular to rounding, caught by the determinant)
}

// rotation matrix -> rotation vector through the unit quaternion (the branch with the largest pivot), angle in [0, pi]
MCBA_HD void rotvec_of_matrix(const double* R, double* w) {
  const double m00 = R[0], m11 = R[4], m22 = R[8], tr = m00 + m11 + m22;
  double q0, q1, q2, q3;
  if (tr >= m00 && tr >= m11 && tr >= m22) { q0 = R[7] - R[5]; q1 = R[2] - R[6]; q2 = R[3] - R[1]; q3 = 1.0 + tr; }
  else if (m00 >= m11 && m00 >= m22) { q0 = 1.0 - tr + 2.0 * m00; q1 = R[3] + R[1]; q2 = R[6] + R[2]; q3 = R[7] - R[5]; }
  else if (m11 >= m22) { q0 = R[1] + R[3]; q1 = 1.0 - tr + 2.0 * m11; q2 = R[7] + R[5]; q3 = R[2] - R[6]; }
  else { q0 = R[2] + R[6]; q1 = R[5] + R[7]; q2 = 1.0 - tr + 2.0 * m22; q3 = R[3] - R[1]; }
  if (q3 < 0.0) { q0 = -q0; q1 = -q1; q2 = -q2; q3 = -q3; }
  const double sn = sqrt(q0 * q0 + q1 * q1 + q2 * q2);
  const double angle = 2.0 * atan2(sn, q3);
  const double scale = sn > 1e-150 ? angle / sn : 0.0;
  w[0] = scale * q0;
  w[1] = scale * q1;
  w[2] = scale * q2;
}

// Cholesky solve of the packed symmetric 6x6 system (upper triangle by rows: index of (i, j), i <= j, is tri6(i, j))
MCBA_HD constexpr int tri6(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }
// (min_pivot: a pivot at or below it counts as vanished)
MCBA_HD bool chol6_solve(const double* H /*[36] full*/, const double* rhs, double* out, double min_pivot = 0.0) {
  double Lm[36];
  MCBA_UNROLL
  for (int i = 0; i < 36; ++i) Lm[i] = 0.0;
  MCBA_UNROLL
  for (int j = 0; j < 6; ++j) {
    double d = H[j * 6 + j];
    MCBA_UNROLL
    for (int k = 0; k < j; ++k) d -= Lm[j * 6 + k] * Lm[j * 6 + k];
    if (!(d > min_pivot)) return false;
    const double l = sqrt(d), il = 1.0 / l;
    Lm[j * 6 + j] = l;
    MCBA_UNROLL
    for (int i = j + 1; i < 6; ++i) {
      double s = H[i * 6 + j];
      MCBA_UNROLL
      for (int k = 0; k < j; ++k) s -= Lm[i * 6 + k] * Lm[j * 6 + k];
      Lm[i * 6 + j] = s * il;
    }
  }
  double z[6];
  MCBA_UNROLL
  for (int i = 0; i < 6; ++i) {
    double s = rhs[i];
    MCBA_UNROLL
    for (int k = 0; k < i; ++k) s -= Lm[i * 6 + k] * z[k];
    z[i] = s / Lm[i * 6 + i];
  }
  MCBA_UNROLL
  for (int i = 5; i >= 0; --i) {
    double s = z[i];
    MCBA_UNROLL
    for (int k = i + 1; k < 6; ++k) s -= Lm[k * 6 + i] * out[k];
    out[i] = s / Lm[i * 6 + i];
  }
  return true;
}

// ---------------------------------------------------------------------------------------------------------
// plane frame of a board: centroid, in-plane axes (largest spread first), normal; returns max |c| / extent (0 for < 3 points)
// (host side of the API call and of the host build: one call per board)
// ---------------------------------------------------------------------------------------------------------
inline double board_plane(const double* pts, int n, double* plane) {
  double o[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) o[k] += pts[3 * i + k];
  for (int k = 0; k < 3; ++k) o[k] = n > 0 ? o[k] / n : 0.0;
  double S[6] = {0, 0, 0, 0, 0, 0}, V[9];
  double extent = 0.0;
  for (int i = 0; i < n; ++i) {
    const double d[3] = {pts[3 * i] - o[0], pts[3 * i + 1] - o[1], pts[3 * i + 2] - o[2]};
    for (int a = 0; a < 3; ++a)
      for (int b = a; b < 3; ++b) S[tri_index(3, a, b)] += d[a] * d[b];
    extent = fmax(extent, sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]));
  }
  jacobi_eig<3>(S, V);
  int order[3] = {0, 1, 2};   // descending eigenvalue
  for (int a = 0; a < 3; ++a)
    for (int b = a + 1; b < 3; ++b)
      if (S[tri_index(3, order[b], order[b])] > S[tri_index(3, order[a], order[a])]) { const int t = order[a]; order[a] = order[b]; order[b] = t; }
  double e1[3], e2[3], e3[3];
  for (int k = 0; k < 3; ++k) { e1[k] = V[3 * k + order[0]]; e2[k] = V[3 * k + order[1]]; }
  cross3(e1, e2, e3);
  for (int k = 0; k < 3; ++k) { plane[k] = o[k]; plane[3 + k] = e1[k]; plane[6 + k] = e2[k]; plane[9 + k] = e3[k]; }
  double dev = 0.0;
  for (int i = 0; i < n; ++i)
    dev = fmax(dev, fabs(e3[0] * (pts[3 * i] - o[0]) + e3[1] * (pts[3 * i + 1] - o[1]) + e3[2] * (pts[3 * i + 2] - o[2])));
  return (n >= 3 && extent > 0.0) ? dev / extent : 0.0;
}

// ---------------------------------------------------------------------------------------------------------
// planar initialisation: homography (plane coordinates -> normalised image) -> pose board -> camera
// ---------------------------------------------------------------------------------------------------------
template <class Pts, class Red>
MCBA_HD bool planar_init(const Pts& pts, const Red& red, const double* plane, double n, double* R, double* t) {
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
  jacobi_eig<9>(tri, V);
  // smallest eigenvalue's vector; the second smallest must stand clear of it (collinear corners: a null space of 2 or more)
  double l0 = tri[0], l1 = 1e300, lmax = tri[0];
  double h[9];
  MCBA_UNROLL
  for (int r = 0; r < 9; ++r) h[r] = V[r * 9];
  MCBA_UNROLL
  for (int k = 1; k < 9; ++k) {
    const double l = tri[tri_index(9, k, k)];
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
  double G[9], H[9];
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
  // H = s [r1 r2 t]: the sign puts the board's centroid in front of the camera, the scale is the geometric mean of |h1|, |h2|
  const double depth = H[6] * ma + H[7] * mb + H[8];
  const double n1 = sqrt(H[0] * H[0] + H[3] * H[3] + H[6] * H[6]), n2 = sqrt(H[1] * H[1] + H[4] * H[4] + H[7] * H[7]);
  if (!(n1 > 0.0) || !(n2 > 0.0) || !(fabs(depth) > 0.0)) return false;
  const double s = (depth > 0.0 ? 1.0 : -1.0) / sqrt(n1 * n2);
  const double r1[3] = {s * H[0], s * H[3], s * H[6]}, r2[3] = {s * H[1], s * H[4], s * H[7]};
  double r3[3];
  cross3(r1, r2, r3);
  double Rh[9] = {r1[0], r2[0], r3[0], r1[1], r2[1], r3[1], r1[2], r2[2], r3[2]};
  if (!nearest_rotation(Rh)) return false;
  const double th[3] = {s * H[2], s * H[5], s * H[8]};
  // plane coordinates -> board frame: X_cam = Rh E^T (X - o) + th
  mat3_mul(Rh, plane + 3, R);
  double Ro[3];
  mat3_vec(R, plane, Ro);
  t[0] = th[0] - Ro[0];
  t[1] = th[1] - Ro[1];
  t[2] = th[2] - Ro[2];
  MCBA_UNROLL
  for (int i = 0; i < 9; ++i)
    if (!(fabs(R[i]) <= 2.0)) return false;
  return fabs(t[0]) < 1e300 && fabs(t[1]) < 1e300 && fabs(t[2]) < 1e300;
}

// ---------------------------------------------------------------------------------------------------------
// Levenberg-Marquardt refinement of p = (rotation vector | translation)
// ---------------------------------------------------------------------------------------------------------
// normal equations at p in the parameters themselves: Hf [36], g [6], cost (sum of squared pixel distances)
template <class Pts, class Red>
MCBA_HD void lm_linearize(const Pts& pts, const Red& red, double fx, double fy, const double* p, double* Hf, double* g,
                          double* cost) {
  double R[9], L[9];
  rodrigues(p, R, L);
  const double tx = p[3], ty = p[4], tz = p[5];
  // 21 + 6 + 1 sums in the camera-frame basis E = A [-[R X]x | I]; the rotation columns take L afterwards
  double s[28];
  red.template sum<28>(pts, [&](int i, double* q) MCBA_TERMS {
    const double Xb[3] = {pts.X[i], pts.Y[i], pts.Z[i]};
    double Xr[3];
    mat3_vec(R, Xb, Xr);
    const double zc = Xr[2] + tz;
    const double iz = 1.0 / zc;
    const double px = (Xr[0] + tx) * iz, py = (Xr[1] + ty) * iz;
    const double rx = fx * (px - pts.x[i]), ry = fy * (py - pts.y[i]);
    const double a0[3] = {fx * iz, 0.0, -fx * px * iz}, a1[3] = {0.0, fy * iz, -fy * py * iz};
    double E[12];
    base_row(a0, Xr, E);
    base_row(a1, Xr, E + 6);
    int idx = 0;
    MCBA_UNROLL
    for (int r = 0; r < 6; ++r) {
      MCBA_UNROLL
      for (int c = r; c < 6; ++c) q[idx++] = E[r] * E[c] + E[6 + r] * E[6 + c];
    }
    MCBA_UNROLL
    for (int r = 0; r < 6; ++r) q[21 + r] = E[r] * rx + E[6 + r] * ry;
    q[27] = rx * rx + ry * ry;
  }, s);
  *cost = s[27];
  // T = diag(L, I):  H = T^T Hs T,  g = T^T gs
  double Hs[36], M[36];
  MCBA_UNROLL
  for (int r = 0; r < 6; ++r) {
    MCBA_UNROLL
    for (int c = r; c < 6; ++c) { Hs[r * 6 + c] = s[tri6(r, c)]; Hs[c * 6 + r] = s[tri6(r, c)]; }
  }
  MCBA_UNROLL
  for (int r = 0; r < 6; ++r) {      // M = Hs T
    MCBA_UNROLL
    for (int c = 0; c < 3; ++c) M[r * 6 + c] = Hs[r * 6] * L[c] + Hs[r * 6 + 1] * L[3 + c] + Hs[r * 6 + 2] * L[6 + c];
    MCBA_UNROLL
    for (int c = 3; c < 6; ++c) M[r * 6 + c] = Hs[r * 6 + c];
  }
  MCBA_UNROLL
  for (int c = 0; c < 6; ++c) {      // Hf = T^T M
    MCBA_UNROLL
    for (int r = 0; r < 3; ++r) Hf[r * 6 + c] = L[r] * M[c] + L[3 + r] * M[6 + c] + L[6 + r] * M[12 + c];
    MCBA_UNROLL
    for (int r = 3; r < 6; ++r) Hf[r * 6 + c] = M[r * 6 + c];
  }
  MCBA_UNROLL
  for (int r = 0; r < 3; ++r) g[r] = L[r] * s[21] + L[3 + r] * s[22] + L[6 + r] * s[23];
  MCBA_UNROLL
  for (int r = 3; r < 6; ++r) g[r] = s[21 + r];
}

template <class Pts, class Red>
MCBA_HD double view_sse(const Pts& pts, const Red& red, double fx, double fy, const double* p) {
  double R[9], L[9];
  rodrigues(p, R, L);
  double s[1];
  red.template sum<1>(pts, [&](int i, double* q) MCBA_TERMS {
    const double Xb[3] = {pts.X[i], pts.Y[i], pts.Z[i]};
    double Xr[3];
    mat3_vec(R, Xb, Xr);
    const double iz = 1.0 / (Xr[2] + p[5]);
    const double rx = fx * ((Xr[0] + p[3]) * iz - pts.x[i]), ry = fy * ((Xr[1] + p[4]) * iz - pts.y[i]);
    q[0] = rx * rx + ry * ry;
  }, s);
  return s[0];
}

// returns true when the step test was met within max_iter linearisations; *iters = linearisations used
template <class Pts, class Red>
MCBA_HD bool lm_refine(const Pts& pts, const Red& red, double fx, double fy, double* p, int max_iter, int* iters) {
  double H[36], g[6], cost;
  lm_linearize(pts, red, fx, fy, p, H, g, &cost);
  int used = 1;
  double lambda = 1e-3;
  bool converged = false;
  if (!(cost < 1e300)) { *iters = used; return false; }
  MCBA_NOUNROLL
  while (used < max_iter) {
    double Hd[36], rhs[6], d[6];
    MCBA_UNROLL
    for (int i = 0; i < 36; ++i) Hd[i] = H[i];
    MCBA_UNROLL
    for (int i = 0; i < 6; ++i) { Hd[i * 7] = H[i * 7] * (1.0 + lambda); rhs[i] = -g[i]; }
    if (!chol6_solve(Hd, rhs, d)) {
      lambda = lambda * 10.0 + 1e-12;
      if (!(lambda < 1e30)) break;
      ++used;   // (counted so that a singular system cannot spin)
      continue;
    }
    double q[6], dn = 0.0, pn = 0.0;
    MCBA_UNROLL
    for (int i = 0; i < 6; ++i) { q[i] = p[i] + d[i]; dn += d[i] * d[i]; pn += p[i] * p[i]; }
    if (sqrt(dn) <= LM_STEP_TOL * (sqrt(pn) + LM_STEP_TOL)) {
      MCBA_UNROLL
      for (int i = 0; i < 6; ++i) p[i] = q[i];
      converged = true;
      break;
    }
    double Hq[36], gq[6], cq;
    lm_linearize(pts, red, fx, fy, q, Hq, gq, &cq);
    ++used;
    if (cq <= cost * (1.0 + LM_ACCEPT_SLACK)) {
      MCBA_UNROLL
      for (int i = 0; i < 6; ++i) { p[i] = q[i]; g[i] = gq[i]; }
      MCBA_UNROLL
      for (int i = 0; i < 36; ++i) H[i] = Hq[i];
      cost = cq;
      lambda = fmax(lambda * 0.1, 1e-15);
    } else {
      lambda = fmin(lambda * 10.0, 1e30);
    }
  }
  *iters = used;
  return converged;
}

// ---------------------------------------------------------------------------------------------------------
// one view: container already loaded.  init: row-major 4x4 start pose or null (planar initialisation from `plane`).
// Outputs: pose [16] row-major, sse, corners used, status, LM linearisations.  Views that end without a pose are the identity.
// ---------------------------------------------------------------------------------------------------------
template <class Pts, class Red>
MCBA_HD void view_pose(const Pts& pts, const Red& red, const double* cam, const double* plane, const double* init, int max_iter,
                       double* pose, double* sse, int* n_used, int* status, int* iters) {
  MCBA_UNROLL
  for (int i = 0; i < 16; ++i) pose[i] = (i % 5 == 0) ? 1.0 : 0.0;
  *sse = 0.0;
  *iters = 0;
  double cnt[1];
  red.template sum<1>(pts, [&](int, double* q) MCBA_TERMS { q[0] = 1.0; }, cnt);
  const int n = (int)(cnt[0] + 0.5);
  *n_used = 0;
  if (n < MIN_CORNERS) { *status = ST_TOO_FEW; return; }
  double p[6], R[9], t[3];
  if (init != nullptr) {
    MCBA_UNROLL
    for (int r = 0; r < 3; ++r) {
      MCBA_UNROLL
      for (int c = 0; c < 3; ++c) R[3 * r + c] = init[4 * r + c];
      t[r] = init[4 * r + 3];
    }
  } else if (!planar_init(pts, red, plane, (double)n, R, t)) {
    *status = ST_DEGENERATE;
    return;
  }
  rotvec_of_matrix(R, p);
  p[3] = t[0]; p[4] = t[1]; p[5] = t[2];
  const double fx = cam[CAM_FX], fy = cam[CAM_FY];
  const bool ok = lm_refine(pts, red, fx, fy, p, max_iter, iters);
  const double cost = view_sse(pts, red, fx, fy, p);
  if (!(cost < 1e300)) { *status = ST_NOT_CONVERGED; return; }   // (non-finite: no pose to report)
  double L[9];
  rodrigues(p, R, L);
  MCBA_UNROLL
  for (int r = 0; r < 3; ++r) {
    MCBA_UNROLL
    for (int c = 0; c < 3; ++c) pose[4 * r + c] = R[3 * r + c];
    pose[4 * r + 3] = p[3 + r];
  }
  *sse = cost;
  *n_used = n;
  *status = ok ? ST_OK : ST_NOT_CONVERGED;
}

}  // namespace pnp
}  // namespace mcba
