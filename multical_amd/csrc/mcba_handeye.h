// mcba_handeye.h -- robot-world hand-eye calibration A_i X = Z B_i for a batch of independent problems (FP64 throughout).
//
// Restates cv2.calibrateRobotWorldHandEye(..., CALIB_ROBOT_WORLD_HAND_EYE_SHAH) as the reference calls it (hand_eye/hand_eye.py:
// 110-113 for every camera pair x board pair, transform/hand_eye.py:39-42 for HandEyeCalibration.initialise): Shah's closed form
// on "points-transforming" 4x4 poses.
//   rotations     R_Z = R_A R_X R_B^T for every pair; with row-major vec this is n vec(R_Z) = K vec(R_X), K = sum_i kron(R_A_i,
//                 R_B_i).  vec(R_X) / vec(R_Z) are the right / left singular vectors of K's largest singular value: v = leading
//                 eigenvector of K^T K (pnp::jacobi_eig<9>), u = K v / |K v|.  Each is reshaped to 3x3, scaled by
//                 sign(det) / |det|^(1/3) -- which also removes the joint sign ambiguity of (u, v) -- and projected to the nearest
//                 rotation (pnp::nearest_rotation).
//                 The 81 entries of K are those of G = sum_i vec(R_A_i) vec(R_B_i)^T in another order,
//                 K[3a + b][3c + d] = G[3a + c][3b + d]: the sum over the pairs is a [9 x n] [n x 9] product.
//   translations  R_A_i t_X - t_Z = R_Z t_B_i - t_A_i stacked over the pairs, 6 unknowns (t_X | t_Z): Cholesky of the normal
//                 matrix [[I, -M^T], [-M, I]], M = mean(R_A) (both sides divided by n, so the pivots are those of a unit-scale
//                 matrix whatever the number of pairs).
//   residual      err_i = |A_i X - Z B_i|_F (transform/hand_eye.py:47-50).
// Status rules (mcba.h: MCBA_HANDEYE_*):
//   TOO_FEW       fewer than 3 usable pairs -- the reference's own rule (hand_eye/hand_eye.py:94);
//   DEGENERATE    the rotations do not determine (X, Z): all equal (pure translations: K = n kron(R_A, R_B), nine equal singular
//                 values) or about one common axis (a one-parameter family of solutions: the leading singular value is multiple,
//                 and M keeps the axis, so I - M M^T is singular).  Tested as
//                   (l1 - l2) <= GAP_TOL l1      on the two largest eigenvalues of K^T K, or
//                   a pivot <= PIVOT_TOL         of the unit-scale 6x6 matrix,
//                 or a non-finite value anywhere in the result (non-finite input).  GAP_TOL = 1e-9: the eigenvalues carry rounding
//                 of about 1e-15 l1 and the leading vector an error of about 1e-16 l1 / (l1 - l2), so a gap at the threshold still
//                 gives 1e-7 -- anything closer is no estimate; a ring rig that turns ALMOST about one axis (sigma2 / sigma1 =
//                 0.99997 at the cfg5 fixtures: a gap of 6e-5) is far above it.  PIVOT_TOL = 1e-10 by the same reasoning for the
//                 translations (the smallest pivot of those fixtures is about 1e-5).
// Everything is MCBA_HD: k_hand_eye (mcba_handeye_kernels.h) runs one problem per wavefront, tests/handeye_host builds the same
// source with g++.  The sums over the pairs are the caller's: the device forms G by MFMA and the others as lane partials folded
// by the xor butterfly, the host build adds the pairs in frame order (or in reversed order).
#pragma once
#include <stdint.h>
#include "mcba_math.h"
#include "mcba_pnp.h"

namespace mcba {
namespace handeye {

// status byte of a problem (mcba.h: MCBA_HANDEYE_*)
constexpr int ST_OK = 0, ST_TOO_FEW = 1, ST_DEGENERATE = 2;
constexpr int MIN_PAIRS = 3;
constexpr double GAP_TOL = 1e-9;
constexpr double PIVOT_TOL = 1e-10;

// row-major 4x4 -> (R [9], t [3]); invert: the rigid inverse (R^T | -R^T t)
MCBA_HD void load_pose(const double* T, bool invert, double* R, double* t) {
  if (!invert) {
    MCBA_UNROLL
    for (int r = 0; r < 3; ++r) {
      MCBA_UNROLL
      for (int c = 0; c < 3; ++c) R[3 * r + c] = T[4 * r + c];
      t[r] = T[4 * r + 3];
    }
  } else {
    MCBA_UNROLL
    for (int r = 0; r < 3; ++r) {
      MCBA_UNROLL
      for (int c = 0; c < 3; ++c) R[3 * r + c] = T[4 * c + r];
      t[r] = -((T[r] * T[3] + T[4 + r] * T[7]) + T[8 + r] * T[11]);
    }
  }
}

MCBA_HD void store_pose(const double* R, const double* t, double* T) {
  MCBA_UNROLL
  for (int r = 0; r < 3; ++r) {
    MCBA_UNROLL
    for (int c = 0; c < 3; ++c) T[4 * r + c] = R[3 * r + c];
    T[4 * r + 3] = t[r];
    T[12 + r] = 0.0;
  }
  T[15] = 1.0;
}

using pnp::identity_pose;

// a 9-vector reshaped to 3x3 -> rotation: scale by sign(det) / |det|^(1/3), then the nearest rotation
MCBA_HD bool rotation_of_vec(const double* v, double* R) {
  const double det = v[0] * (v[4] * v[8] - v[5] * v[7]) - v[1] * (v[3] * v[8] - v[5] * v[6]) + v[2] * (v[3] * v[7] - v[4] * v[6]);
  if (!(fabs(det) > 1e-300) || !(fabs(det) < 1e300)) return false;
  const double s = (det > 0.0 ? 1.0 : -1.0) / cbrt(fabs(det));
  MCBA_UNROLL
  for (int i = 0; i < 9; ++i) R[i] = s * v[i];
  return pnp::nearest_rotation(R);
}

// G [81] = sum over the pairs of vec(R_A) vec(R_B)^T (row-major, G[9 i + j] = sum R_A[i] R_B[j]).
// K[r][c] of K = sum kron(R_A, R_B) in terms of G
MCBA_HD constexpr int k_index(int r, int c) { return 9 * (3 * (r / 3) + c / 3) + 3 * (r % 3) + c % 3; }

// v [9] = eigenvector of the largest eigenvalue of K^T K; false when the second largest does not stand clear of it
MCBA_HD bool leading_vector(const double* G, double* v) {
  double tri[45], V[81];
  MCBA_UNROLL
  for (int p = 0; p < 9; ++p) {
    MCBA_UNROLL
    for (int q = p; q < 9; ++q) {
      double s = 0.0;
      MCBA_UNROLL
      for (int r = 0; r < 9; ++r) s += G[k_index(r, p)] * G[k_index(r, q)];
      tri[pnp::tri_index(9, p, q)] = s;
    }
  }
  pnp::jacobi_eig<9>(tri, V);
  double l1 = tri[0], l2 = -1.0;
  MCBA_UNROLL
  for (int r = 0; r < 9; ++r) v[r] = V[r * 9];
  MCBA_UNROLL
  for (int k = 1; k < 9; ++k) {
    const double l = tri[pnp::tri_index(9, k, k)];
    if (l > l1) {
      l2 = l1;
      l1 = l;
      MCBA_UNROLL
      for (int r = 0; r < 9; ++r) v[r] = V[r * 9 + k];
    } else if (l > l2) {
      l2 = l;
    }
  }
  return l1 > 0.0 && l1 - l2 > GAP_TOL * l1;
}

// R_X from v, R_Z from u = K v (|K v| is not divided out: rotation_of_vec scales by the determinant)
MCBA_HD bool rotations_of_vector(const double* G, const double* v, double* RX, double* RZ) {
  double u[9];
  MCBA_UNROLL
  for (int r = 0; r < 9; ++r) {
    double s = 0.0;
    MCBA_UNROLL
    for (int c = 0; c < 9; ++c) s += G[k_index(r, c)] * v[c];
    u[r] = s;
  }
  return rotation_of_vec(v, RX) && rotation_of_vec(u, RZ);
}

// one pair's terms of the translation system: q[0..2] = R_A^T r, q[3..5] = r,  r = R_Z t_B - t_A
MCBA_HD void rhs_terms(const double* RA, const double* tA, const double* tB, const double* RZ, double* q) {
  double r[3];
  mat3_vec(RZ, tB, r);
  MCBA_UNROLL
  for (int k = 0; k < 3; ++k) r[k] -= tA[k];
  MCBA_UNROLL
  for (int k = 0; k < 3; ++k) {
    q[k] = (RA[k] * r[0] + RA[3 + k] * r[1]) + RA[6 + k] * r[2];
    q[3 + k] = r[k];
  }
}

// t_X, t_Z from sumRA [9] = sum R_A, rhs [6] = sum of rhs_terms, n pairs
MCBA_HD bool solve_translations(const double* sumRA, const double* rhs, double n, double* tX, double* tZ) {
  const double in = 1.0 / n;
  double H[36], b[6], x[6];
  MCBA_UNROLL
  for (int i = 0; i < 36; ++i) H[i] = 0.0;
  MCBA_UNROLL
  for (int i = 0; i < 6; ++i) H[7 * i] = 1.0;
  MCBA_UNROLL
  for (int r = 0; r < 3; ++r) {
    MCBA_UNROLL
    for (int c = 0; c < 3; ++c) {
      const double m = -sumRA[3 * r + c] * in;   // unknowns (t_X | t_Z): the block below the diagonal is -M
      H[6 * (3 + r) + c] = m;
      H[6 * c + 3 + r] = m;
    }
  }
  MCBA_UNROLL
  for (int k = 0; k < 3; ++k) { b[k] = rhs[k] * in; b[3 + k] = -rhs[3 + k] * in; }
  if (!pnp::chol6_solve(H, b, x, PIVOT_TOL)) return false;
  MCBA_UNROLL
  for (int k = 0; k < 3; ++k) { tX[k] = x[k]; tZ[k] = x[3 + k]; }
  return true;
}

// |A X - Z B|_F of one pair
MCBA_HD double pair_error(const double* RA, const double* tA, const double* RB, const double* tB, const double* RX,
                          const double* tX, const double* RZ, const double* tZ) {
  double L[9], Rr[9], l[3], r[3];
  mat3_mul(RA, RX, L);
  mat3_mul(RZ, RB, Rr);
  mat3_vec(RA, tX, l);
  mat3_vec(RZ, tB, r);
  double s = 0.0;
  MCBA_UNROLL
  for (int i = 0; i < 9; ++i) s += (L[i] - Rr[i]) * (L[i] - Rr[i]);
  MCBA_UNROLL
  for (int k = 0; k < 3; ++k) {
    const double d = (l[k] + tA[k]) - (r[k] + tZ[k]);
    s += d * d;
  }
  return sqrt(s);
}

MCBA_HD bool all_finite(const double* a, int n) {
  bool ok = true;
  for (int i = 0; i < n; ++i) ok = ok && (fabs(a[i]) < 1e300);
  return ok;
}

}  // namespace handeye
}  // namespace mcba
