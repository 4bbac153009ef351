// mcba_uncertainty.h -- how far a calibration can be trusted at a pixel where no board ever was: the 2 x 2 covariance of a projected
// point under the covariance of the shared parameters.
//
// A job is (camera b, reference, inverse distance rho, W).  A query is a pixel q.
//   reference = rig frame    the point X_rig = T_b^-1 (n_b(q) / rho) is fixed in the rig frame; intrinsics and pose of b vary.
//   reference = camera a     camera a sees the point at q at distance 1 / rho; everything of a and of b varies.
// n(q) is the UNIT ray of the pixel through the exact Newton inverse (pnp::undistort_point).  The scaled point Y = rho X is what is
// carried: the projection does not depend on the scale of its argument and its derivative A(X) = rho A(Y), so translation columns
// carry a factor rho and rho = 0 (directions only) is no special case.
// The row pair J (2 x KP) is never materialised by the query.  Its columns, in the fixed order of the job's W:
//   [COL_CAM_B, +18)   fx fy cx cy k0..k13 of b       Kc_b                                (project_point<ND, FISH, true>)
//   [COL_POSE_B, +6)   left perturbation of T_b       A_b [ -[Y_b]x | rho I ]             (base_rows with the scaled point)
//   [COL_POSE_A, +6)   left perturbation of T_a       A_b R_ba [ [Y_a]x | -rho I ]
//   [COL_CAM_A, +18)   fx fy cx cy k0..k13 of a       -A_b R_ba D (A_xy^-1 Kc_a): the implicit derivative of the inverse at its
//                                                     solution, D = d n / d(x, y) = (I - n n^T) [e_x e_y] / |(x, y, 1)|
// (a camera's coefficients beyond its own count have J = 0 exactly).  Stored parameters (rotation vectors, the single focal length
// of fix_aspect) enter through W alone: the caller folds d(column) / d(stored parameter) into it, so W^T is [r][KP] and
// C = J W W^T J^T = z z^T with z = J W -- positive semi-definite by construction.  Per column w of W the response is
//   s = Kc_b w_b + A_b dY,   dY = omega_b x Y_b + rho tau_b + R_ba (Y_a x omega_a - rho tau_a - D (A_xy^-1 Kc_a) w_a)
// and C accumulates (s0^2, s0 s1, s1^2).  A column flagged unconstrained (unobserved and not held) with a non-zero entry of J
// makes the prediction unconstrained: NaN and a status of its own.
// MCBA_HD like mcba_pnp.h: k_projection_uncertainty (mcba_uncertainty_kernels.h) and tests/uncertainty_host compile this source.
#pragma once
#include <stdint.h>
#include "mcba_undistort.h"

namespace mcba {
namespace uncertainty {

constexpr int ST_OK = 0, ST_NOT_CONVERGED = 1, ST_BEHIND = 2, ST_UNCONSTRAINED = 3;   // mcba.h: MCBA_UNC_*
constexpr int KI = 4 + MAX_DIST;                 // columns of a camera: fx fy cx cy | 14 coefficients
constexpr int COL_CAM_B = 0, COL_POSE_B = KI, COL_POSE_A = KI + 6, COL_CAM_A = KI + 12;
constexpr int KP = 2 * KI + 12;                  // 48: mcba.h: MCBA_UNC_MAX_K
constexpr int KP_RIG = KI + 6;                   // the columns a job without a reference camera has
constexpr int MAX_RANK = KP;                     // columns of W

// The record of a job, as the kernel stages it in LDS and the host build in a vector: the two camera entries (whose spare slots
// carry what the entry lacks), R_ba | t_ba, the scalars, then W^T.
constexpr int REC_CAM_B = 0, REC_CAM_A = CAM_STRIDE, REC_R = 2 * CAM_STRIDE, REC_T = REC_R + 9, REC_RHO = REC_T + 3,
              REC_HAS_A = REC_RHO + 1, REC_RANK = REC_HAS_A + 1, REC_LOOSE = REC_RANK + 1, REC_W = 128;
// W^T holds REC_LOOSE unit columns e_k first, one per unconstrained column k of J, then the REC_RANK columns of W: at most MAX_RANK
// together (an unconstrained column has a zero row in W, so a W of full column rank leaves the room)
constexpr int REC_STRIDE = REC_W + MAX_RANK * KP;   // 2432 doubles = 19 KiB, of which REC_W + (loose + rank) * KP are staged
constexpr int REC_ND = 49;                       // spare slot of a camera_entry: the camera's own coefficient count
static_assert(REC_LOOSE < REC_W && REC_ND > CAM_ISFISH && REC_ND < CAM_STRIDE, "the header of a job record");

struct Result {
  double uu, uv, vv, std;
  int status;
};

// larger eigenvalue of (uu uv; uv vv), the formula of the per-observation covariance (mcba.h states it): one operation per
// statement, nothing for a compiler to contract
MCBA_HD double sym2_max_eig(double uu, double uv, double vv) {
  const double sum = uu + vv;
  const double dif = uu - vv;
  const double hs = 0.5 * sum;
  const double hd = 0.5 * dif;
  const double a = hd * hd;
  const double b = uv * uv;
  const double ab = a + b;
  const double r = sqrt(ab);
  return hs + r;
}
MCBA_HD double std_of(double uu, double uv, double vv) { return sqrt(fmax(sym2_max_eig(uu, uv, vv), 0.0)); }

// pixel, A = d(u, v) / dX and Kc padded to 2 x KI (row stride KI) through the camera's own family
template <int ND, int FISH>
MCBA_HD void project_padded_as(const double* cam, const double* X, double* uv, double* A, double* K) {
  double Kc[2 * (4 + ND)];
  project_point<ND, FISH, true>(cam, cam + CAM_TILT, X, uv, A, Kc);
  MCBA_UNROLL
  for (int i = 0; i < KI; ++i) {
    K[i] = i < 4 + ND ? Kc[i < 4 + ND ? i : 0] : 0.0;
    K[KI + i] = i < 4 + ND ? Kc[i < 4 + ND ? 4 + ND + i : 0] : 0.0;
  }
}
MCBA_HD bool project_padded(const double* cam, const double* X, double* uv, double* A, double* K) {
  if (cam[CAM_ISFISH] != 0.0) { project_padded_as<4, 1>(cam, X, uv, A, K); return true; }
  switch ((int)cam[REC_ND]) {
    case 4: project_padded_as<4, 0>(cam, X, uv, A, K); return true;
    case 5: project_padded_as<5, 0>(cam, X, uv, A, K); return true;
    case 8: project_padded_as<8, 0>(cam, X, uv, A, K); return true;
    case 12: project_padded_as<12, 0>(cam, X, uv, A, K); return true;
    case 14: project_padded_as<14, 0>(cam, X, uv, A, K); return true;
    default: return false;        // (plan_cameras lets no other family through)
  }
}

// what a query keeps of its two projections
struct Pieces {
  double Kb[2 * KI];      // Kc_b
  double Ab[6];           // A_b at the scaled point
  double Yb[3], Ya[3];    // scaled points (Ya: the unit ray of the reference camera)
  double Ma[2 * KI];      // A_xy^-1 Kc_a
  double Dx[3], Dy[3];    // d n_a / dx, d n_a / dy
};

// status, and the pieces where it is OK.  rec: the job's record
MCBA_HD int prepare(const double* rec, double u, double v, Pieces& p) {
  const double* cb = rec + REC_CAM_B;
  const double* ca = rec + REC_CAM_A;
  const bool has_a = rec[REC_HAS_A] != 0.0;
  const double* src = has_a ? ca : cb;
  double x, y;
  if (!pnp::undistort_point(src, (int)src[REC_ND], src[CAM_ISFISH] != 0.0, u, v, x, y)) return ST_NOT_CONVERGED;
  const double inv = 1.0 / sqrt(x * x + y * y + 1.0);
  const double n[3] = {x * inv, y * inv, inv};
  double uvb[2];
  if (!has_a) {
    p.Yb[0] = n[0]; p.Yb[1] = n[1]; p.Yb[2] = n[2];
    if (!project_padded(cb, p.Yb, uvb, p.Ab, p.Kb)) return ST_NOT_CONVERGED;
    return ST_OK;
  }
  const double* R = rec + REC_R;
  const double* t = rec + REC_T;
  const double rho = rec[REC_RHO];
  MCBA_UNROLL
  for (int i = 0; i < 3; ++i) {
    p.Ya[i] = n[i];
    p.Yb[i] = R[3 * i] * n[0] + R[3 * i + 1] * n[1] + R[3 * i + 2] * n[2] + rho * t[i];
  }
  if (!(p.Yb[2] > 0.0)) return ST_BEHIND;
  // implicit derivative of a's inverse at its solution (x, y, 1)
  const double P1[3] = {x, y, 1.0};
  double uva[2], Aa[6];
  if (!project_padded(ca, P1, uva, Aa, p.Ma)) return ST_NOT_CONVERGED;
  const double det = Aa[0] * Aa[4] - Aa[1] * Aa[3];
  if (!(det > 0.0)) return ST_NOT_CONVERGED;
  const double i00 = Aa[4] / det, i01 = -Aa[1] / det, i10 = -Aa[3] / det, i11 = Aa[0] / det;
  MCBA_UNROLL
  for (int i = 0; i < KI; ++i) {
    const double k0 = p.Ma[i], k1 = p.Ma[KI + i];
    p.Ma[i] = i00 * k0 + i01 * k1;
    p.Ma[KI + i] = i10 * k0 + i11 * k1;
  }
  // n = (x, y, 1) inv:  d n / dx = e_x inv - n (n_x inv)
  p.Dx[0] = inv - n[0] * n[0] * inv; p.Dx[1] = -n[1] * n[0] * inv; p.Dx[2] = -n[2] * n[0] * inv;
  p.Dy[0] = -n[0] * n[1] * inv; p.Dy[1] = inv - n[1] * n[1] * inv; p.Dy[2] = -n[2] * n[1] * inv;
  if (!project_padded(cb, p.Yb, uvb, p.Ab, p.Kb)) return ST_NOT_CONVERGED;
  // b's model must be monotone where the point lands: det d(u, v) / d(X, Y) > 0, the test of the Newton inverse
  if (!(p.Ab[0] * p.Ab[4] - p.Ab[1] * p.Ab[3] > 0.0)) return ST_NOT_CONVERGED;
  return ST_OK;
}

// s = J w for one column; w(k): entry k of the column (k in the fixed order of the head of this file)
template <class Column>
MCBA_HD void response(const double* rec, const Pieces& p, const Column& w, double& s0, double& s1) {
  const double rho = rec[REC_RHO];
  double a0 = 0.0, a1 = 0.0;
  MCBA_UNROLL
  for (int i = 0; i < KI; ++i) {
    const double wi = w(COL_CAM_B + i);
    a0 += p.Kb[i] * wi;
    a1 += p.Kb[KI + i] * wi;
  }
  const double ob[3] = {w(COL_POSE_B), w(COL_POSE_B + 1), w(COL_POSE_B + 2)};
  double dY[3];
  cross3(ob, p.Yb, dY);
  MCBA_UNROLL
  for (int i = 0; i < 3; ++i) dY[i] += rho * w(COL_POSE_B + 3 + i);
  if (rec[REC_HAS_A] != 0.0) {
    double m0 = 0.0, m1 = 0.0;
    MCBA_UNROLL
    for (int i = 0; i < KI; ++i) {
      const double wi = w(COL_CAM_A + i);
      m0 += p.Ma[i] * wi;
      m1 += p.Ma[KI + i] * wi;
    }
    const double oa[3] = {w(COL_POSE_A), w(COL_POSE_A + 1), w(COL_POSE_A + 2)};
    double va[3];
    cross3(p.Ya, oa, va);
    MCBA_UNROLL
    for (int i = 0; i < 3; ++i) va[i] -= rho * w(COL_POSE_A + 3 + i) + p.Dx[i] * m0 + p.Dy[i] * m1;
    const double* R = rec + REC_R;
    MCBA_UNROLL
    for (int i = 0; i < 3; ++i) dY[i] += R[3 * i] * va[0] + R[3 * i + 1] * va[1] + R[3 * i + 2] * va[2];
  }
  s0 = a0 + (p.Ab[0] * dY[0] + p.Ab[1] * dY[1] + p.Ab[2] * dY[2]);
  s1 = a1 + (p.Ab[3] * dY[0] + p.Ab[4] * dY[1] + p.Ab[5] * dY[2]);
}

struct StoredColumn {        // a column of W as the record stores it: W^T, KP entries a column
  const double* w;
  MCBA_HD double operator()(int k) const { return w[k]; }
};
struct UnitColumn {          // e_k: the response is column k of J
  int k;
  MCBA_HD double operator()(int i) const { return i == k ? 1.0 : 0.0; }
};

MCBA_HD int columns_of(const double* rec) { return rec[REC_HAS_A] != 0.0 ? KP : KP_RIG; }

// one query
MCBA_HD void query(const double* rec, double u, double v, Result& out) {
  const double nan = undistort::quiet_nan();
  out.uu = out.uv = out.vv = out.std = nan;
  Pieces p;
  out.status = prepare(rec, u, v, p);
  if (out.status != ST_OK) return;
  const int loose = (int)rec[REC_LOOSE], columns = loose + (int)rec[REC_RANK];
  double uu = 0.0, uv = 0.0, vv = 0.0;
  bool unconstrained = false;
  MCBA_NOUNROLL
  for (int j = 0; j < columns; ++j) {
    double s0, s1;
    response(rec, p, StoredColumn{rec + REC_W + j * KP}, s0, s1);
    if (j < loose) {                                    // (uniform) column k of J itself: it must vanish
      unconstrained = unconstrained || s0 != 0.0 || s1 != 0.0;
    } else {
      uu += s0 * s0;
      uv += s0 * s1;
      vv += s1 * s1;
    }
  }
  if (unconstrained) { out.status = ST_UNCONSTRAINED; return; }
  out.uu = uu; out.uv = uv; out.vv = vv;
  out.std = std_of(uu, uv, vv);
}

// tests: the row pair J [2][KP] of a query (columns past columns_of(rec) are 0); the status of prepare()
MCBA_HD int query_rows(const double* rec, double u, double v, double* J) {
  for (int i = 0; i < 2 * KP; ++i) J[i] = 0.0;
  Pieces p;
  const int status = prepare(rec, u, v, p);
  if (status != ST_OK) return status;
  const int K = columns_of(rec);
  for (int k = 0; k < K; ++k) response(rec, p, UnitColumn{k}, J[k], J[KP + k]);
  return status;
}

// query i of a grid of gw columns: centre (u0 + ix du, v0 + iy dv), each a product and a sum rounded on their own (a list of the
// same coordinates computed in IEEE double arithmetic holds the same bits)
MCBA_HD void grid_pixel(long long i, int gw, double u0, double v0, double du, double dv, double& u, double& v) {
  const long long iy = i / gw, ix = i - iy * gw;
  const double ou = (double)ix * du;
  const double ov = (double)iy * dv;
  u = u0 + ou;
  v = v0 + ov;
}

}  // namespace uncertainty
}  // namespace mcba
