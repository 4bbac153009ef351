// mcba_warp.h -- the residual field applied as a warp of the image plane, shared by the kernels
// (mcba_warp_kernels.h) and the g++ build the tests compare them with (tests/correction_host).
//
// DEFINITIONS (they decide every sign):
//   field          e_c(u, v) = sum_k b_k(u, v) coef[c][k][:], the fit of mcba_residual_gram's rows: grid nx x ny over the image
//                  (W_c, H_c), spline_cell / cubic_weights / column a (nx + 3) + b of mcba_residual_field.h.  It was fitted to
//                  r = projected - observed as a function of the OBSERVED pixel.
//   outside        outside the closed rectangle [0, W] x [0, H] the field is evaluated at the pixel clamped to it: a constant,
//                  continuous extension whose derivative in the clamped direction is zero.
//   forward warp   raw -> corrected:  w(p) = p + e(p).  Since r = projected - observed, the corrected observation is what the
//                  parametric model predicts.
//   inverse warp   corrected -> raw:  solve p + e(p) = q by Newton with the analytic Jacobian I + De(p), start p = q - e(q), stop
//                  at max |dp| <= 1e-11 px, at most 50 steps.  Non-finite input: NaN, NOT_CONVERGED.
//   fold bound     L = max over the two components of max |D_x coef| nx / W + max |D_y coef| ny / H (D: first difference of
//                  neighbouring control values) bounds the infinity norm of De everywhere.  Below FOLD_LIMIT = 0.2 the Newton map
//                  contracts by 2 L / (1 - L) <= 0.5 a step from any start; a field at or above it is refused by the callers.
//   corrected      project_corrected(X) = w^-1(pi(X)), undistort_corrected(p) = pi^-1(w(p)); the source coordinate of destination
//   camera         pixel (u, v) of a corrected map is w^-1(pi(iR [u v 1])), FP64 throughout, rounded ONCE to float32.
//
// Host and device evaluate with the SAME roundings: every multiply-add of the field, its Jacobian and the Newton step is an explicit
// fma, every other statement holds a single operation, so neither -ffp-contract=on nor =off changes a bit.  (The projection that
// feeds map_coordinate_corrected is the existing one, with the roundings it has in each build.)
#pragma once
#include <stdint.h>
#include "mcba_residual_field.h"
#include "mcba_undistort.h"

namespace mcba {
namespace warp {

constexpr int MAX_K = resfield::MAX_NC - 2;        // control points of a camera: (nx + 3)(ny + 3) <= 62
constexpr int ST_OK = 0, ST_NOT_CONVERGED = 1;     // mcba.h: MCBA_UNDISTORT_*
constexpr int MAX_STEPS = 50;
constexpr double STEP_TOL = 1e-11;                 // px
constexpr double FOLD_LIMIT = 0.2;

// one camera's field: coef [K][2] (global memory, LDS or host), the image extent and the grid
struct Field {
  const double* coef;
  double W, H;
  int nx, ny;
};

MCBA_HD double clamp_to(double u, double hi) { return u < 0.0 ? 0.0 : (u > hi ? hi : u); }

// d/dt of cubic_weights
MCBA_HD void cubic_weight_derivatives(double t, double d[4]) {
  const double m = 1.0 - t;
  const double mm = m * m;
  const double tt = t * t;
  d[0] = -0.5 * mm;
  d[1] = fma(1.5, tt, -2.0 * t);
  d[2] = fma(-1.5, tt, t + 0.5);
  d[3] = 0.5 * tt;
}

// sum_a wy[a] sum_b wx[b] coef[(iy + a)(nx + 3) + ix + b][comp]: along a row of control points first, then down the four rows
MCBA_HD double tensor_sum(const double* coef, int first, int row_stride, int comp, const double wx[4], const double wy[4]) {
  double s = 0.0;
  MCBA_UNROLL
  for (int a = 0; a < 4; ++a) {
    const double* p = coef + 2 * (first + a * row_stride) + comp;
    double r = wx[0] * p[0];
    r = fma(wx[1], p[2], r);
    r = fma(wx[2], p[4], r);
    r = fma(wx[3], p[6], r);
    s = a == 0 ? wy[0] * r : fma(wy[a], r, s);
  }
  return s;
}

// e(u, v) of finite (u, v)
MCBA_HD void field_value(const Field& f, double u, double v, double e[2]) {
  const resfield::Cell cx = resfield::spline_cell(clamp_to(u, f.W), f.W, f.nx), cy = resfield::spline_cell(clamp_to(v, f.H), f.H, f.ny);
  double wx[4], wy[4];
  resfield::cubic_weights(cx.t, wx);
  resfield::cubic_weights(cy.t, wy);
  const int first = cy.i * (f.nx + 3) + cx.i;
  e[0] = tensor_sum(f.coef, first, f.nx + 3, 0, wx, wy);
  e[1] = tensor_sum(f.coef, first, f.nx + 3, 1, wx, wy);
}

// e and De = [de_x/du de_x/dv; de_y/du de_y/dv] (row-major J[4]) of finite (u, v); strictly outside the rectangle the derivative in the
// clamped direction is zero, on its edges it is the one-sided derivative from inside
MCBA_HD void field_value_jacobian(const Field& f, double u, double v, double e[2], double J[4]) {
  const resfield::Cell cx = resfield::spline_cell(clamp_to(u, f.W), f.W, f.nx), cy = resfield::spline_cell(clamp_to(v, f.H), f.H, f.ny);
  double wx[4], wy[4], dx[4], dy[4];
  resfield::cubic_weights(cx.t, wx);
  resfield::cubic_weights(cy.t, wy);
  cubic_weight_derivatives(cx.t, dx);
  cubic_weight_derivatives(cy.t, dy);
  const double nxd = (double)f.nx, nyd = (double)f.ny;
  const double sx = (u < 0.0 || u > f.W) ? 0.0 : nxd / f.W;
  const double sy = (v < 0.0 || v > f.H) ? 0.0 : nyd / f.H;
  MCBA_UNROLL
  for (int i = 0; i < 4; ++i) {
    dx[i] = dx[i] * sx;
    dy[i] = dy[i] * sy;
  }
  const int first = cy.i * (f.nx + 3) + cx.i, stride = f.nx + 3;
  MCBA_UNROLL
  for (int comp = 0; comp < 2; ++comp) {
    e[comp] = tensor_sum(f.coef, first, stride, comp, wx, wy);
    J[2 * comp] = tensor_sum(f.coef, first, stride, comp, dx, wy);
    J[2 * comp + 1] = tensor_sum(f.coef, first, stride, comp, wx, dy);
  }
}

// L of one camera (see the head of the file); finite coefficients are the caller's business
MCBA_HD double fold_bound(const double* coef, int nx, int ny, double W, double H) {
  const int gx = nx + 3, gy = ny + 3;
  const double kx = (double)nx / W, ky = (double)ny / H;
  double L = 0.0;
  for (int comp = 0; comp < 2; ++comp) {
    double mx = 0.0, my = 0.0;
    for (int a = 0; a < gy; ++a)
      for (int b = 0; b < gx; ++b) {
        const double c0 = coef[2 * (a * gx + b) + comp];
        if (b + 1 < gx) {
          const double d = fabs(coef[2 * (a * gx + b + 1) + comp] - c0);
          if (d > mx) mx = d;
        }
        if (a + 1 < gy) {
          const double d = fabs(coef[2 * ((a + 1) * gx + b) + comp] - c0);
          if (d > my) my = d;
        }
      }
    const double l = fma(mx, kx, my * ky);
    if (l > L) L = l;
  }
  return L;
}

// raw -> corrected
MCBA_HD int warp_forward(const Field& f, double u, double v, double out[2]) {
  if (!undistort::finite_d(u) || !undistort::finite_d(v)) {
    out[0] = out[1] = undistort::quiet_nan();
    return ST_NOT_CONVERGED;
  }
  double e[2];
  field_value(f, u, v, e);
  out[0] = u + e[0];
  out[1] = v + e[1];
  return ST_OK;
}

// corrected -> raw
MCBA_HD int warp_inverse(const Field& f, double qu, double qv, double out[2]) {
  if (!undistort::finite_d(qu) || !undistort::finite_d(qv)) {
    out[0] = out[1] = undistort::quiet_nan();
    return ST_NOT_CONVERGED;
  }
  double e[2], J[4];
  field_value(f, qu, qv, e);
  double pu = qu - e[0], pv = qv - e[1];
  for (int it = 0; it < MAX_STEPS; ++it) {
    field_value_jacobian(f, pu, pv, e, J);
    const double du = pu - qu, dv = pv - qv;
    const double gu = du + e[0], gv = dv + e[1];               // g = p + e(p) - q
    const double a = 1.0 + J[0], b = J[1], c = J[2], d = 1.0 + J[3];
    const double bc = b * c;
    const double det = fma(a, d, -bc);
    const double bgv = b * gv, cgu = c * gu;
    const double su = fma(d, gu, -bgv) / det;                  // (I + De)^-1 g
    const double sv = fma(a, gv, -cgu) / det;
    const double nu = pu - su, nv = pv - sv;
    // (beyond about 1e5 px half a unit in the last place of p exceeds STEP_TOL: a step that no longer moves p is the end as well)
    const bool done = (fabs(su) <= STEP_TOL && fabs(sv) <= STEP_TOL) || (nu == pu && nv == pv);
    pu = nu;
    pv = nv;
    if (done) {
      out[0] = pu;
      out[1] = pv;
      return ST_OK;
    }
  }
  out[0] = out[1] = undistort::quiet_nan();
  return ST_NOT_CONVERGED;
}

// source coordinate of destination pixel (u, v) of the corrected camera: w^-1(pi(iR [u v 1])) in FP64, each coordinate rounded once
// to float32.  The FP64 body is that of undistort::map_coordinate, statement for statement; w <= 0, a non-finite projection or an
// inverse warp that does not converge: (NaN, NaN), which remap_pixel turns into the border value.
MCBA_HD void map_coordinate_corrected(const double* cam, int nd, bool fisheye, const double* iR, const Field& f, double u, double v,
                                      float& mx, float& my) {
  double X[3], uv[2], p[2];
  X[0] = iR[0] * u + iR[1] * v + iR[2];
  X[1] = iR[3] * u + iR[4] * v + iR[5];
  X[2] = iR[6] * u + iR[7] * v + iR[8];
  if (!(X[2] > 0.0)) { mx = my = (float)undistort::quiet_nan(); return; }
  undistort::project_any(cam, nd, fisheye, X, uv);
  if (!undistort::finite_d(uv[0]) || !undistort::finite_d(uv[1])) { mx = my = (float)undistort::quiet_nan(); return; }
  if (warp_inverse(f, uv[0], uv[1], p) != ST_OK) { mx = my = (float)undistort::quiet_nan(); return; }
  mx = (float)p[0];
  my = (float)p[1];
}

#if !defined(__HIPCC__)
// The specification of the entry points as sequential loops.  size [C][2] (W, H) as doubles, coef [C][K][2].
inline Field host_field(const double* size, const double* coef, int nx, int ny, int c) {
  return Field{coef + (size_t)c * resfield::n_control(nx, ny) * 2, size[2 * c], size[2 * c + 1], nx, ny};
}

// mcba_warp_points: out [n][2], status [n] or null
inline void host_warp_points(const double* size, const double* coef, int nx, int ny, long long n, const int32_t* camera_of, int inverse,
                             const double* uv, double* out, uint8_t* status) {
  for (long long i = 0; i < n; ++i) {
    const Field f = host_field(size, coef, nx, ny, camera_of ? camera_of[i] : 0);
    const int st = inverse ? warp_inverse(f, uv[2 * i], uv[2 * i + 1], out + 2 * i) : warp_forward(f, uv[2 * i], uv[2 * i + 1], out + 2 * i);
    if (status) status[i] = (uint8_t)st;
  }
}

// mcba_undistort_maps_corrected: cam [C][CAM_STRIDE], nd, fish [C], iR [C][9] -> maps [C][height][width][2]
inline void host_warp_maps(int C, const double* cam, const int32_t* nd, const uint8_t* fish, const double* iR, const double* size,
                           const double* coef, int nx, int ny, int width, int height, float* maps) {
  for (int c = 0; c < C; ++c) {
    const Field f = host_field(size, coef, nx, ny, c);
    for (int y = 0; y < height; ++y)
      for (int x = 0; x < width; ++x) {
        float* m = maps + (((size_t)c * height + y) * width + x) * 2;
        map_coordinate_corrected(cam + (size_t)c * CAM_STRIDE, nd[c], fish[c] != 0, iR + 9 * (size_t)c, f, (double)x, (double)y, m[0], m[1]);
      }
  }
}
#endif

}  // namespace warp
}  // namespace mcba
