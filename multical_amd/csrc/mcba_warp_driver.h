// mcba_warp_driver.h -- host side of the corrected entry points that does not touch the device: the checks of a mcba_field_set and
// its tables.  Shared by the driver (mcba_warp.hip) and the host build of the mathematics (tests/correction_host), so that both
// serve the same calls with the same refusals.
#pragma once
#include <math.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/mcba.h"
#include "mcba_undistort_driver.h"
#include "mcba_warp.h"

namespace mcba {
namespace warp {

struct FieldPlan {
  int C = 0, nx = 0, ny = 0, K = 0;
  std::vector<double> size;         // [C][2] W, H
  std::vector<double> coef;         // [C][K][2]
  std::vector<double> L;            // [C] fold bound of every camera
};

// cameras: the camera count the field set must have, or < 0 = any
inline bool plan_fields(const mcba_field_set* f, int cameras, const char* who, FieldPlan& out, std::string& err) {
  const std::string w(who);
  char msg[200];
  if (!f || f->C <= 0 || !f->image_size || !f->coef) { err = w + ": no field set"; return false; }
  if (cameras >= 0 && f->C != cameras) {
    snprintf(msg, sizeof msg, "%s: the field set has %d cameras, the camera set %d", who, (int)f->C, cameras);
    err = msg;
    return false;
  }
  if (f->nx < 1 || f->ny < 1) { err = w + ": nx and ny must be at least 1"; return false; }
  if ((long long)(f->nx + 3) * (f->ny + 3) > MAX_K) {
    snprintf(msg, sizeof msg, "%s: %d x %d intervals need %lld control points, more than %d", who, (int)f->nx, (int)f->ny,
             (long long)(f->nx + 3) * (f->ny + 3), MAX_K);
    err = msg;
    return false;
  }
  out.C = f->C; out.nx = f->nx; out.ny = f->ny; out.K = resfield::n_control(f->nx, f->ny);
  out.size.resize((size_t)f->C * 2);
  out.L.resize(f->C);
  for (int c = 0; c < f->C; ++c) {
    if (f->image_size[2 * c] <= 0 || f->image_size[2 * c + 1] <= 0) {
      snprintf(msg, sizeof msg, "%s: image size of camera %d is not positive", who, c);
      err = msg;
      return false;
    }
    out.size[2 * c] = (double)f->image_size[2 * c];
    out.size[2 * c + 1] = (double)f->image_size[2 * c + 1];
  }
  const size_t n = (size_t)f->C * out.K * 2;
  for (size_t i = 0; i < n; ++i)
    if (!undistort::finite_d(f->coef[i])) {
      snprintf(msg, sizeof msg, "%s: a coefficient of camera %d is not finite", who, (int)(i / ((size_t)out.K * 2)));
      err = msg;
      return false;
    }
  out.coef.assign(f->coef, f->coef + n);
  for (int c = 0; c < f->C; ++c) {
    out.L[c] = fold_bound(f->coef + (size_t)c * out.K * 2, f->nx, f->ny, out.size[2 * c], out.size[2 * c + 1]);
    if (!(out.L[c] < FOLD_LIMIT)) {
      snprintf(msg, sizeof msg, "%s: the field folds the image: fold bound %.4f of camera %d is not below %.1f", who, out.L[c], c,
               FOLD_LIMIT);
      err = msg;
      return false;
    }
  }
  return true;
}

}  // namespace warp
}  // namespace mcba
