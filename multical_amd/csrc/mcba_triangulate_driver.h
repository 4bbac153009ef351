// mcba_triangulate_driver.h -- host side of mcba_triangulate that does not touch the device: argument checks and the camera entries
// with what the staged records read from their spare slots.  Shared by the driver (mcba_triangulate.hip) and the host build of the
// mathematics (tests/triangulate_host), so that both refuse the same calls with the same messages.
#pragma once
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/mcba.h"
#include "mcba_triangulate.h"
#include "mcba_undistort_driver.h"

namespace mcba {
namespace triangulate {

static_assert(MAX_CAMERAS == MCBA_TRI_MAX_CAMERAS, "mcba.h states the limit of the LDS staging");
static_assert(ST_OK == MCBA_TRI_OK && ST_TOO_FEW == MCBA_TRI_TOO_FEW && ST_DEGENERATE == MCBA_TRI_DEGENERATE &&
              ST_NOT_CONVERGED == MCBA_TRI_NOT_CONVERGED && ST_BEHIND == MCBA_TRI_BEHIND, "mcba.h states the status bytes");

// checks the call and fills cam [C][CAM_STRIDE]; *n_points = F * M (0: nothing to do, the outputs are not looked at)
inline bool plan_problem(const mcba_triangulate_problem* p, const double* X, const uint8_t* status, std::vector<double>& cam,
                         int64_t* n_points, std::string& err) {
  const char* who = "mcba_triangulate";
  const std::string w(who);
  if (!p) { err = w + ": null argument"; return false; }
  undistort::CameraPlan plan;
  if (!undistort::plan_cameras(&p->cams, who, plan, err)) return false;
  const int C = p->cams.C;
  if (C > MAX_CAMERAS) {
    char msg[160];
    snprintf(msg, sizeof msg, "%s: %d cameras, at most %d are served (the records of a frame are staged in LDS)", who, C, MAX_CAMERAS);
    err = msg;
    return false;
  }
  if (p->F < 0 || p->M < 0) { err = w + ": negative size"; return false; }
  if (!(p->sigma_px == p->sigma_px) || p->sigma_px - p->sigma_px != 0.0) { err = w + ": sigma_px must be finite"; return false; }
  if (p->views_end && !p->image_heights) { err = w + ": views_end needs image_heights (the scan time is v / height)"; return false; }
  if (p->views_end)
    for (int c = 0; c < C; ++c)
      if (!(p->image_heights[c] > 0.0)) { err = w + ": image heights must be positive"; return false; }
  *n_points = (int64_t)p->F * p->M;
  if (*n_points == 0) return true;
  if (!p->views || !p->points || !p->valid || !X || !status) { err = w + ": null argument"; return false; }
  cam = plan.cam;
  for (int c = 0; c < C; ++c) {
    double* e = cam.data() + (size_t)c * CAM_STRIDE;
    e[CAM_HEIGHT] = p->views_end ? p->image_heights[c] : 0.0;
    e[CAM_ISFISH] = plan.cam_fish[c] ? 1.0 : 0.0;
    e[REC_ND] = (double)plan.cam_nd[c];
  }
  return true;
}

}  // namespace triangulate
}  // namespace mcba
