// mcba_localize_driver.h -- host side of mcba_rig_poses that does not touch the device: argument checks, the camera records, the
// world points W = board_pose X, the frame-major observation records and -- for a call without `init` -- the list of the views whose
// pose the start is taken from.  Shared by the driver (mcba_localize.hip) and the host build of the mathematics (tests/localize_host),
// so that both refuse the same calls with the same messages and walk the same records.
#pragma once
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/mcba.h"
#include "mcba_localize.h"
#include "mcba_pnp_driver.h"
#include "mcba_undistort_driver.h"

namespace mcba {
namespace localize {

static_assert(MAX_CAMERAS == MCBA_RIG_MAX_CAMERAS, "mcba.h states the limit of the LDS staging");
static_assert(ST_OK == MCBA_RIG_OK && ST_TOO_FEW == MCBA_RIG_TOO_FEW && ST_DEGENERATE == MCBA_RIG_DEGENERATE &&
              ST_NOT_CONVERGED == MCBA_RIG_NOT_CONVERGED && ST_BEHIND == MCBA_RIG_BEHIND, "mcba.h states the status bytes");

constexpr int MAX_VIEW_CORNERS = 1024;   // the largest board k_view_pose serves (pnp::view_pose_npl; mcba_localize.hip asserts it)

struct Plan {
  int C = 0, F = 0, B = 0, P = 0, K = 6, max_iter = DEFAULT_ITERATIONS;
  bool rolling = false;
  std::vector<double> recs;          // [C][REC_STRIDE]
  std::vector<double> W;             // [B P][3]
  std::vector<int32_t> first;        // [F + 1] record range of every frame
  std::vector<double> uv;            // [N][2]
  std::vector<int32_t> ocam, owpt;   // [N]
  std::vector<int64_t> slot;         // [N] index of the record in [C,F,B,P]
  // the start from views (calls without init)
  undistort::CameraPlan cams;        // camera table of k_view_pose
  std::vector<double> planes;        // [B][PLANE_STRIDE]
  std::vector<int32_t> view_first;   // [F + 1] range of every frame's active views, (c, b) order inside a frame
  std::vector<int32_t> view_desc;    // [views][2] camera, board
  std::vector<int64_t> view_row;     // [views] index of the view in [C,F,B]
  std::vector<double> cam_inv, board_inv;   // [C][12], [B][12]
  size_t n_records() const { return ocam.size(); }
  size_t n_views() const { return view_row.size(); }
};

inline bool usable(const mcba_rig_pose_problem* p, size_t slot, int b, int j) {
  if (!p->valid[slot]) return false;
  if (p->board_valid && !p->board_valid[(size_t)b * p->P + j]) return false;
  const double u = p->points[2 * slot], v = p->points[2 * slot + 1];
  return u - u == 0.0 && v - v == 0.0;
}

// checks the call and fills the plan; *empty: nothing to do (F == 0 or no cell in the table: the outputs are not looked at)
inline bool plan_problem(const mcba_rig_pose_problem* p, const double* poses, const uint8_t* status, Plan& out, bool* empty,
                         std::string& err) {
  const char* who = "mcba_rig_poses";
  const std::string w(who);
  *empty = true;
  if (!p) { err = w + ": null argument"; return false; }
  if (!undistort::plan_cameras(&p->cams, who, out.cams, err)) return false;
  const int C = p->cams.C;
  if (C > MAX_CAMERAS) {
    char msg[160];
    snprintf(msg, sizeof msg, "%s: %d cameras, at most %d are served (the camera records are staged in LDS)", who, C, MAX_CAMERAS);
    err = msg;
    return false;
  }
  if (p->F < 0 || p->B < 0 || p->P < 0) { err = w + ": negative size"; return false; }
  if (!(p->sigma_px == p->sigma_px) || p->sigma_px - p->sigma_px != 0.0) { err = w + ": sigma_px must be finite"; return false; }
  const bool rolling = p->rolling != 0;
  if (rolling && !p->image_heights) { err = w + ": rolling needs image_heights (the scan time is v / height)"; return false; }
  if (rolling)
    for (int c = 0; c < C; ++c)
      if (!(p->image_heights[c] > 0.0)) { err = w + ": image heights must be positive"; return false; }
  if (p->init_end && !p->init) { err = w + ": init_end needs init"; return false; }
  out.C = C; out.F = p->F; out.B = p->B; out.P = p->P;
  out.rolling = rolling;
  out.K = n_unknowns(rolling);
  out.max_iter = clamp_iterations(p->max_iterations);
  const long long cells = (long long)C * p->F * p->B * p->P;
  if (p->F == 0 || cells == 0) return true;
  if (cells >= (1ll << 31)) { err = w + ": table too large"; return false; }
  if (!p->camera_poses || !p->board_poses || !p->board_points || !p->points || !p->valid || !poses || !status) {
    err = w + ": null argument";
    return false;
  }
  *empty = false;
  const int F = p->F, B = p->B, P = p->P;
  out.recs.assign((size_t)C * REC_STRIDE, 0.0);
  out.cam_inv.assign((size_t)C * 12, 0.0);
  for (int c = 0; c < C; ++c) {
    double* e = out.recs.data() + (size_t)c * REC_STRIDE;
    memcpy(e, out.cams.cam.data() + (size_t)c * CAM_STRIDE, CAM_STRIDE * sizeof(double));
    e[CAM_HEIGHT] = rolling ? p->image_heights[c] : 0.0;
    e[CAM_ISFISH] = out.cams.cam_fish[c] ? 1.0 : 0.0;
    e[REC_ND] = (double)out.cams.cam_nd[c];
    memcpy(e + REC_POSE, p->camera_poses + (size_t)c * 16, 12 * sizeof(double));
    rigid_inverse(e + REC_POSE, out.cam_inv.data() + (size_t)c * 12);
  }
  out.W.assign((size_t)B * P * 3, 0.0);
  out.board_inv.assign((size_t)B * 12, 0.0);
  for (int b = 0; b < B; ++b) {
    const double* T = p->board_poses + (size_t)b * 16;
    rigid_inverse(T, out.board_inv.data() + (size_t)b * 12);
    for (int j = 0; j < P; ++j) triangulate::transform(T, p->board_points + ((size_t)b * P + j) * 3, out.W.data() + ((size_t)b * P + j) * 3);
  }
  // frame-major records: camera, then board, then point inside a frame
  out.first.assign((size_t)F + 1, 0);
  out.view_first.assign((size_t)F + 1, 0);
  const bool views = p->init == nullptr;
  for (int f = 0; f < F; ++f) {
    for (int c = 0; c < C; ++c)
      for (int b = 0; b < B; ++b) {
        const size_t view = ((size_t)c * F + f) * B + b;
        int n = 0;
        for (int j = 0; j < P; ++j) {
          const size_t slot = view * P + j;
          if (!usable(p, slot, b, j)) continue;
          out.uv.push_back(p->points[2 * slot]);
          out.uv.push_back(p->points[2 * slot + 1]);
          out.ocam.push_back(c);
          out.owpt.push_back(b * P + j);
          out.slot.push_back((int64_t)slot);
          ++n;
        }
        if (views && n >= pnp::MIN_CORNERS) {
          out.view_desc.push_back(c);
          out.view_desc.push_back(b);
          out.view_row.push_back((int64_t)view);
        }
      }
    out.first[(size_t)f + 1] = (int32_t)out.ocam.size();
    out.view_first[(size_t)f + 1] = (int32_t)out.view_row.size();
  }
  if (views && out.n_views() > 0) {
    if (P > MAX_VIEW_CORNERS) { err = w + ": boards of more than 1024 corners need init (the start comes from mcba_view_poses)"; return false; }
    // a board's plane is fitted to its VALID points only (board_valid may have holes): they are moved to the front of a copy of the row
    std::vector<int32_t> sizes((size_t)B, P);
    std::vector<double> packed;
    const double* fit = p->board_points;
    if (p->board_valid) {
      packed.assign((size_t)B * P * 3, 0.0);
      for (int b = 0; b < B; ++b) {
        int n = 0;
        for (int j = 0; j < P; ++j)
          if (p->board_valid[(size_t)b * P + j]) {
            memcpy(packed.data() + ((size_t)b * P + n) * 3, p->board_points + ((size_t)b * P + j) * 3, 3 * sizeof(double));
            ++n;
          }
        sizes[b] = n;
      }
      fit = packed.data();
    }
    if (!pnp::fit_board_planes(fit, sizes.data(), B, P, true, who, "init", out.planes, err)) return false;
  }
  return true;
}

// the pixel rows and usable masks of the active views, gathered for k_view_pose / pnp::view_pose: px [views][P][2], ok [views][P]
inline void gather_views(const mcba_rig_pose_problem* p, const Plan& plan, double* px, uint8_t* ok) {
  const size_t P = (size_t)plan.P;
  for (size_t k = 0; k < plan.n_views(); ++k) {
    const size_t v = (size_t)plan.view_row[k];
    const int b = plan.view_desc[2 * k + 1];
    memcpy(px + k * P * 2, p->points + v * P * 2, P * 2 * sizeof(double));
    for (size_t j = 0; j < P; ++j) {
      const bool good = usable(p, v * P + j, b, (int)j);
      ok[k * P + j] = good ? 1 : 0;
      if (!good) px[(k * P + j) * 2] = px[(k * P + j) * 2 + 1] = 0.0;
    }
  }
}

// per-slot errors from per-record errors: err [C,F,B,P], 0 where nothing entered
inline void scatter_errors(const Plan& plan, const double* err_rec, double* err) {
  const size_t cells = (size_t)plan.C * plan.F * plan.B * plan.P;
  for (size_t i = 0; i < cells; ++i) err[i] = 0.0;
  for (size_t i = 0; i < plan.n_records(); ++i) err[(size_t)plan.slot[i]] = err_rec[i];
}

// outputs of a call with nothing to launch (F > 0 but an empty table)
inline void fill_empty(const mcba_rig_pose_problem* p, int K, double* poses, double* poses_end, double* cov, double* sse, int32_t* n_obs,
                       int32_t* iters, uint8_t* status) {
  for (int f = 0; f < p->F; ++f) {
    if (poses) pnp::identity_pose(poses + 16 * (size_t)f);
    if (poses_end) pnp::identity_pose(poses_end + 16 * (size_t)f);
    if (cov)
      for (int i = 0; i < n_cov(K); ++i) cov[(size_t)f * n_cov(K) + i] = undistort::quiet_nan();
    if (sse) sse[f] = 0.0;
    if (n_obs) n_obs[f] = 0;
    if (iters) iters[f] = 0;
    if (status) status[f] = (uint8_t)ST_TOO_FEW;
  }
}

}  // namespace localize
}  // namespace mcba
