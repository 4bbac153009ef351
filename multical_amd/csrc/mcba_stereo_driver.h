// mcba_stereo_driver.h -- host side of mcba_stereo_calibrate that does not touch the device: argument checks, the camera records,
// the views of every pair with their common-corner counts, the compaction to the pairs that are launched, and the scatter of the
// per-view results.  Shared by the driver (mcba_stereo.hip) and the host build of the mathematics (tests/stereo_host), so that
// both refuse the same calls with the same messages and walk the same views.
#pragma once
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/mcba.h"
#include "mcba_stereo.h"
#include "mcba_undistort_driver.h"

namespace mcba {
namespace stereo {

static_assert(ST_OK == MCBA_STEREO_OK && ST_TOO_FEW == MCBA_STEREO_TOO_FEW && ST_DEGENERATE == MCBA_STEREO_DEGENERATE &&
              ST_NOT_CONVERGED == MCBA_STEREO_NOT_CONVERGED, "mcba.h states the status bytes");

// the common corners of a slot lie on one line: the farthest point from their centroid gives the direction, and no point stands off
// that line by more than COLLINEAR_TOL of that distance (the square of it is PIVOT_FLOOR: what the factor of the view's scaled block
// would meet).  Such a view leaves the rotation about its line free and is dropped like one with too few corners
constexpr double COLLINEAR_TOL = 1e-6;
inline bool collinear_view(const Tables& t, size_t rowl, size_t rowr, int b) {
  double c[3] = {0.0, 0.0, 0.0}, far[3] = {0.0, 0.0, 0.0}, dmax = 0.0;
  int n = 0;
  for (int j = 0; j < t.P; ++j)
    if (common_corner(t, rowl, rowr, b, j)) {
      for (int i = 0; i < 3; ++i) c[i] += t.board[((size_t)b * t.P + j) * 3 + i];
      ++n;
    }
  if (n == 0) return true;
  for (int i = 0; i < 3; ++i) c[i] /= (double)n;
  for (int j = 0; j < t.P; ++j)
    if (common_corner(t, rowl, rowr, b, j)) {
      const double* X = t.board + ((size_t)b * t.P + j) * 3;
      const double d[3] = {X[0] - c[0], X[1] - c[1], X[2] - c[2]}, q = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
      if (q > dmax) { dmax = q; far[0] = d[0]; far[1] = d[1]; far[2] = d[2]; }
    }
  if (!(dmax > 0.0)) return true;
  for (int j = 0; j < t.P; ++j)
    if (common_corner(t, rowl, rowr, b, j)) {
      const double* X = t.board + ((size_t)b * t.P + j) * 3;
      const double d[3] = {X[0] - c[0], X[1] - c[1], X[2] - c[2]};
      const double along = (d[0] * far[0] + d[1] * far[1] + d[2] * far[2]) / dmax;
      const double o[3] = {d[0] - along * far[0], d[1] - along * far[1], d[2] - along * far[2]};
      if (o[0] * o[0] + o[1] * o[1] + o[2] * o[2] > COLLINEAR_TOL * COLLINEAR_TOL * dmax) return false;
    }
  return true;
}

struct Plan {
  int C = 0, F = 0, B = 0, P = 0, n_pairs = 0, min_common = DEFAULT_MIN_COMMON, max_iter = DEFAULT_ITERATIONS;
  undistort::CameraPlan cams;
  std::vector<double> recs;            // [C][CAM_STRIDE]
  std::vector<int32_t> n_views, n_points;   // [n_pairs]
  std::vector<int32_t> n_collinear;    // [n_pairs] slots with enough common corners, all on one line: dropped
  // the pairs that are launched (at least one view), in the order of the call
  std::vector<int32_t> launched;       // [n_launched] index of the pair in the call
  std::vector<int32_t> desc;           // [n_launched][2] left, right
  std::vector<int32_t> first;          // [n_launched + 1] view range of every launched pair
  std::vector<int32_t> slot, n_common; // [views] f B + b; common corners
  size_t n_launched() const { return launched.size(); }
  size_t total_views() const { return slot.size(); }
};

inline Tables host_tables(const mcba_stereo_problem* p, const Plan& plan) {
  return Tables{plan.F, plan.B, plan.P, plan.recs.data(), p->board_points, p->board_valid, p->points, p->valid, p->view_poses};
}

// checks the call and fills the plan
inline bool plan_problem(const mcba_stereo_problem* p, const double* T, const uint8_t* status, Plan& out, std::string& err) {
  const char* who = "mcba_stereo_calibrate";
  const std::string w(who);
  if (!p) { err = w + ": null argument"; return false; }
  if (p->n_pairs < 0 || p->F < 0 || p->B < 0 || p->P < 0) { err = w + ": negative size"; return false; }
  out.n_pairs = p->n_pairs;
  out.F = p->F; out.B = p->B; out.P = p->P;
  out.min_common = p->min_common <= 0 ? DEFAULT_MIN_COMMON : p->min_common;
  out.max_iter = clamp_iterations(p->max_iterations);
  if (p->n_pairs == 0) return true;
  if (!undistort::plan_cameras(&p->cams, who, out.cams, err)) return false;
  const int C = out.C = p->cams.C;
  if (out.min_common < MIN_MIN_COMMON) { err = w + ": min_common below 3 (a view of fewer common corners does not fix its pose)"; return false; }
  if (!(p->sigma_px == p->sigma_px) || p->sigma_px - p->sigma_px != 0.0) { err = w + ": sigma_px must be finite"; return false; }
  if (!p->pairs || !T || !status) { err = w + ": null argument"; return false; }
  for (int k = 0; k < p->n_pairs; ++k) {
    const int l = p->pairs[2 * k], r = p->pairs[2 * k + 1];
    if (l < 0 || l >= C || r < 0 || r >= C || l == r) {
      char msg[160];
      snprintf(msg, sizeof msg, "%s: pair %d is (%d, %d): two different cameras out of %d are needed", who, k, l, r, C);
      err = msg;
      return false;
    }
  }
  const long long cells = (long long)C * p->F * p->B * p->P;
  if (cells >= (1ll << 31)) { err = w + ": table too large"; return false; }
  out.n_views.assign((size_t)p->n_pairs, 0);
  out.n_points.assign((size_t)p->n_pairs, 0);
  out.n_collinear.assign((size_t)p->n_pairs, 0);
  out.first.assign(1, 0);
  if (cells == 0) return true;
  if (!p->board_points || !p->points || !p->valid || !p->view_poses || !p->view_valid) { err = w + ": null argument"; return false; }
  out.recs.assign((size_t)C * CAM_STRIDE, 0.0);
  for (int c = 0; c < C; ++c) {
    double* e = out.recs.data() + (size_t)c * CAM_STRIDE;
    memcpy(e, out.cams.cam.data() + (size_t)c * CAM_STRIDE, CAM_STRIDE * sizeof(double));
    e[CAM_ISFISH] = out.cams.cam_fish[c] ? 1.0 : 0.0;
    e[triangulate::REC_ND] = (double)out.cams.cam_nd[c];
  }
  const Tables t = host_tables(p, out);
  const int FB = p->F * p->B;
  for (int k = 0; k < p->n_pairs; ++k) {
    const int l = p->pairs[2 * k], r = p->pairs[2 * k + 1];
    for (int s = 0; s < FB; ++s) {
      if (!p->view_valid[(size_t)l * FB + s] || !p->view_valid[(size_t)r * FB + s]) continue;
      const size_t rowl = slot_row(t, l, s), rowr = slot_row(t, r, s);
      int n = 0;
      for (int j = 0; j < p->P; ++j) n += common_corner(t, rowl, rowr, s % p->B, j) ? 1 : 0;
      if (n < out.min_common) continue;
      if (collinear_view(t, rowl, rowr, s % p->B)) { out.n_collinear[k] += 1; continue; }
      out.slot.push_back(s);
      out.n_common.push_back(n);
      out.n_views[k] += 1;
      out.n_points[k] += n;
    }
    if (out.n_views[k] > 0) {
      out.launched.push_back(k);
      out.desc.push_back(l);
      out.desc.push_back(r);
      out.first.push_back((int32_t)out.slot.size());
    }
  }
  return true;
}

// what every pair returns before anything is solved: no result; TOO_FEW, or DEGENERATE where all it has are collinear views
inline void fill_unsolved(const mcba_stereo_problem* p, const Plan& plan, double* T, double* cov, double* sse, int32_t* n_views,
                          int32_t* n_points, int32_t* iterations, double* view_poses_out, double* view_sse, uint8_t* status) {
  const size_t FB = (size_t)plan.F * plan.B;
  for (int k = 0; k < p->n_pairs; ++k) {
    pnp::identity_pose(T + 16 * (size_t)k);
    if (cov)
      for (int i = 0; i < 36; ++i) cov[36 * (size_t)k + i] = undistort::quiet_nan();
    if (sse) sse[k] = 0.0;
    if (n_views) n_views[k] = plan.n_views.empty() ? 0 : plan.n_views[k];
    if (n_points) n_points[k] = plan.n_points.empty() ? 0 : plan.n_points[k];
    if (iterations) iterations[k] = 0;
    if (view_poses_out)
      for (size_t s = 0; s < FB; ++s) pnp::identity_pose(view_poses_out + ((size_t)k * FB + s) * 16);
    if (view_sse)
      for (size_t s = 0; s < 2 * FB; ++s) view_sse[(size_t)k * 2 * FB + s] = 0.0;
    status[k] = (uint8_t)(!plan.n_collinear.empty() && plan.n_collinear[k] > 0 ? ST_DEGENERATE : ST_TOO_FEW);
  }
}

// the per-view results of the launched pairs, from the view blocks ws [views][VB_STRIDE], to their slots; have [n_launched]
inline void scatter_views(const Plan& plan, const double* ws, const uint8_t* pair_status, double* view_poses_out, double* view_sse) {
  const size_t FB = (size_t)plan.F * plan.B;
  for (size_t i = 0; i < plan.n_launched(); ++i) {
    if (pair_status[i] != ST_OK && pair_status[i] != ST_NOT_CONVERGED) continue;
    const size_t k = (size_t)plan.launched[i];
    for (int v = plan.first[i]; v < plan.first[i + 1]; ++v) {
      const double* vb = ws + (size_t)v * VB_STRIDE;
      const size_t s = k * FB + (size_t)plan.slot[v];
      if (view_poses_out) intr::params_to_pose(vb + VB_P, view_poses_out + 16 * s);
      if (view_sse) { view_sse[2 * s] = vb[VB_SSE]; view_sse[2 * s + 1] = vb[VB_SSE + 1]; }
    }
  }
}

}  // namespace stereo
}  // namespace mcba
