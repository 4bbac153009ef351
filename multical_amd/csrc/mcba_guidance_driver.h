// mcba_guidance_driver.h -- host side of mcba_view_information that does not touch the device: argument checks, the camera and view
// records of mcba_guidance.h, the list of views that are launched, the score list, and the greedy loop over a back-end (the device
// in mcba_guidance.hip, plain loops in tests/guidance), so that both refuse the same calls and pick by the same rule.
#pragma once
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/mcba.h"
#include "mcba_guidance.h"
#include "mcba_undistort_driver.h"

namespace mcba {
namespace guidance {

static_assert(MAX_R == MCBA_GUIDE_MAX_R, "mcba.h states the widest factor");
static_assert(ST_OK == MCBA_GUIDE_OK && ST_TOO_FEW == MCBA_GUIDE_TOO_FEW && ST_DEGENERATE == MCBA_GUIDE_DEGENERATE &&
              ST_UNCONSTRAINED == MCBA_GUIDE_UNCONSTRAINED && CRIT_FOCUS == MCBA_GUIDE_BY_FOCUS && CRIT_GAIN == MCBA_GUIDE_BY_GAIN,
              "mcba.h states the status bytes and the criteria");

struct Plan {
  int C = 0, V = 0, rs = 1, n_picks = 0, criterion = 0, board_stride = 0;
  double inv_s2 = 1.0;
  std::vector<double> crecs;          // [C][CREC_STRIDE]
  std::vector<double> vrecs;          // [V + C][V_STRIDE]: the candidates, then the focus of every camera (V_N = 0: none)
  std::vector<double> uv;             // the pixel lists
  std::vector<double> board_points;   // [B][board_stride][3]
  std::vector<double> board_mean;     // [B][3] the centroid of every board
  std::vector<int32_t> cam_r;         // [C]
  std::vector<uint8_t> cam_served;    // [C] r > 0 and no unconstrained intrinsic
  std::vector<int32_t> view_camera;   // [V + C]
  std::vector<uint8_t> status0;       // [V + C] what a view that is not launched keeps
  std::vector<int32_t> launch;        // the views k_view_schur serves
  std::vector<int32_t> entries;       // the score list: -(c + 1) of every served camera, then its candidates in view order
  int n_null = 0;                     // how many null entries lead the list
};

inline bool finite_arg(double v) { return v - v == 0.0; }

inline bool plan_view(const mcba_guidance_view& view, bool focus, int j, int n_boards, const int32_t* board_n, Plan& out, double* rec,
                      std::string& err) {
  const char* who = "mcba_view_information";
  const char* what = focus ? "focus" : "view";
  char msg[240];
  if (view.n_nuisance != 0 && view.n_nuisance != 3 && view.n_nuisance != 6) {
    snprintf(msg, sizeof msg, "%s: %s %d: n_nuisance = %d (0, 3 or 6)", who, what, j, view.n_nuisance); err = msg; return false;
  }
  if (view.min_points < 0) { snprintf(msg, sizeof msg, "%s: %s %d: negative min_points", who, what, j); err = msg; return false; }
  rec[V_CAMERA] = (double)view.camera;
  rec[V_NN] = (double)view.n_nuisance;
  rec[V_MIN] = (double)view.min_points;
  if (!focus) {
    if (view.board < 0 || view.board >= n_boards) {
      snprintf(msg, sizeof msg, "%s: view %d: board %d of %d", who, j, view.board, n_boards); err = msg; return false;
    }
    for (int i = 0; i < 12; ++i) {
      if (!finite_arg(view.pose[i])) { snprintf(msg, sizeof msg, "%s: view %d: the pose is not finite", who, j); err = msg; return false; }
      rec[V_POSE + i] = view.pose[i];
    }
    rec[V_KIND] = (double)KIND_BOARD;
    rec[V_BOARD] = (double)view.board;
    rec[V_RHO] = 1.0;
    rec[V_N] = (double)board_n[view.board];
    const double* mean = out.board_mean.data() + 3 * (size_t)view.board;
    for (int k = 0; k < 3; ++k)
      rec[V_CENTRE + k] = view.pose[4 * k] * mean[0] + view.pose[4 * k + 1] * mean[1] + view.pose[4 * k + 2] * mean[2] + view.pose[4 * k + 3];
    return true;
  }
  if (view.board >= 0) { snprintf(msg, sizeof msg, "%s: focus %d: a focus has board < 0", who, j); err = msg; return false; }
  if (!finite_arg(view.inv_distance) || view.inv_distance < 0.0 || (view.n_nuisance == 6 && !(view.inv_distance > 0.0))) {
    snprintf(msg, sizeof msg, "%s: focus %d: inv_distance must be finite and >= 0, and > 0 with n_nuisance = 6", who, j);
    err = msg;
    return false;
  }
  rec[V_RHO] = view.inv_distance;
  rec[V_CENTRE + 2] = 1.0;
  if (view.grid_w > 0) {
    if (view.grid_h <= 0 || (int64_t)view.grid_w * view.grid_h > (1 << 24) || !finite_arg(view.u0) || !finite_arg(view.v0) ||
        !finite_arg(view.du) || !finite_arg(view.dv)) {
      snprintf(msg, sizeof msg, "%s: focus %d: a grid needs grid_h > 0, at most 2^24 pixels and finite u0, v0, du, dv", who, j);
      err = msg;
      return false;
    }
    rec[V_KIND] = (double)KIND_GRID;
    rec[V_GW] = (double)view.grid_w;
    rec[V_N] = (double)((int64_t)view.grid_w * view.grid_h);
    rec[V_U0] = view.u0; rec[V_V0] = view.v0; rec[V_DU] = view.du; rec[V_DV] = view.dv;
  } else {
    if (view.grid_w < 0 || view.n < 0 || view.n > (1 << 24)) {
      snprintf(msg, sizeof msg, "%s: focus %d: 0 .. 2^24 pixels", who, j); err = msg; return false;
    }
    if (view.n > 0 && !view.uv) { snprintf(msg, sizeof msg, "%s: focus %d: uv is null", who, j); err = msg; return false; }
    rec[V_KIND] = (double)KIND_LIST;
    rec[V_N] = (double)view.n;
    rec[V_FIRST] = (double)(out.uv.size() / 2);
    out.uv.insert(out.uv.end(), view.uv, view.uv + 2 * view.n);
  }
  return true;
}

inline bool plan_views(const mcba_camera_set* cams, const mcba_guidance_camera* info, int32_t n_boards, int32_t board_stride,
                       const int32_t* board_n, const double* board_points, double margin, double sigma2, int32_t n_views,
                       const mcba_guidance_view* views, const mcba_guidance_view* foci, int32_t n_picks, int32_t criterion,
                       const mcba_guidance_result* res, Plan& out, std::string& err) {
  const char* who = "mcba_view_information";
  const std::string w(who);
  undistort::CameraPlan plan;
  if (!undistort::plan_cameras(cams, who, plan, err)) return false;
  const int C = cams->C;
  char msg[240];
  if (!info || !res) { err = w + ": null argument"; return false; }
  if (n_views < 0 || n_boards < 0 || board_stride < 0 || n_picks < 0) { err = w + ": negative size"; return false; }
  if (n_views > 0 && !views) { err = w + ": null argument"; return false; }
  if (n_boards > 0 && (!board_n || !board_points)) { err = w + ": null argument"; return false; }
  if (!(sigma2 > 0.0) || !finite_arg(sigma2)) { err = w + ": sigma2 must be positive and finite"; return false; }
  if (!finite_arg(margin)) { err = w + ": margin must be finite"; return false; }
  if (criterion != CRIT_FOCUS && criterion != CRIT_GAIN) { err = w + ": criterion is MCBA_GUIDE_BY_FOCUS or MCBA_GUIDE_BY_GAIN"; return false; }
  if (n_views > 0 && (!res->n_visible || !res->status || !res->gain || !res->focus_rms)) { err = w + ": null output"; return false; }
  if (n_picks > 0 && (!res->picks || !res->pick_gain || !res->pick_focus_rms)) { err = w + ": null output"; return false; }
  for (int b = 0; b < n_boards; ++b)
    if (board_n[b] < 0 || board_n[b] > board_stride) {
      snprintf(msg, sizeof msg, "%s: board %d: %d points in rows of %d", who, b, board_n[b], board_stride); err = msg; return false;
    }
  out.C = C; out.V = n_views; out.n_picks = n_picks; out.criterion = criterion; out.board_stride = board_stride;
  out.inv_s2 = 1.0 / sigma2;
  out.board_points.assign(board_points, board_points + (size_t)n_boards * board_stride * 3);
  for (double v : out.board_points)
    if (!finite_arg(v)) { err = w + ": board_points are not finite"; return false; }
  out.board_mean.assign((size_t)n_boards * 3, 0.0);
  for (int b = 0; b < n_boards; ++b)
    for (int i = 0; i < board_n[b]; ++i)
      for (int k = 0; k < 3; ++k) out.board_mean[3 * (size_t)b + k] += out.board_points[((size_t)b * board_stride + i) * 3 + k] / board_n[b];
  out.crecs.assign((size_t)C * CREC_STRIDE, 0.0);
  out.cam_r.assign(C, 0);
  out.cam_served.assign(C, 0);
  out.rs = 1;
  for (int c = 0; c < C; ++c) {
    const mcba_guidance_camera& ci = info[c];
    const int ki = 4 + plan.cam_nd[c];
    if (ci.r < 0 || ci.r > MAX_R) { snprintf(msg, sizeof msg, "%s: camera %d: r = %d, W has 0 .. %d columns", who, c, ci.r, MAX_R); err = msg; return false; }
    if (ci.r > 0 && !ci.W) { snprintf(msg, sizeof msg, "%s: camera %d: W is null", who, c); err = msg; return false; }
    if (!(ci.image_w > 0.0) || !(ci.image_h > 0.0) || !finite_arg(ci.image_w) || !finite_arg(ci.image_h)) {
      snprintf(msg, sizeof msg, "%s: camera %d: the image size must be positive", who, c); err = msg; return false;
    }
    double* rec = out.crecs.data() + (size_t)c * CREC_STRIDE;
    const double* e = plan.cam.data() + (size_t)c * CAM_STRIDE;
    for (int i = 0; i < CAM_STRIDE; ++i) rec[i] = e[i];
    rec[CAM_ISFISH] = plan.cam_fish[c] ? 1.0 : 0.0;
    rec[uncertainty::REC_ND] = (double)plan.cam_nd[c];
    rec[CREC_W_IMG] = ci.image_w; rec[CREC_H_IMG] = ci.image_h; rec[CREC_RANK] = (double)ci.r; rec[CREC_MARGIN] = margin;
    for (int k = 0; k < ki; ++k)
      for (int j = 0; j < ci.r; ++j) {
        const double v = ci.W[(size_t)k * ci.r + j];
        if (!finite_arg(v)) { snprintf(msg, sizeof msg, "%s: camera %d: W is not finite", who, c); err = msg; return false; }
        rec[CREC_W + k * MAX_R + j] = v;
      }
    out.cam_r[c] = ci.r;
    out.cam_served[c] = ci.r > 0 && !ci.unconstrained;
    if (ci.r > out.rs) out.rs = ci.r;
  }
  const size_t N = (size_t)n_views + C;
  out.vrecs.assign(N * V_STRIDE, 0.0);
  out.view_camera.assign(N, 0);
  out.status0.assign(N, (uint8_t)ST_OK);
  out.uv.clear();
  out.launch.clear();
  for (int j = 0; j < n_views; ++j) {
    const int c = views[j].camera;
    if (c < 0 || c >= C) { snprintf(msg, sizeof msg, "%s: view %d: camera %d of %d", who, j, c, C); err = msg; return false; }
    if (!plan_view(views[j], views[j].board < 0, j, n_boards, board_n, out, out.vrecs.data() + (size_t)j * V_STRIDE, err)) return false;
    out.view_camera[j] = c;
    if (info[c].unconstrained) out.status0[j] = (uint8_t)ST_UNCONSTRAINED;
    else if (out.cam_served[c]) out.launch.push_back(j);
  }
  for (int c = 0; c < C; ++c) {
    const size_t f = (size_t)n_views + c;
    out.view_camera[f] = c;
    out.vrecs[f * V_STRIDE + V_CAMERA] = (double)c;
    out.status0[f] = (uint8_t)(info[c].unconstrained ? ST_UNCONSTRAINED : ST_TOO_FEW);
    if (!foci || foci[c].camera < 0) continue;
    if (foci[c].camera != c) { snprintf(msg, sizeof msg, "%s: focus %d names camera %d", who, c, foci[c].camera); err = msg; return false; }
    if (!plan_view(foci[c], true, c, n_boards, board_n, out, out.vrecs.data() + f * V_STRIDE, err)) return false;
    if (out.cam_served[c] && out.vrecs[f * V_STRIDE + V_N] > 0.0 && n_views > 0) out.launch.push_back((int32_t)f);
    else if (out.cam_r[c] == 0 && !info[c].unconstrained) out.status0[f] = (uint8_t)ST_OK;
  }
  out.entries.clear();
  for (int c = 0; c < C; ++c)
    if (out.cam_served[c]) out.entries.push_back(-(c + 1));
  out.n_null = (int)out.entries.size();
  for (int j = 0; j < n_views; ++j)
    if (out.cam_served[views[j].camera]) out.entries.push_back(j);
  return true;
}

// what the outputs hold before anything is computed (and all they hold after a call with nothing to launch)
inline void fill_defaults(const Plan& p, const mcba_guidance_result* res) {
  const double nan = undistort::quiet_nan();
  const size_t rr = (size_t)p.rs * p.rs;
  for (int j = 0; j < p.V; ++j) {
    const bool ok = p.status0[j] == ST_OK && !p.cam_served[p.view_camera[j]];     // a camera with r = 0
    res->n_visible[j] = 0;
    res->status[j] = p.status0[j];
    res->gain[j] = ok ? 0.0 : nan;
    res->focus_rms[j] = ok ? 0.0 : nan;
  }
  if (res->S) for (size_t i = 0; i < (size_t)p.V * rr; ++i) res->S[i] = 0.0;
  if (res->Q) for (size_t i = 0; i < (size_t)p.C * rr; ++i) res->Q[i] = 0.0;
  if (res->posterior) for (size_t i = 0; i < (size_t)p.C * rr; ++i) res->posterior[i] = 0.0;
  for (int c = 0; c < p.C; ++c) {
    if (res->focus_status) res->focus_status[c] = p.status0[(size_t)p.V + c];
    if (res->focus_n_visible) res->focus_n_visible[c] = 0;
    if (res->focus_before) res->focus_before[c] = p.cam_r[c] == 0 && p.status0[(size_t)p.V + c] == ST_OK ? 0.0 : nan;
    if (res->posterior && p.cam_served[c])
      for (int i = 0; i < p.cam_r[c]; ++i) res->posterior[c * rr + (size_t)i * p.rs + i] = 1.0;
    for (int k = 0; k < p.n_picks; ++k) {
      res->picks[(size_t)c * p.n_picks + k] = -1;
      res->pick_gain[(size_t)c * p.n_picks + k] = nan;
      res->pick_focus_rms[(size_t)c * p.n_picks + k] = nan;
    }
  }
  for (size_t i = 0; i < (size_t)p.n_picks * p.V; ++i) {
    if (res->round_gain) res->round_gain[i] = nan;
    if (res->round_focus_rms) res->round_focus_rms[i] = nan;
  }
}

// The greedy loop.  Backend: score(n_entries, with_posterior) scores the first n_entries of the list into gain() / focus() (host
// arrays of the list's length); add(winners [C]) adds the winners' A to the bases.
template <class Backend>
void greedy_rounds(const Plan& p, Backend& be, const mcba_guidance_result* res) {
  const size_t ne = p.entries.size();
  std::vector<uint8_t> taken((size_t)p.V, 0);
  std::vector<int32_t> winners((size_t)p.C, -1), null_at((size_t)p.C, -1);
  for (int e = 0; e < p.n_null; ++e) null_at[-p.entries[e] - 1] = e;
  for (int round = 0; round <= p.n_picks; ++round) {
    const bool last = round == p.n_picks;
    if (last && round > 0 && !res->posterior && !res->pick_focus_rms) break;
    be.score(last && round > 0 ? (size_t)p.n_null : ne, last && res->posterior != nullptr);
    const double* gain = be.gain();
    const double* focus = be.focus();
    for (int c = 0; c < p.C; ++c) {
      if (null_at[c] < 0) continue;
      if (round == 0 && res->focus_before) res->focus_before[c] = focus[null_at[c]];
      if (round > 0) res->pick_focus_rms[(size_t)c * p.n_picks + round - 1] = winners[c] >= 0 ? focus[null_at[c]] : undistort::quiet_nan();
    }
    if (last && round > 0) break;
    for (size_t e = (size_t)p.n_null; e < ne; ++e) {
      const int v = p.entries[e];
      if (round == 0) { res->gain[v] = gain[e]; res->focus_rms[v] = focus[e]; }
      if (!last && res->round_gain) res->round_gain[(size_t)round * p.V + v] = gain[e];
      if (!last && res->round_focus_rms) res->round_focus_rms[(size_t)round * p.V + v] = focus[e];
    }
    if (last) break;
    std::vector<double> best((size_t)p.C, 0.0);
    for (int c = 0; c < p.C; ++c) winners[c] = -1;
    for (size_t e = (size_t)p.n_null; e < ne; ++e) {
      const int v = p.entries[e], c = p.view_camera[v];
      const double s = p.criterion == CRIT_GAIN ? gain[e] : -focus[e];
      if (taken[v] || !(s == s) || !(gain[e] == gain[e])) continue;
      if (winners[c] < 0 || s > best[c]) { winners[c] = v; best[c] = s; }
    }
    for (size_t e = (size_t)p.n_null; e < ne; ++e) {
      const int v = p.entries[e], c = p.view_camera[v];
      if (winners[c] != v) continue;
      taken[v] = 1;
      res->picks[(size_t)c * p.n_picks + round] = v;
      res->pick_gain[(size_t)c * p.n_picks + round] = gain[e];
    }
    be.add(winners.data());
  }
}

}  // namespace guidance
}  // namespace mcba
