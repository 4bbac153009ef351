// mcba_rigview_driver.h -- host side of mcba_rig_view_information that does not touch the device: argument checks and refusals, the
// camera, slot and focus-pair records of mcba_rigview.h, the fold of the focus Gram matrices into Q, and the greedy loop over a
// back-end (the device in mcba_rigview.hip, plain loops in tests/rigview), so that both refuse the same calls and pick by one rule.
#pragma once
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/mcba.h"
#include "mcba_rigview.h"
#include "mcba_undistort_driver.h"

namespace mcba {
namespace rigview {

static_assert(MAX_R == MCBA_RIG_MAX_R && KC == MCBA_RIG_COLUMNS, "mcba.h states the widest factor and the rows of a W");

struct Plan {
  int C = 0, V = 0, r = 0, rs = 1, n_picks = 0, criterion = 0, board_stride = 0, min_cameras = 1;
  double inv_s2 = 1.0;
  std::vector<double> crecs;          // [C][RC_STRIDE]
  std::vector<double> srecs;          // [V C][S_STRIDE]
  std::vector<double> board_points;   // [B][board_stride][3]
  std::vector<double> W;              // [C][KC][rs]
  std::vector<uint8_t> loose;         // [C]
  std::vector<int32_t> launch;        // the slots k_rig_gram serves: all of them
  std::vector<int32_t> entries;       // the score list: -1 (the base alone), then every view
  // the focus
  int n_pairs = 0, gw = 0, gn = 0;
  double u0 = 0.0, v0 = 0.0, du = 0.0, dv = 0.0;
  bool focus_loose = false;
  std::vector<double> frecs;          // [n_pairs][F_STRIDE]
  std::vector<double> Wab;            // [n_pairs][KP][rs]: the rows of the factor in the column order of the pair's job
  bool nothing = false;               // r = 0 or V = 0: nothing is launched
};

inline bool finite_arg(double v) { return v - v == 0.0; }

inline bool plan_rig(const mcba_camera_set* cams, const double* camera_poses, int32_t r, const mcba_rig_camera* info, int32_t boards,
                     int32_t n_boards, int32_t board_stride, const int32_t* board_n, const double* board_points, int32_t n_views,
                     const mcba_rig_view* views, int32_t min_cameras, double margin, double sigma2, const mcba_rig_focus* focus,
                     int32_t n_picks, int32_t criterion, int32_t workspace_mb, const mcba_rig_result* res, Plan& out, std::string& err) {
  const char* who = "mcba_rig_view_information";
  const std::string w(who);
  undistort::CameraPlan plan;
  if (!undistort::plan_cameras(cams, who, plan, err)) return false;
  const int C = cams->C;
  char msg[320];
  if (!info || !res || !camera_poses) { err = w + ": null argument"; return false; }
  if (n_views < 0 || n_boards < 0 || board_stride < 0 || n_picks < 0 || r < 0) { err = w + ": negative size"; return false; }
  if (boards != 0) {
    err = w + ": boards=True: the board points are parameters of this calibration, and a candidate's board is then not a known object; "
              "rig views are scored with the boards held (optimize boards=False)";
    return false;
  }
  if (r > MAX_R) {
    snprintf(msg, sizeof msg, "%s: r = %d: the factor of this camera group has more than MCBA_RIG_MAX_R = %d columns; pass a smaller "
             "cameras= group", who, r, MAX_R);
    err = msg;
    return false;
  }
  const int rs = r > 0 ? r : 1;
  if (workspace_mb < 0) { err = w + ": negative workspace_mb"; return false; }
  if ((double)n_views * rs * rs * 8.0 > (double)workspace_mb * 1048576.0) {
    snprintf(msg, sizeof msg, "%s: %d candidates of %d x %d doubles exceed the workspace of %d MB; pass fewer candidates per call "
             "(or a larger workspace_mb)", who, n_views, rs, rs, workspace_mb);
    err = msg;
    return false;
  }
  if (n_views > 0 && !views) { err = w + ": null argument"; return false; }
  if (n_boards > 0 && (!board_n || !board_points)) { err = w + ": null argument"; return false; }
  if (!(sigma2 > 0.0) || !finite_arg(sigma2)) { err = w + ": sigma2 must be positive and finite"; return false; }
  if (!finite_arg(margin)) { err = w + ": margin must be finite"; return false; }
  if (min_cameras < 1) { err = w + ": min_cameras is at least 1"; return false; }
  if (criterion != CRIT_FOCUS && criterion != CRIT_GAIN) { err = w + ": criterion is MCBA_GUIDE_BY_FOCUS or MCBA_GUIDE_BY_GAIN"; return false; }
  if (n_views > 0 && (!res->n_cameras || !res->n_visible || !res->status || !res->gain || !res->focus_rms)) { err = w + ": null output"; return false; }
  if (n_picks > 0 && (!res->picks || !res->pick_gain || !res->pick_focus_rms)) { err = w + ": null output"; return false; }
  for (int b = 0; b < n_boards; ++b)
    if (board_n[b] < 0 || board_n[b] > board_stride) {
      snprintf(msg, sizeof msg, "%s: board %d: %d points in rows of %d", who, b, board_n[b], board_stride); err = msg; return false;
    }
  for (int i = 0; i < 12 * C; ++i)
    if (!finite_arg(camera_poses[i])) { err = w + ": camera_poses are not finite"; return false; }
  out.C = C; out.V = n_views; out.r = r; out.rs = rs; out.n_picks = n_picks; out.criterion = criterion; out.board_stride = board_stride;
  out.min_cameras = min_cameras;
  out.inv_s2 = 1.0 / sigma2;
  out.board_points.assign(board_points, board_points + (size_t)n_boards * board_stride * 3);
  for (double v : out.board_points)
    if (!finite_arg(v)) { err = w + ": board_points are not finite"; return false; }
  std::vector<double> board_mean((size_t)n_boards * 3, 0.0);
  for (int b = 0; b < n_boards; ++b)
    for (int i = 0; i < board_n[b]; ++i)
      for (int k = 0; k < 3; ++k) board_mean[3 * (size_t)b + k] += out.board_points[((size_t)b * board_stride + i) * 3 + k] / board_n[b];
  out.crecs.assign((size_t)C * RC_STRIDE, 0.0);
  out.W.assign((size_t)C * KC * rs, 0.0);
  out.loose.assign(C, 0);
  for (int c = 0; c < C; ++c) {
    const mcba_rig_camera& ci = info[c];
    if (r > 0 && !ci.W) { snprintf(msg, sizeof msg, "%s: camera %d: W is null", who, c); err = msg; return false; }
    if (!(ci.image_w > 0.0) || !(ci.image_h > 0.0) || !finite_arg(ci.image_w) || !finite_arg(ci.image_h)) {
      snprintf(msg, sizeof msg, "%s: camera %d: the image size must be positive", who, c); err = msg; return false;
    }
    double* rec = out.crecs.data() + (size_t)c * RC_STRIDE;
    double* e = plan.cam.data() + (size_t)c * CAM_STRIDE;
    e[CAM_ISFISH] = plan.cam_fish[c] ? 1.0 : 0.0;
    e[uncertainty::REC_ND] = (double)plan.cam_nd[c];
    for (int i = 0; i < CAM_STRIDE; ++i) rec[i] = e[i];
    rec[guidance::CREC_W_IMG] = ci.image_w; rec[guidance::CREC_H_IMG] = ci.image_h; rec[guidance::CREC_MARGIN] = margin;
    for (int k = 0; k < KC; ++k)
      for (int j = 0; j < r; ++j) {
        const double v = ci.W[(size_t)k * r + j];
        if (!finite_arg(v)) { snprintf(msg, sizeof msg, "%s: camera %d: W is not finite", who, c); err = msg; return false; }
        if (k >= 4 + plan.cam_nd[c] && k < KI && v != 0.0) {
          snprintf(msg, sizeof msg, "%s: camera %d: row %d of W belongs to a coefficient the camera does not have", who, c, k); err = msg; return false;
        }
        out.W[((size_t)c * KC + k) * rs + j] = v;
      }
    out.loose[c] = ci.unconstrained ? 1 : 0;
  }
  out.srecs.assign((size_t)n_views * C * S_STRIDE, 0.0);
  out.launch.clear();
  for (int v = 0; v < n_views; ++v) {
    const mcba_rig_view& view = views[v];
    if (view.board < 0 || view.board >= n_boards) { snprintf(msg, sizeof msg, "%s: view %d: board %d of %d", who, v, view.board, n_boards); err = msg; return false; }
    if (view.min_points < 0) { snprintf(msg, sizeof msg, "%s: view %d: negative min_points", who, v); err = msg; return false; }
    for (int i = 0; i < 12; ++i)
      if (!finite_arg(view.pose[i])) { snprintf(msg, sizeof msg, "%s: view %d: the pose is not finite", who, v); err = msg; return false; }
    const double* mean = board_mean.data() + 3 * (size_t)view.board;
    for (int c = 0; c < C; ++c) {
      const size_t slot = (size_t)v * C + c;
      double* rec = out.srecs.data() + slot * S_STRIDE;
      const double* Tc = camera_poses + 12 * (size_t)c;
      rec[guidance::V_CAMERA] = (double)c;
      rec[guidance::V_NN] = (double)NN;
      rec[guidance::V_MIN] = (double)view.min_points;
      rec[guidance::V_KIND] = (double)guidance::KIND_BOARD;
      rec[guidance::V_BOARD] = (double)view.board;
      rec[guidance::V_RHO] = 1.0;
      rec[guidance::V_N] = (double)board_n[view.board];
      for (int i = 0; i < 3; ++i)                       // T_c Z
        for (int j = 0; j < 4; ++j)
          rec[guidance::V_POSE + 4 * i + j] = Tc[4 * i] * view.pose[j] + Tc[4 * i + 1] * view.pose[4 + j] + Tc[4 * i + 2] * view.pose[8 + j] +
                                              (j == 3 ? Tc[4 * i + 3] : 0.0);
      slot_centre(rec + guidance::V_POSE, mean, rec + guidance::V_CENTRE);
      double* D = rec + S_D;                              // D_c = blockdiag(R_c, R_c)
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) D[i * NN + j] = D[(3 + i) * NN + 3 + j] = Tc[4 * i + j];
      out.launch.push_back((int32_t)slot);
    }
  }
  out.entries.assign(1, -1);
  for (int v = 0; v < n_views; ++v) out.entries.push_back(v);
  out.nothing = r == 0 || n_views == 0;
  // the focus
  out.n_pairs = 0;
  out.frecs.clear();
  out.Wab.clear();
  out.focus_loose = false;
  if (focus) {
    const int a = focus->reference;
    if (a < 0 || a >= C) { snprintf(msg, sizeof msg, "%s: focus: reference %d of %d", who, a, C); err = msg; return false; }
    if (focus->n_members < 0 || (focus->n_members > 0 && !focus->members)) { err = w + ": focus: members"; return false; }
    if (focus->grid_w <= 0 || focus->grid_h <= 0 || (int64_t)focus->grid_w * focus->grid_h > (1 << 24) || !finite_arg(focus->u0) ||
        !finite_arg(focus->v0) || !finite_arg(focus->du) || !finite_arg(focus->dv)) {
      err = w + ": focus: a grid of 1 .. 2^24 pixels with finite u0, v0, du, dv";
      return false;
    }
    if (!finite_arg(focus->inv_distance) || focus->inv_distance < 0.0) { err = w + ": focus: inv_distance must be finite and >= 0"; return false; }
    out.gw = focus->grid_w; out.gn = focus->grid_w * focus->grid_h;
    out.u0 = focus->u0; out.v0 = focus->v0; out.du = focus->du; out.dv = focus->dv;
    out.focus_loose = out.loose[a] != 0;
    for (int m = 0; m < focus->n_members; ++m) {
      const int b = focus->members[m];
      if (b < 0 || b >= C) { snprintf(msg, sizeof msg, "%s: focus: member %d of %d", who, b, C); err = msg; return false; }
      if (b == a) continue;                           // (the reference sees its own pixel where it is: nothing to transfer)
      out.focus_loose = out.focus_loose || out.loose[b] != 0;
      out.frecs.resize(out.frecs.size() + F_STRIDE, 0.0);
      double* rec = out.frecs.data() + (size_t)out.n_pairs * F_STRIDE;
      const double* eb = plan.cam.data() + (size_t)b * CAM_STRIDE;
      const double* ea = plan.cam.data() + (size_t)a * CAM_STRIDE;
      for (int i = 0; i < CAM_STRIDE; ++i) { rec[uncertainty::REC_CAM_B + i] = eb[i]; rec[uncertainty::REC_CAM_A + i] = ea[i]; }
      rec[uncertainty::REC_RHO] = focus->inv_distance;
      rec[uncertainty::REC_HAS_A] = 1.0;
      const double* Tb = camera_poses + 12 * (size_t)b;
      const double* Ta = camera_poses + 12 * (size_t)a;
      for (int i = 0; i < 3; ++i) {                   // R_ba = R_b R_a^T, t_ba = t_b - R_ba t_a
        for (int k = 0; k < 3; ++k)
          rec[uncertainty::REC_R + 3 * i + k] = Tb[4 * i] * Ta[4 * k] + Tb[4 * i + 1] * Ta[4 * k + 1] + Tb[4 * i + 2] * Ta[4 * k + 2];
        rec[uncertainty::REC_T + i] = Tb[4 * i + 3] - (rec[uncertainty::REC_R + 3 * i] * Ta[3] + rec[uncertainty::REC_R + 3 * i + 1] * Ta[7] +
                                                       rec[uncertainty::REC_R + 3 * i + 2] * Ta[11]);
      }
      // camera b | pose b | pose a | camera a
      out.Wab.resize(out.Wab.size() + (size_t)KP * rs, 0.0);
      double* Wp = out.Wab.data() + (size_t)out.n_pairs * KP * rs;
      const double* Wb = out.W.data() + (size_t)b * KC * rs;
      const double* Wa = out.W.data() + (size_t)a * KC * rs;
      for (int j = 0; j < rs; ++j) {
        for (int k = 0; k < KI; ++k) {
          Wp[(size_t)(uncertainty::COL_CAM_B + k) * rs + j] = Wb[(size_t)k * rs + j];
          Wp[(size_t)(uncertainty::COL_CAM_A + k) * rs + j] = Wa[(size_t)k * rs + j];
        }
        for (int k = 0; k < 6; ++k) {
          Wp[(size_t)(uncertainty::COL_POSE_B + k) * rs + j] = Wb[(size_t)(KI + k) * rs + j];
          Wp[(size_t)(uncertainty::COL_POSE_A + k) * rs + j] = Wa[(size_t)(KI + k) * rs + j];
        }
      }
      ++out.n_pairs;
    }
  }
  return true;
}

// Q [rs][rs] = sum over the pairs of W_ab^T H W_ab: Z = H W_ab, then Q[i][j] += sum_k W_ab[k][i] Z[k][j], pairs and k ascending
inline void fold_focus(const Plan& p, const double* H, double* Q) {
  const int rs = p.rs, r = p.r;
  for (size_t i = 0; i < (size_t)rs * rs; ++i) Q[i] = 0.0;
  std::vector<double> Z((size_t)KP * rs);
  for (int pr = 0; pr < p.n_pairs; ++pr) {
    const double* Hp = H + (size_t)pr * KP * KP;
    const double* Wp = p.Wab.data() + (size_t)pr * KP * rs;
    for (int k = 0; k < KP; ++k)
      for (int j = 0; j < r; ++j) {
        double s = 0.0;
        for (int m = 0; m < KP; ++m) s += Hp[k * KP + m] * Wp[(size_t)m * rs + j];
        Z[(size_t)k * rs + j] = s;
      }
    for (int i = 0; i < r; ++i)
      for (int j = 0; j < r; ++j) {
        double s = Q[(size_t)i * rs + j];
        for (int k = 0; k < KP; ++k) s += Wp[(size_t)k * rs + i] * Z[(size_t)k * rs + j];
        Q[(size_t)i * rs + j] = s;
      }
  }
}
inline int focus_status(const Plan& p, int n_ok) { return p.focus_loose ? ST_UNCONSTRAINED : n_ok > 0 ? ST_OK : ST_TOO_FEW; }

// what the outputs hold before anything is computed (and all they hold after a call with nothing to launch)
inline void fill_defaults(const Plan& p, const mcba_rig_result* res) {
  const double nan = undistort::quiet_nan();
  const size_t rr = (size_t)p.rs * p.rs;
  for (int v = 0; v < p.V; ++v) {
    res->n_cameras[v] = 0;
    for (int c = 0; c < p.C; ++c) res->n_visible[(size_t)v * p.C + c] = 0;
    res->status[v] = (uint8_t)ST_OK;
    res->gain[v] = 0.0;                                   // (r = 0: nothing is left to learn)
    res->focus_rms[v] = 0.0;
  }
  if (res->A) for (size_t i = 0; i < (size_t)p.V * rr; ++i) res->A[i] = 0.0;
  if (res->Q) for (size_t i = 0; i < rr; ++i) res->Q[i] = 0.0;
  if (res->posterior) {
    for (size_t i = 0; i < rr; ++i) res->posterior[i] = 0.0;
    for (int i = 0; i < p.r; ++i) res->posterior[(size_t)i * p.rs + i] = 1.0;
  }
  if (res->focus_status) *res->focus_status = (uint8_t)(p.r == 0 ? ST_OK : ST_TOO_FEW);
  if (res->focus_n) *res->focus_n = 0;
  if (res->focus_before) *res->focus_before = p.r == 0 ? 0.0 : nan;
  for (int k = 0; k < p.n_picks; ++k) {
    res->picks[k] = -1;
    res->pick_gain[k] = nan;
    res->pick_focus_rms[k] = nan;
  }
  for (size_t i = 0; i < (size_t)p.n_picks * p.V; ++i) {
    if (res->round_gain) res->round_gain[i] = nan;
    if (res->round_focus_rms) res->round_focus_rms[i] = nan;
  }
}

// The greedy loop.  Backend: score(n_entries, with_posterior) scores the first n_entries of the list into half_log_det() / focus()
// (host arrays of the list's length; entry 0 is the base alone); add(winner) adds the winner's A to the base.
template <class Backend>
void greedy_rounds(const Plan& p, Backend& be, const mcba_rig_result* res) {
  const size_t ne = p.entries.size();
  const double nan = undistort::quiet_nan();
  std::vector<uint8_t> taken((size_t)p.V, 0);
  int winner = -1;
  for (int round = 0; round <= p.n_picks; ++round) {
    const bool last = round == p.n_picks;
    be.score(last && round > 0 ? (size_t)1 : ne, last && res->posterior != nullptr);
    const double* hld = be.half_log_det();
    const double* focus = be.focus();
    if (round == 0 && res->focus_before) *res->focus_before = focus[0];
    if (round > 0) res->pick_focus_rms[round - 1] = winner >= 0 ? focus[0] : nan;
    if (last && round > 0) break;
    for (size_t e = 1; e < ne; ++e) {
      const int v = p.entries[e];
      const double gain = hld[e] - hld[0];
      if (round == 0) { res->gain[v] = gain; res->focus_rms[v] = focus[e]; }
      if (!last && res->round_gain) res->round_gain[(size_t)round * p.V + v] = gain;
      if (!last && res->round_focus_rms) res->round_focus_rms[(size_t)round * p.V + v] = focus[e];
    }
    if (last) break;
    winner = -1;
    double best = 0.0, best_gain = nan;
    for (size_t e = 1; e < ne; ++e) {
      const int v = p.entries[e];
      const double gain = hld[e] - hld[0];
      const double s = p.criterion == CRIT_GAIN ? gain : -focus[e];
      if (taken[v] || !(s == s) || !(gain == gain)) continue;
      if (winner < 0 || s > best) { winner = v; best = s; best_gain = gain; }
    }
    if (winner < 0) continue;                           // (nothing is left: the later rounds find nothing either)
    taken[winner] = 1;
    res->picks[round] = winner;
    res->pick_gain[round] = best_gain;
    be.add(winner);
  }
}

}  // namespace rigview
}  // namespace mcba
