// TEST INFRASTRUCTURE: g++ build of the view-information mathematics (multical_amd/csrc/mcba_guidance.h) behind the signature of
// mcba_view_information: plain loops over views, points and score-list entries, the Gram matrix summed in point order.  The argument
// checks, the records, the score list and the greedy loop come from the same driver header the API uses.
#include <string>
#include <vector>

#include "../../multical_amd/csrc/mcba_guidance_driver.h"

using namespace mcba;
using namespace mcba::guidance;

static thread_local std::string g_error;

namespace {

struct HostRounds {
  const Plan& plan;
  std::vector<double>& S;             // [V + C][rs][rs]
  const std::vector<int32_t>& nvis;
  const std::vector<uint8_t>& status;
  std::vector<double> B, scores;
  double* posterior;

  const double* gain() const { return scores.data(); }
  const double* focus() const { return scores.data() + plan.entries.size(); }
  void score(size_t n_entries, bool with_posterior) {
    const double nan = undistort::quiet_nan();
    const int rs = plan.rs;
    const size_t rr = (size_t)rs * rs, ne = plan.entries.size();
    for (size_t e = 0; e < n_entries; ++e) {
      const int ent = plan.entries[e];
      const bool null_view = ent < 0;
      const int c = null_view ? -ent - 1 : plan.view_camera[ent], r = plan.cam_r[c];
      double& gain = scores[e];
      double& focus = scores[ne + e];
      gain = focus = nan;
      if (!null_view && status[ent] != ST_OK) continue;
      double Lm[MAX_R * MAX_R], Lb[MAX_R * MAX_R], X[MAX_R * MAX_R], Yw[MAX_R * MAX_R];
      form_lower(r, B.data() + c * rr, null_view ? nullptr : S.data() + ent * rr, rs, plan.inv_s2, Lm);
      form_lower(r, B.data() + c * rr, nullptr, rs, plan.inv_s2, Lb);
      if (!chol_lower(r, Lm) || !chol_lower(r, Lb)) continue;
      const size_t f = (size_t)plan.V + c;
      const bool has_focus = status[f] == ST_OK && nvis[f] > 0;
      gain = half_log_det(r, Lm) - half_log_det(r, Lb);
      if (has_focus) {
        for (int j = 0; j < r; ++j) forward_column(r, Lm, S.data() + f * rr, rs, j, X);
        double trace = 0.0;
        for (int i = 0; i < r; ++i) trace += diagonal_entry(Lm, X, i, Yw);
        focus = focus_rms_of(trace, (double)nvis[f]);
      }
      if (with_posterior && null_view && posterior)
        for (int j = 0; j < r; ++j) inverse_column(r, Lm, j, Yw, posterior + c * rr, rs);
    }
  }
  void add(const int32_t* winners) {
    const size_t rr = (size_t)plan.rs * plan.rs;
    for (int c = 0; c < plan.C; ++c) {
      if (winners[c] < 0) continue;
      const int r = plan.cam_r[c];
      for (int i = 0; i < r; ++i)
        for (int j = 0; j < r; ++j) {
          const size_t at = (size_t)i * plan.rs + j;
          B[c * rr + at] = B[c * rr + at] + plan.inv_s2 * S[winners[c] * rr + at];
        }
    }
  }
};

// one view: S (row stride rs), the visible count and the status
int view_schur(const Plan& plan, int v, double* S, int32_t* n_visible) {
  const double* vrec = plan.vrecs.data() + (size_t)v * V_STRIDE;
  const double* crec = plan.crecs.data() + (size_t)(int)vrec[V_CAMERA] * CREC_STRIDE;
  const int r = (int)crec[CREC_RANK], nn = (int)vrec[V_NN], n = (int)vrec[V_N], cols = r + nn, rs = plan.rs;
  std::vector<double> G((size_t)GS * GS, 0.0);
  int count = 0;
  for (int i = 0; i < n; ++i) {
    double rows[2][MAX_COLS];
    if (!point_rows(crec, vrec, plan.board_points.data(), plan.board_stride, plan.uv.data(), i, r, nn, rows[0], rows[1])) continue;
    ++count;
    for (int h = 0; h < 2; ++h)
      for (int a = 0; a < cols; ++a)
        for (int b = a; b < cols; ++b) G[a * GS + b] += rows[h][a] * rows[h][b];
  }
  double L[MAX_NN * MAX_NN], Y[MAX_NN * MAX_R];
  const bool factored = nn == 0 || nuisance_factor(G.data(), r, nn, L);
  const int status = view_status(count, (int)vrec[V_MIN], factored);
  *n_visible = count;
  if (status == ST_OK)
    for (int c = 0; c < r && nn > 0; ++c) nuisance_column(G.data(), r, nn, L, c, Y);
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < r; ++j) S[(size_t)i * rs + j] = status == ST_OK ? schur_entry(G.data(), nn, Y, i, j) : 0.0;
  return status;
}

}  // namespace

extern "C" {

const char* gdh_last_error(void) { return g_error.c_str(); }

int32_t gdh_view_information(const mcba_camera_set* cams, const mcba_guidance_camera* info, int32_t n_boards, int32_t board_stride,
                             const int32_t* board_n, const double* board_points, double margin, double sigma2, int32_t n_views,
                             const mcba_guidance_view* views, const mcba_guidance_view* foci, int32_t n_picks, int32_t criterion,
                             const mcba_guidance_result* out) {
  Plan plan;
  if (!plan_views(cams, info, n_boards, board_stride, board_n, board_points, margin, sigma2, n_views, views, foci, n_picks, criterion,
                  out, plan, g_error))
    return 1;
  fill_defaults(plan, out);
  if (n_views == 0 || plan.launch.empty()) return 0;
  const size_t N = (size_t)plan.V + plan.C, rr = (size_t)plan.rs * plan.rs;
  std::vector<double> S(N * rr, 0.0);
  std::vector<int32_t> nvis(N, 0);
  std::vector<uint8_t> status(plan.status0);
  for (int v : plan.launch) status[v] = (uint8_t)view_schur(plan, v, S.data() + (size_t)v * rr, &nvis[v]);
  std::vector<double> B((size_t)plan.C * rr, 0.0);
  for (int c = 0; c < plan.C; ++c)
    for (int i = 0; i < plan.cam_r[c]; ++i) B[c * rr + (size_t)i * plan.rs + i] = 1.0;
  HostRounds rounds{plan, S, nvis, status, B, std::vector<double>(2 * plan.entries.size(), 0.0), out->posterior};
  greedy_rounds(plan, rounds, out);
  for (int j = 0; j < plan.V; ++j) { out->n_visible[j] = nvis[j]; out->status[j] = status[j]; }
  if (out->S) for (size_t i = 0; i < (size_t)plan.V * rr; ++i) out->S[i] = S[i];
  for (int c = 0; c < plan.C; ++c) {
    if (out->focus_status) out->focus_status[c] = status[(size_t)plan.V + c];
    if (out->focus_n_visible) out->focus_n_visible[c] = nvis[(size_t)plan.V + c];
    if (out->Q) for (size_t i = 0; i < rr; ++i) out->Q[c * rr + i] = S[((size_t)plan.V + c) * rr + i];
  }
  return 0;
}

}
