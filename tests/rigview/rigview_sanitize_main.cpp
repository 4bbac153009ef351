// TEST INFRASTRUCTURE: stand-alone program around the host build of the rig-view mathematics, compiled by
// tests/test_rig_guidance_host.py with -fsanitize=address,undefined and run on the CPU.  Every input and every output is a heap block
// of exactly its size, so a read or a store outside it stops the program.  Three cameras side by side (5 and 4 Brown-Conrady
// coefficients, one Kannala-Brandt) serve the edge cases: views that all, two, one and none of them see, a camera below min_points,
// min_cameras above what contributes, collinear points and a single point, a board whose row of the table is shorter than the stride,
// a loose camera, r = 1, an odd r and the widest r, every optional output left out, more picks than candidates, no focus, a focus at
// infinity, r = 0, an empty call and the calls that are refused.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rigview.cpp"

static const int C = 3, ND = 5, STRIDE = 5 + ND;

template <class T>
static T* block(size_t n) { return (T*)calloc(n > 0 ? n : 1, sizeof(T)); }

static mcba_rig_view rig_view(int board, int min_points, double x, double z) {
  mcba_rig_view v = {};
  v.board = board; v.min_points = min_points;
  const double c = cos(0.3), s = sin(0.3);
  const double T[12] = {c, 0.0, s, x, 0.0, 1.0, 0.0, 0.01, -s, 0.0, c, z};
  memcpy(v.pose, T, sizeof T);
  return v;
}

static int run(int n_views, const mcba_rig_view* views_in, int r, int loose_camera, int focus_kind, int n_picks, int criterion,
               bool optional, double sigma2, int min_cameras, int boards, int workspace_mb, int want_rc, const int* want_status,
               const int* want_cameras) {
  double* cams_blk = block<double>((size_t)C * STRIDE);
  const double blocks[3][10] = {{200.0, 205.0, 100.0, 75.0, 0.0, -0.12, 0.3, 1e-3, -1e-3, -0.2},
                                {210.0, 200.0, 98.0, 77.0, 0.0, -0.1, 0.2, 1e-3, 1e-3, 0.0},
                                {190.0, 195.0, 101.0, 74.0, 0.0, 0.05, 0.01, -0.005, 0.001, 0.0}};
  for (int c = 0; c < C; ++c)
    for (int i = 0; i < STRIDE; ++i) cams_blk[c * STRIDE + i] = blocks[c][i];
  int32_t* nd = block<int32_t>(C);
  uint8_t* fish = block<uint8_t>(C);
  nd[0] = 5; nd[1] = 4; nd[2] = 4; fish[2] = 1;
  mcba_camera_set cams = {C, cams_blk, ND, nd, fish};
  double* poses = block<double>((size_t)C * 12);
  for (int c = 0; c < C; ++c) {
    const double a = 0.1 * (c - 1), ca = cos(a), sa = sin(a);
    const double T[12] = {ca, 0.0, sa, -0.06 * (c - 1), 0.0, 1.0, 0.0, 0.002 * c, -sa, 0.0, ca, 0.0};
    memcpy(poses + 12 * c, T, sizeof T);
  }
  mcba_rig_camera* info = block<mcba_rig_camera>(C);
  double* W[C];
  for (int c = 0; c < C; ++c) {
    const int ki = 4 + (fish[c] ? 4 : nd[c]);
    W[c] = r > 0 ? block<double>((size_t)MCBA_RIG_COLUMNS * r) : nullptr;
    unsigned s = 99u + 31u * c + r;
    for (int k = 0; k < MCBA_RIG_COLUMNS && r > 0; ++k)
      for (int j = 0; j < r; ++j) {
        s = s * 1664525u + 1013904223u;
        const bool mine = k < ki || k >= 18;
        W[c][k * r + j] = mine ? (k < 4 ? 0.3 : 3e-4) * ((double)(s >> 8) / 16777216.0 - 0.5) : 0.0;
      }
    info[c].unconstrained = c == loose_camera; info[c].W = W[c]; info[c].image_w = 200.0; info[c].image_h = 150.0;
  }
  // three boards in a table of stride 30: a 5 x 5 grid, 7 collinear points, one point
  const int n_boards = 3, stride = 30;
  int32_t* board_n = block<int32_t>(n_boards);
  board_n[0] = 25; board_n[1] = 7; board_n[2] = 1;
  double* pts = block<double>((size_t)n_boards * stride * 3);
  for (int i = 0; i < 25; ++i) { pts[3 * i] = 0.02 * (i % 5 - 2); pts[3 * i + 1] = 0.02 * (i / 5 - 2); }
  for (int i = 0; i < 7; ++i) pts[3 * (stride + i)] = 0.015 * (i - 3);
  mcba_rig_view* views = block<mcba_rig_view>(n_views);
  if (n_views > 0) memcpy(views, views_in, (size_t)n_views * sizeof(mcba_rig_view));
  int32_t* members = block<int32_t>(C);
  for (int c = 0; c < C; ++c) members[c] = c;
  mcba_rig_focus* focus = focus_kind ? block<mcba_rig_focus>(1) : nullptr;
  if (focus) {
    focus->reference = 1; focus->n_members = C; focus->members = members; focus->grid_w = 7; focus->grid_h = 5;
    focus->u0 = 10.0; focus->v0 = 10.0; focus->du = 30.0; focus->dv = 32.0; focus->inv_distance = focus_kind == 1 ? 0.0 : 1.5;
  }
  const int rs = r > 0 ? r : 1;
  const size_t rr = (size_t)rs * rs, V = (size_t)n_views, NP = (size_t)n_picks;
  mcba_rig_result out = {};
  out.n_cameras = block<int32_t>(V); out.n_visible = block<int32_t>(V * C); out.status = block<uint8_t>(V); out.gain = block<double>(V);
  out.focus_rms = block<double>(V); out.picks = block<int32_t>(NP); out.pick_gain = block<double>(NP); out.pick_focus_rms = block<double>(NP);
  if (optional && want_rc == 0) {
    out.A = block<double>(V * rr); out.focus_status = block<uint8_t>(1); out.focus_n = block<int32_t>(1); out.focus_before = block<double>(1);
    out.Q = block<double>(rr); out.posterior = block<double>(rr); out.round_gain = block<double>(NP * V);
    out.round_focus_rms = block<double>(NP * V);
  }
  const int rc = rvh_rig_view_information(&cams, poses, r, info, boards, n_boards, stride, board_n, pts, n_views, views, min_cameras, 2.0,
                                          sigma2, focus, n_picks, criterion, workspace_mb, &out);
  int bad = 0;
  if ((rc != 0) != (want_rc != 0)) { fprintf(stderr, "rc %d, expected %d: %s\n", rc, want_rc, rvh_last_error()); bad = 1; }
  for (int j = 0; rc == 0 && want_status && j < n_views; ++j) {
    if (out.status[j] != want_status[j]) { fprintf(stderr, "view %d: status %d, expected %d\n", j, out.status[j], want_status[j]); bad = 1; }
    if (want_cameras && out.n_cameras[j] != want_cameras[j]) { fprintf(stderr, "view %d: %d cameras, expected %d\n", j, out.n_cameras[j], want_cameras[j]); bad = 1; }
    const bool ok = out.status[j] == MCBA_GUIDE_OK;
    if (ok != (out.gain[j] == out.gain[j]) || (ok && !(out.gain[j] >= 0.0))) { fprintf(stderr, "view %d: gain %g\n", j, out.gain[j]); bad = 1; }
  }
  for (size_t i = 0; rc == 0 && i < NP; ++i)
    if (out.picks[i] < -1 || out.picks[i] >= n_views) { fprintf(stderr, "pick %d\n", out.picks[i]); bad = 1; }
  free(cams_blk); free(nd); free(fish); free(poses); free(info); free(board_n); free(pts); free(views); free(members); free(focus);
  for (int c = 0; c < C; ++c) free(W[c]);
  free(out.n_cameras); free(out.n_visible); free(out.status); free(out.gain); free(out.focus_rms); free(out.picks); free(out.pick_gain);
  free(out.pick_focus_rms); free(out.A); free(out.focus_status); free(out.focus_n); free(out.focus_before); free(out.Q);
  free(out.posterior); free(out.round_gain); free(out.round_focus_rms);
  return bad;
}

int main() {
  const int OK = MCBA_GUIDE_OK, FEW = MCBA_GUIDE_TOO_FEW, DEG = MCBA_GUIDE_DEGENERATE, UNC = MCBA_GUIDE_UNCONSTRAINED;
  // all see it | the left two | camera 1 below min_points | off to the side | behind | collinear | one point
  const mcba_rig_view views[] = {rig_view(0, 4, 0.0, 0.7),  rig_view(0, 4, -0.12, 0.5), rig_view(0, 26, 0.0, 0.7), rig_view(0, 1, 4.0, 0.5),
                                 rig_view(0, 1, 0.0, -0.5), rig_view(1, 4, 0.0, 0.7),   rig_view(2, 1, 0.0, 0.7)};
  const int n = (int)(sizeof views / sizeof views[0]);
  const int st_two[] = {OK, OK, FEW, FEW, FEW, DEG, DEG};
  const int st_four[] = {FEW, FEW, FEW, FEW, FEW, FEW, FEW};
  const int st_loose[] = {UNC, UNC, FEW, FEW, FEW, UNC, UNC};
  const int st_none[] = {OK, OK, OK, OK, OK, OK, OK};
  int bad = 0;
  for (int optional = 0; optional <= 1; ++optional) {
    const bool o = optional != 0;
    bad += run(n, views, 20, -1, 2, 3, MCBA_GUIDE_BY_FOCUS, o, 0.25, 2, 0, 64, 0, st_two, nullptr);
    bad += run(n, views, 17, -1, 1, 2, MCBA_GUIDE_BY_GAIN, o, 1.0, 2, 0, 64, 0, st_two, nullptr);             // focus at infinity, odd r
    bad += run(n, views, 1, -1, 2, 9, MCBA_GUIDE_BY_GAIN, o, 1.0, 2, 0, 64, 0, st_two, nullptr);              // more picks than candidates
    bad += run(n, views, 128, -1, 0, 1, MCBA_GUIDE_BY_GAIN, o, 4.0, 2, 0, 64, 0, st_two, nullptr);            // the widest factor, no focus
    bad += run(n, views, 20, -1, 2, 1, MCBA_GUIDE_BY_FOCUS, o, 1.0, 4, 0, 64, 0, st_four, nullptr);           // min_cameras above the group
    bad += run(n, views, 20, 1, 2, 1, MCBA_GUIDE_BY_FOCUS, o, 1.0, 2, 0, 64, 0, st_loose, nullptr);           // a loose camera
    bad += run(n, views, 0, -1, 2, 1, MCBA_GUIDE_BY_FOCUS, o, 1.0, 2, 0, 64, 0, st_none, nullptr);            // r = 0
    bad += run(n, views, 20, -1, 2, 0, MCBA_GUIDE_BY_FOCUS, o, 1.0, 2, 0, 64, 0, st_two, nullptr);            // no pick
    bad += run(0, nullptr, 20, -1, 2, 2, MCBA_GUIDE_BY_FOCUS, o, 1.0, 2, 0, 64, 0, nullptr, nullptr);         // no view
  }
  bad += run(n, views, 129, -1, 2, 1, MCBA_GUIDE_BY_GAIN, true, 1.0, 2, 0, 64, 1, nullptr, nullptr);          // refused: r
  bad += run(n, views, 128, -1, 2, 1, MCBA_GUIDE_BY_GAIN, true, 1.0, 2, 0, 0, 1, nullptr, nullptr);           // refused: the workspace
  bad += run(n, views, 20, -1, 2, 1, MCBA_GUIDE_BY_GAIN, true, 1.0, 2, 1, 64, 1, nullptr, nullptr);           // refused: boards
  bad += run(n, views, 20, -1, 2, 1, 2, true, 1.0, 2, 0, 64, 1, nullptr, nullptr);                            // refused: criterion
  bad += run(n, views, 20, -1, 2, 1, MCBA_GUIDE_BY_GAIN, true, 0.0, 2, 0, 64, 1, nullptr, nullptr);           // refused: sigma2
  bad += run(n, views, 20, -1, 2, 1, MCBA_GUIDE_BY_GAIN, true, 1.0, 0, 0, 64, 1, nullptr, nullptr);           // refused: min_cameras
  const mcba_rig_view wrong = rig_view(3, 4, 0.0, 0.7);
  bad += run(1, &wrong, 20, -1, 2, 1, MCBA_GUIDE_BY_GAIN, true, 1.0, 2, 0, 64, 1, nullptr, nullptr);          // refused: the board
  if (bad) { fprintf(stderr, "a case failed\n"); return 1; }
  printf("rigview sanitize: ok\n");
  return 0;
}
