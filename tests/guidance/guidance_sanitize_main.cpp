// TEST INFRASTRUCTURE: stand-alone program around the host build of the view-information mathematics, compiled by
// tests/test_guidance_host.py with -fsanitize=address,undefined and run on the CPU.  Every input and every output is a heap block of
// exactly its size, so a read or a store outside it stops the program.  Three cameras (5 and 4 Brown-Conrady coefficients, one
// Kannala-Brandt) serve the edge cases: board views with 0, 3 and 6 nuisance parameters, pixel views as candidates, foci as grids
// and lists, a board whose row of the table is shorter than the stride, a view outside the image, one behind the camera, collinear
// points, a camera with r = 0 and one with a loose intrinsic, every optional output left out, more picks than candidates, an empty
// call and calls that are refused.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "guidance.cpp"

static const int C = 3, ND = 5, STRIDE = 5 + ND;

template <class T>
static T* block(size_t n) { return (T*)calloc(n > 0 ? n : 1, sizeof(T)); }

static mcba_guidance_view board_view(int camera, int board, int nn, int min_points, double x, double z) {
  mcba_guidance_view v = {};
  v.camera = camera; v.board = board; v.n_nuisance = nn; v.min_points = min_points;
  const double c = cos(0.3), s = sin(0.3);
  const double T[12] = {c, 0.0, s, x, 0.0, 1.0, 0.0, 0.01, -s, 0.0, c, z};
  memcpy(v.pose, T, sizeof T);
  return v;
}

static int run(int n_views, const mcba_guidance_view* views_in, const int* r_of, int loose_camera, bool with_foci, bool focus_list,
               int n_picks, int criterion, bool optional, double sigma2, int want_rc, const int* want_status) {
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
  mcba_guidance_camera* info = block<mcba_guidance_camera>(C);
  double* W[C];
  int rs = 1;
  for (int c = 0; c < C; ++c) {
    const int ki = 4 + (fish[c] ? 4 : nd[c]), r = r_of[c];
    W[c] = r > 0 ? block<double>((size_t)ki * r) : nullptr;
    unsigned s = 99u + 31u * c + r;
    for (int i = 0; i < ki * r; ++i) { s = s * 1664525u + 1013904223u; W[c][i] = (i < 4 * r ? 0.3 : 3e-4) * ((double)(s >> 8) / 16777216.0 - 0.5); }
    info[c].r = r; info[c].unconstrained = c == loose_camera; info[c].W = W[c]; info[c].image_w = 200.0; info[c].image_h = 150.0;
    if (r > rs) rs = r;
  }
  // two boards in a table of stride 30: a 5 x 5 grid, and 7 collinear points
  const int n_boards = 2, stride = 30;
  int32_t* board_n = block<int32_t>(n_boards);
  board_n[0] = 25; board_n[1] = 7;
  double* pts = block<double>((size_t)n_boards * stride * 3);
  for (int i = 0; i < 25; ++i) { pts[3 * i] = 0.02 * (i % 5 - 2); pts[3 * i + 1] = 0.02 * (i / 5 - 2); }
  for (int i = 0; i < 7; ++i) pts[3 * (stride + i)] = 0.015 * (i - 3);
  mcba_guidance_view* views = block<mcba_guidance_view>(n_views);
  if (n_views > 0) memcpy(views, views_in, (size_t)n_views * sizeof(mcba_guidance_view));
  const double list[12] = {100.0, 75.0, 10.0, 10.0, 190.0, 140.0, 30.0, 120.0, NAN, 5.0, 1e9, -1e9};
  double* uv = block<double>(12);
  memcpy(uv, list, sizeof list);
  for (int j = 0; j < n_views; ++j)
    if (views[j].board < 0 && views[j].grid_w == 0) views[j].uv = uv;
  mcba_guidance_view* foci = with_foci ? block<mcba_guidance_view>(C) : nullptr;
  for (int c = 0; with_foci && c < C; ++c) {
    foci[c].camera = c == 1 ? -1 : c; foci[c].board = -1; foci[c].n_nuisance = 3; foci[c].min_points = 3;
    if (focus_list) { foci[c].n = 6; foci[c].uv = uv; }
    else { foci[c].grid_w = 7; foci[c].grid_h = 5; foci[c].u0 = 10.0; foci[c].v0 = 10.0; foci[c].du = 30.0; foci[c].dv = 32.0; }
  }
  const size_t rr = (size_t)rs * rs, V = (size_t)n_views, NP = (size_t)n_picks;
  mcba_guidance_result out = {};
  out.n_visible = block<int32_t>(V); out.status = block<uint8_t>(V); out.gain = block<double>(V); out.focus_rms = block<double>(V);
  out.picks = block<int32_t>(C * NP); out.pick_gain = block<double>(C * NP); out.pick_focus_rms = block<double>(C * NP);
  if (optional) {
    out.S = block<double>(V * rr); out.focus_status = block<uint8_t>(C); out.focus_n_visible = block<int32_t>(C);
    out.focus_before = block<double>(C); out.Q = block<double>(C * rr); out.posterior = block<double>(C * rr);
    out.round_gain = block<double>(NP * V); out.round_focus_rms = block<double>(NP * V);
  }
  const int rc = gdh_view_information(&cams, info, n_boards, stride, board_n, pts, 2.0, sigma2, n_views, views, foci, n_picks,
                                      criterion, &out);
  int bad = 0;
  if ((rc != 0) != (want_rc != 0)) { fprintf(stderr, "rc %d, expected %d: %s\n", rc, want_rc, gdh_last_error()); bad = 1; }
  for (int j = 0; rc == 0 && want_status && j < n_views; ++j) {
    if (out.status[j] != want_status[j]) { fprintf(stderr, "view %d: status %d, expected %d\n", j, out.status[j], want_status[j]); bad = 1; }
    const bool ok = out.status[j] == MCBA_GUIDE_OK;
    if (ok != (out.gain[j] == out.gain[j]) || (ok && !(out.gain[j] >= 0.0))) { fprintf(stderr, "view %d: gain %g\n", j, out.gain[j]); bad = 1; }
  }
  for (size_t i = 0; rc == 0 && i < C * NP; ++i)
    if (out.picks[i] < -1 || out.picks[i] >= n_views) { fprintf(stderr, "pick %d\n", out.picks[i]); bad = 1; }
  free(cams_blk); free(nd); free(fish); free(info); free(board_n); free(pts); free(views); free(uv); free(foci);
  for (int c = 0; c < C; ++c) free(W[c]);
  free(out.n_visible); free(out.status); free(out.gain); free(out.focus_rms); free(out.picks); free(out.pick_gain);
  free(out.pick_focus_rms); free(out.S); free(out.focus_status); free(out.focus_n_visible); free(out.focus_before); free(out.Q);
  free(out.posterior); free(out.round_gain); free(out.round_focus_rms);
  return bad;
}

int main() {
  const int OK = MCBA_GUIDE_OK, FEW = MCBA_GUIDE_TOO_FEW, DEG = MCBA_GUIDE_DEGENERATE, UNC = MCBA_GUIDE_UNCONSTRAINED;
  mcba_guidance_view pixels = {};
  pixels.camera = 0; pixels.board = -1; pixels.n_nuisance = 3; pixels.min_points = 2; pixels.n = 6;
  mcba_guidance_view grid = {};
  grid.camera = 2; grid.board = -1; grid.n_nuisance = 6; grid.min_points = 4; grid.inv_distance = 0.5; grid.grid_w = 9; grid.grid_h = 8;
  grid.u0 = 4.0; grid.v0 = 3.0; grid.du = 24.0; grid.dv = 20.0;
  const mcba_guidance_view views[] = {board_view(0, 0, 6, 4, 0.0, 0.4),  board_view(0, 0, 3, 4, 0.02, 0.5), board_view(0, 0, 0, 4, -0.02, 0.45),
                                      board_view(0, 0, 6, 26, 0.0, 0.4), board_view(0, 0, 6, 1, 4.0, 0.4),  board_view(0, 0, 6, 1, 0.0, -0.4),
                                      board_view(0, 1, 6, 4, 0.0, 0.4),  board_view(1, 0, 6, 4, 0.0, 0.4),  board_view(2, 0, 6, 4, 0.0, 0.4),
                                      pixels, grid};
  const int n = (int)(sizeof views / sizeof views[0]);
  const int full[3] = {9, 8, 8}, held[3] = {5, 0, 8}, none[3] = {0, 0, 0}, wide[3] = {18, 3, 1};
  const int st_full[] = {OK, OK, OK, FEW, FEW, FEW, DEG, OK, OK, OK, OK};
  const int st_held[] = {OK, OK, OK, FEW, FEW, FEW, DEG, OK, OK, OK, OK};
  const int st_loose[] = {OK, OK, OK, FEW, FEW, FEW, DEG, UNC, OK, OK, OK};
  const int st_none[] = {OK, OK, OK, OK, OK, OK, OK, OK, OK, OK, OK};
  int bad = 0;
  for (int optional = 0; optional <= 1; ++optional) {
    bad += run(n, views, full, -1, true, false, 3, MCBA_GUIDE_BY_FOCUS, optional != 0, 0.25, 0, st_full);
    bad += run(n, views, held, -1, true, true, 2, MCBA_GUIDE_BY_GAIN, optional != 0, 1.0, 0, st_held);
    bad += run(n, views, full, 1, true, false, 12, MCBA_GUIDE_BY_GAIN, optional != 0, 1.0, 0, st_loose);      // more picks than candidates
    bad += run(n, views, wide, -1, false, false, 1, MCBA_GUIDE_BY_GAIN, optional != 0, 4.0, 0, st_full);
    bad += run(n, views, none, -1, true, false, 1, MCBA_GUIDE_BY_FOCUS, optional != 0, 1.0, 0, st_none);       // r = 0 everywhere
    bad += run(n, views, full, -1, true, false, 0, MCBA_GUIDE_BY_FOCUS, optional != 0, 1.0, 0, st_full);       // no pick
    bad += run(0, nullptr, full, -1, true, false, 2, MCBA_GUIDE_BY_FOCUS, optional != 0, 1.0, 0, nullptr);     // no view
  }
  bad += run(n, views, full, -1, true, false, 1, 2, true, 1.0, 1, nullptr);                   // refused: criterion
  bad += run(n, views, full, -1, true, false, 1, MCBA_GUIDE_BY_GAIN, true, 0.0, 1, nullptr);  // refused: sigma2
  bad += run(n, views, full, -1, true, false, 1, MCBA_GUIDE_BY_GAIN, true, NAN, 1, nullptr);
  mcba_guidance_view wrong[3] = {board_view(3, 0, 6, 4, 0.0, 0.4), board_view(0, 2, 6, 4, 0.0, 0.4), board_view(0, 0, 5, 4, 0.0, 0.4)};
  for (int i = 0; i < 3; ++i) bad += run(1, wrong + i, full, -1, true, false, 1, MCBA_GUIDE_BY_GAIN, true, 1.0, 1, nullptr);
  const int too_wide[3] = {19, 1, 1};
  bad += run(n, views, too_wide, -1, true, false, 1, MCBA_GUIDE_BY_GAIN, true, 1.0, 1, nullptr);
  if (bad) { fprintf(stderr, "a case failed\n"); return 1; }
  printf("guidance sanitize run: ok\n");
  return 0;
}
