// TEST INFRASTRUCTURE: stand-alone program around the host build of the projection-difference mathematics, compiled by
// tests/test_projection_diff_host.py with -fsanitize=address,undefined and run on the CPU.  Every input and every output is a heap
// block of exactly its size, so a read or a store outside it stops the program.  Three cameras (5 and 4 Brown-Conrady coefficients,
// one Kannala-Brandt) under two calibrations serve the edge cases: every fit mode, fit sets of 0, 1, 2, 3 and 65 pixels as a list
// and as a grid, a focus disc with nothing inside, pixels that are not finite or outside the model among fit pixels and queries, a
// transfer job, the same camera twice, a point behind the camera, the optional outputs left out, an empty call and refused calls.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "projdiff_host.cpp"

static const int C = 3, ND = 5, STRIDE = 5 + ND;
static double* g_cams[2];
static int32_t* g_nd;
static uint8_t* g_fish;
static double* g_poses[2];

static double* heap_copy(const double* src, size_t n) {
  double* p = (double*)malloc((n > 0 ? n : 1) * sizeof(double));
  if (n > 0) memcpy(p, src, n * sizeof(double));
  return p;
}

// one job: fit set = list of n_fit pixels (fit_grid: a 13 x 5 grid instead), queries = list of n_q pixels (grid: 9 x 7)
static int run(int b, int a, double rho, int mode, const double* fit_list, int n_fit, bool fit_grid, double focus_radius,
               const double* q_list, int n_q, bool grid, bool optional, int want_rc, int want_fit_status, int want_status0) {
  mcba_projdiff_job job = {};
  job.camera = b; job.reference = a; job.inv_distance = rho; job.fit = mode;
  double* fit_uv = heap_copy(fit_list, (size_t)n_fit * 2);
  double* uv = heap_copy(q_list, (size_t)n_q * 2);
  if (fit_grid) { job.fit_grid_w = 13; job.fit_grid_h = 5; job.fit_u0 = 20.0; job.fit_v0 = 30.0; job.fit_du = 12.5; job.fit_dv = 20.0; }
  else { job.fit_n = n_fit; job.fit_uv = fit_uv; }
  job.focus_u = 100.0; job.focus_v = 75.0; job.focus_radius = focus_radius;
  int64_t n = n_q;
  if (grid) { job.grid_w = 9; job.grid_h = 7; job.u0 = 5.0; job.v0 = 4.0; job.du = 23.0; job.dv = 21.0; n = 63; }
  else { job.n = n_q; job.uv = uv; }
  const size_t N = (size_t)(n > 0 ? n : 1);
  double* transform = optional ? (double*)malloc(6 * sizeof(double)) : nullptr;
  double* fit_info = (double*)malloc(5 * sizeof(double));
  double* diff = (double*)malloc(N * 2 * sizeof(double));
  double* mag = optional ? (double*)malloc(N * sizeof(double)) : nullptr;
  double* landing = optional ? (double*)malloc(N * 2 * sizeof(double)) : nullptr;
  uint8_t* status = (uint8_t*)malloc(N);
  mcba_camera_set c0 = {C, g_cams[0], ND, g_nd, g_fish}, c1 = {C, g_cams[1], ND, g_nd, g_fish};
  const int rc = phd_projection_diff(&c0, g_poses[0], &c1, g_poses[1], 1, &job, transform, fit_info, diff, mag, landing, status);
  int bad = 0;
  if ((rc != 0) != (want_rc != 0)) { fprintf(stderr, "rc %d, expected %d: %s\n", rc, want_rc, phd_last_error()); bad = 1; }
  if (rc == 0 && n > 0) {
    if (want_fit_status >= 0 && (int)fit_info[4] != want_fit_status) {
      fprintf(stderr, "job (%d, %d, rho %g, mode %d): fit status %d, expected %d\n", b, a, rho, mode, (int)fit_info[4], want_fit_status);
      bad = 1;
    }
    if (want_status0 >= 0 && status[0] != want_status0) {
      fprintf(stderr, "job (%d, %d, rho %g, mode %d): status %d, expected %d\n", b, a, rho, mode, status[0], want_status0);
      bad = 1;
    }
    if (want_status0 == MCBA_PDIFF_OK && !(diff[0] == diff[0] && diff[1] == diff[1])) { fprintf(stderr, "NaN with status OK\n"); bad = 1; }
    if (want_status0 > 0 && diff[0] == diff[0]) { fprintf(stderr, "no NaN with status %d\n", want_status0); bad = 1; }
    if (a == b && want_status0 == MCBA_PDIFF_OK && (diff[0] != 0.0 || diff[1] != 0.0)) { fprintf(stderr, "not exactly 0\n"); bad = 1; }
    if (optional && a >= 0 && want_status0 == MCBA_PDIFF_OK && !(landing[0] == landing[0])) { fprintf(stderr, "no landing\n"); bad = 1; }
    if (optional && want_fit_status > 0 && transform[0] == transform[0]) { fprintf(stderr, "a failed fit has a transform\n"); bad = 1; }
  }
  free(fit_uv); free(uv); free(transform); free(fit_info); free(diff); free(mag); free(landing); free(status);
  return bad;
}

int main() {
  const double blocks[2][3][10] = {{{200.0, 205.0, 100.0, 75.0, 0.0, -0.12, 0.3, 1e-3, -1e-3, -0.2},
                                    {210.0, 200.0, 98.0, 77.0, 0.0, -0.1, 0.2, 1e-3, 1e-3, 0.0},
                                    {190.0, 195.0, 101.0, 74.0, 0.0, 0.05, 0.01, -0.005, 0.001, 0.0}},
                                   {{200.2, 204.9, 102.0, 73.5, 0.0, -0.125, 0.31, 1.1e-3, -0.9e-3, -0.19},
                                    {209.8, 200.1, 96.5, 78.0, 0.0, -0.105, 0.19, 0.9e-3, 1.1e-3, 0.0},
                                    {190.1, 194.8, 102.5, 75.5, 0.0, 0.052, 0.0095, -0.0052, 0.00105, 0.0}}};
  for (int k = 0; k < 2; ++k) {
    g_cams[k] = (double*)calloc((size_t)C * STRIDE, sizeof(double));
    for (int c = 0; c < C; ++c)
      for (int i = 0; i < STRIDE; ++i) g_cams[k][c * STRIDE + i] = blocks[k][c][i];
    g_poses[k] = (double*)calloc((size_t)C * 16, sizeof(double));
    for (int c = 0; c < C; ++c) {
      double* T = g_poses[k] + 16 * c;
      T[0] = T[5] = T[10] = T[15] = 1.0;
      T[3] = -0.1 * (c - 1) + 1e-3 * k;
    }
  }
  g_nd = (int32_t*)malloc(C * sizeof(int32_t));
  g_fish = (uint8_t*)malloc(C);
  g_nd[0] = 5; g_nd[1] = 4; g_nd[2] = 4;
  g_fish[0] = 0; g_fish[1] = 0; g_fish[2] = 1;
  double fit65[130];
  for (int i = 0; i < 65; ++i) { fit65[2 * i] = 30.0 + 2.1 * i; fit65[2 * i + 1] = 20.0 + 1.7 * ((i * 7) % 65); }
  double mixed[16];
  memcpy(mixed, fit65, 10 * sizeof(double));
  mixed[10] = NAN; mixed[11] = 10.0; mixed[12] = 1e9; mixed[13] = -1e9; mixed[14] = 5000.0; mixed[15] = 4000.0;
  const double centre[2] = {100.0, 75.0};
  const double pixels[10] = {100.0, 75.0, 0.0, 0.0, 199.0, 149.0, NAN, 10.0, 1e9, -1e9};
  const double outside[2] = {5000.0, 4000.0};
  const int NONE = MCBA_PDIFF_MODE_NONE, ROT = MCBA_PDIFF_MODE_ROTATION, RIGID = MCBA_PDIFF_MODE_RIGID;
  const int OK = MCBA_PDIFF_OK, FOK = MCBA_PDIFF_FIT_OK, FEW = MCBA_PDIFF_FIT_TOO_FEW;
  int bad = 0;
  for (int optional = 0; optional <= 1; ++optional) {
    for (int b = 0; b < C; ++b) {
      bad += run(b, -1, 0.0, ROT, fit65, 65, false, 0.0, pixels, 5, false, optional != 0, 0, FOK, OK);
      bad += run(b, -1, 0.5, RIGID, fit65, 65, false, 0.0, nullptr, 0, true, optional != 0, 0, FOK, OK);
      bad += run(b, -1, 2.0, RIGID, nullptr, 0, true, 0.0, pixels, 5, false, optional != 0, 0, FOK, OK);
      bad += run(b, -1, 0.5, NONE, nullptr, 0, false, 0.0, pixels, 5, false, optional != 0, 0, FOK, OK);
      bad += run(b, (b + 1) % C, 0.5, NONE, nullptr, 0, false, 0.0, pixels, 5, false, optional != 0, 0, FOK, OK);
    }
  }
  bad += run(0, -1, 0.0, ROT, fit65, 0, false, 0.0, centre, 1, false, true, 0, FEW, MCBA_PDIFF_NO_FIT);    // fit sets of 0, 1, 2, 3
  bad += run(0, -1, 0.0, ROT, fit65, 1, false, 0.0, centre, 1, false, true, 0, FEW, MCBA_PDIFF_NO_FIT);
  bad += run(0, -1, 0.0, ROT, fit65, 2, false, 0.0, centre, 1, false, true, 0, FOK, OK);
  bad += run(0, -1, 0.5, RIGID, fit65, 2, false, 0.0, centre, 1, false, true, 0, FEW, MCBA_PDIFF_NO_FIT);
  bad += run(0, -1, 0.5, RIGID, fit65, 3, false, 0.0, centre, 1, false, true, 0, FOK, OK);
  bad += run(1, -1, 0.5, RIGID, nullptr, 0, true, 1e-3, centre, 1, false, true, 0, FEW, MCBA_PDIFF_NO_FIT);  // nothing inside the disc
  bad += run(1, -1, 0.5, RIGID, nullptr, 0, true, 60.0, centre, 1, false, true, 0, FOK, OK);
  bad += run(2, -1, 0.0, ROT, mixed, 8, false, 0.0, outside, 1, false, true, 0, FOK, MCBA_PDIFF_NOT_CONVERGED);
  bad += run(1, 1, 2.0, NONE, nullptr, 0, false, 0.0, pixels, 5, false, true, 0, FOK, OK);                   // the same camera: exactly 0
  bad += run(0, 2, 1.0, NONE, nullptr, 0, false, 0.0, outside, 1, false, true, 0, FOK, MCBA_PDIFF_NOT_CONVERGED);
  bad += run(0, -1, 1.0, ROT, fit65, 65, false, 0.0, centre, 0, false, true, 0, -1, -1);                      // no query
  bad += run(0, -1, 0.0, RIGID, fit65, 65, false, 0.0, centre, 1, false, true, 1, -1, -1);                    // refused: rigid at rho = 0
  bad += run(0, -1, -1.0, ROT, fit65, 65, false, 0.0, centre, 1, false, true, 1, -1, -1);                     // refused: rho < 0
  bad += run(0, -1, NAN, ROT, fit65, 65, false, 0.0, centre, 1, false, true, 1, -1, -1);
  bad += run(0, 3, 1.0, NONE, nullptr, 0, false, 0.0, centre, 1, false, true, 1, -1, -1);                     // refused: reference out of range
  bad += run(0, -1, 1.0, 5, fit65, 65, false, 0.0, centre, 1, false, true, 1, -1, -1);                        // refused: fit mode
  double* T = g_poses[1] + 16 * 2;                                                                            // behind: camera 2 turned round
  T[0] = -1.0; T[10] = -1.0;
  bad += run(2, 0, 1.0, NONE, nullptr, 0, false, 0.0, centre, 1, false, true, 0, FOK, MCBA_PDIFF_BEHIND);
  // the header's fit function on a planted transform, fit pixels outside the model among them
  {
    mcba_projdiff_job job = {};
    job.camera = 2; job.reference = -1; job.inv_distance = 0.0; job.fit = ROT;
    double* fit_uv = heap_copy(mixed, 16);
    job.fit_n = 8; job.fit_uv = fit_uv;
    double* planted = (double*)malloc(6 * sizeof(double));
    const double p[6] = {3e-3, -2e-3, 1.5e-3, 0.0, 0.0, 0.0};
    memcpy(planted, p, sizeof p);
    double* fit = (double*)malloc(FIT_STRIDE * sizeof(double));
    uint8_t* valid = (uint8_t*)malloc(8);
    mcba_camera_set c0 = {C, g_cams[0], ND, g_nd, g_fish}, c1 = {C, g_cams[1], ND, g_nd, g_fish};
    if (phd_fit_planted(&c0, &c1, &job, planted, fit, valid) != 0 || (int)fit[FIT_STATUS] != FOK || (int)fit[FIT_NFIT] != 5 || valid[5] ||
        valid[6] || valid[7]) {
      fprintf(stderr, "planted fit: %s, status %d, n_fit %d\n", phd_last_error(), (int)fit[FIT_STATUS], (int)fit[FIT_NFIT]);
      bad += 1;
    }
    for (int i = 0; i < 6; ++i)
      if (!(fabs(fit[i] - p[i]) <= 1e-9)) { fprintf(stderr, "planted fit: entry %d is %g\n", i, fit[i]); bad += 1; }
    free(fit_uv); free(planted); free(fit); free(valid);
  }
  // an empty call touches no array
  mcba_camera_set c0 = {C, g_cams[0], ND, g_nd, g_fish}, c1 = {C, g_cams[1], ND, g_nd, g_fish};
  bad += phd_projection_diff(&c0, nullptr, &c1, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  for (int k = 0; k < 2; ++k) { free(g_cams[k]); free(g_poses[k]); }
  free(g_nd); free(g_fish);
  if (bad) { fprintf(stderr, "a case failed\n"); return 1; }
  printf("projdiff sanitize run: ok\n");
  return 0;
}
