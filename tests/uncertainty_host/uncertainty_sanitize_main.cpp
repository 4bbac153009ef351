// TEST INFRASTRUCTURE: stand-alone program around the host build of the projection-uncertainty mathematics, compiled by
// tests/test_projection_uncertainty_host.py with -fsanitize=address,undefined and run on the CPU.  Every input and every output is a
// heap block of exactly its size, so a read or a store outside it stops the program.  Three cameras (5 and 4 Brown-Conrady
// coefficients, one Kannala-Brandt) serve the edge cases: the rig frame and a reference camera, a grid and a list, the same camera
// twice, a held-everything job (r = 0), pixels that are not finite or outside the model, a point behind the camera, an
// unconstrained column, the optional output left out, an empty call and calls that are refused.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uncertainty_host.cpp"

static const int C = 3, ND = 5, STRIDE = 5 + ND;
static double* g_cams;
static int32_t* g_nd;
static uint8_t* g_fish;
static double* g_poses;

static int own_k(int c) { return c < C ? 4 + (g_fish[c] ? 4 : g_nd[c]) : 8; }   // (a camera that does not exist: the call is refused)

// one job with a W of r columns of exactly K * r doubles
static int run(int b, int a, double rho, int r, bool grid, bool with_std, int flagged, const double* list, int n_list, int want_rc,
               int want_status0) {
  const int K = own_k(b) + 6 + (a >= 0 ? 6 + own_k(a) : 0);
  double* W = r > 0 ? (double*)malloc((size_t)K * r * sizeof(double)) : nullptr;
  unsigned s = 1234u + 17u * b + r;
  for (int i = 0; i < K * r; ++i) { s = s * 1664525u + 1013904223u; W[i] = 1e-3 * ((double)(s >> 8) / 16777216.0 - 0.5); }
  uint8_t* flags = (uint8_t*)calloc(K, 1);
  if (flagged >= 0) {
    flags[flagged] = 1;
    for (int c = 0; c < r; ++c) W[flagged * r + c] = 0.0;
  }
  mcba_uncertainty_job job = {};
  job.camera = b; job.reference = a; job.inv_distance = rho; job.K = K; job.r = r; job.W = W; job.unconstrained = flags;
  int64_t n = n_list;
  double* uv = nullptr;
  if (grid) {
    job.grid_w = 9; job.grid_h = 7; job.u0 = 5.0; job.v0 = 4.0; job.du = 23.0; job.dv = 21.0;
    n = 63;
  } else {
    uv = (double*)malloc((size_t)(n_list > 0 ? n_list : 1) * 2 * sizeof(double));
    memcpy(uv, list, (size_t)n_list * 2 * sizeof(double));
    job.n = n_list; job.uv = uv;
  }
  double* cov = (double*)malloc((size_t)(n > 0 ? n : 1) * 3 * sizeof(double));
  double* std = with_std ? (double*)malloc((size_t)(n > 0 ? n : 1) * sizeof(double)) : nullptr;
  uint8_t* status = (uint8_t*)malloc((size_t)(n > 0 ? n : 1));
  mcba_camera_set cams = {C, g_cams, ND, g_nd, g_fish};
  int rc = unh_projection_uncertainty(&cams, g_poses, 1, &job, cov, std, status);
  int bad = 0;
  if ((rc != 0) != (want_rc != 0)) { fprintf(stderr, "rc %d, expected %d: %s\n", rc, want_rc, unh_last_error()); bad = 1; }
  if (rc == 0 && n > 0 && want_status0 >= 0 && status[0] != want_status0) {
    fprintf(stderr, "job (%d, %d, rho %g): status %d, expected %d\n", b, a, rho, status[0], want_status0);
    bad = 1;
  }
  if (rc == 0 && n > 0 && want_status0 == MCBA_UNC_OK) {
    if (!(cov[0] >= 0.0) || !(cov[2] >= 0.0)) { fprintf(stderr, "a variance is negative or NaN\n"); bad = 1; }
    if ((r == 0 || a == b) && (cov[0] != 0.0 || cov[1] != 0.0 || cov[2] != 0.0)) { fprintf(stderr, "not exactly 0\n"); bad = 1; }
  }
  if (rc == 0 && n > 0 && want_status0 > 0 && cov[0] == cov[0]) { fprintf(stderr, "no NaN with status %d\n", want_status0); bad = 1; }
  free(W); free(flags); free(uv); free(cov); free(std); free(status);
  return bad;
}

int main() {
  g_cams = (double*)calloc((size_t)C * STRIDE, sizeof(double));
  const double blocks[3][10] = {{200.0, 205.0, 100.0, 75.0, 0.0, -0.12, 0.3, 1e-3, -1e-3, -0.2},
                                {210.0, 200.0, 98.0, 77.0, 0.0, -0.1, 0.2, 1e-3, 1e-3, 0.0},
                                {190.0, 195.0, 101.0, 74.0, 0.0, 0.05, 0.01, -0.005, 0.001, 0.0}};
  for (int c = 0; c < C; ++c)
    for (int i = 0; i < STRIDE; ++i) g_cams[c * STRIDE + i] = blocks[c][i];
  g_nd = (int32_t*)malloc(C * sizeof(int32_t));
  g_fish = (uint8_t*)malloc(C);
  g_nd[0] = 5; g_nd[1] = 4; g_nd[2] = 4;
  g_fish[0] = 0; g_fish[1] = 0; g_fish[2] = 1;
  g_poses = (double*)calloc((size_t)C * 16, sizeof(double));
  for (int c = 0; c < C; ++c) {
    double* T = g_poses + 16 * c;
    T[0] = T[5] = T[10] = T[15] = 1.0;
    T[3] = -0.1 * (c - 1);
  }
  // camera 2 of the last case looks the other way (a half turn about y)
  const double centre[2] = {100.0, 75.0};
  const double pixels[10] = {100.0, 75.0, 0.0, 0.0, 199.0, 149.0, NAN, 10.0, 1e9, -1e9};
  const double outside[2] = {5000.0, 4000.0};
  int bad = 0;
  for (int with_std = 0; with_std <= 1; ++with_std) {
    bad += run(0, -1, 0.5, 11, true, with_std != 0, -1, nullptr, 0, 0, MCBA_UNC_OK);
    bad += run(1, 0, 0.5, 30, true, with_std != 0, -1, nullptr, 0, 0, MCBA_UNC_OK);
    bad += run(2, 1, 0.0, 48, false, with_std != 0, -1, pixels, 5, 0, MCBA_UNC_OK);
    bad += run(0, 2, 2.0, 7, false, with_std != 0, -1, pixels, 5, 0, MCBA_UNC_OK);
  }
  bad += run(1, 1, 2.0, 12, false, true, -1, pixels, 5, 0, MCBA_UNC_OK);                 // the same camera: exactly 0
  bad += run(1, -1, 2.0, 0, false, true, -1, pixels, 5, 0, MCBA_UNC_OK);                 // held everything
  bad += run(1, 2, 2.0, 0, true, true, -1, nullptr, 0, 0, MCBA_UNC_OK);
  bad += run(2, -1, 1.0, 5, false, true, -1, outside, 1, 0, MCBA_UNC_NOT_CONVERGED);     // no fisheye camera produced this pixel
  bad += run(0, 2, 1.0, 5, false, true, -1, outside, 1, 0, MCBA_UNC_NOT_CONVERGED);
  bad += run(0, -1, 1.0, 5, false, true, 2, centre, 1, 0, MCBA_UNC_UNCONSTRAINED);       // cx is unconstrained
  bad += run(0, -1, 0.0, 5, false, true, 9 + 5, centre, 1, 0, MCBA_UNC_OK);              // a translation at infinity: J = 0
  bad += run(0, -1, 1.0, 5, false, true, -1, centre, 0, 0, -1);                          // no query
  bad += run(0, -1, -1.0, 5, false, true, -1, centre, 1, 1, -1);                         // refused: rho < 0
  bad += run(0, -1, NAN, 5, false, true, -1, centre, 1, 1, -1);
  bad += run(0, 3, 1.0, 5, false, true, -1, centre, 1, 1, -1);                           // refused: reference out of range
  double* T = g_poses + 16 * 2;                                                          // behind: camera 2 turned round
  T[0] = -1.0; T[10] = -1.0;
  bad += run(2, 0, 1.0, 5, false, true, -1, centre, 1, 0, MCBA_UNC_BEHIND);
  // an empty call touches no array
  mcba_camera_set cams = {C, g_cams, ND, g_nd, g_fish};
  bad += unh_projection_uncertainty(&cams, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
  free(g_cams); free(g_nd); free(g_fish); free(g_poses);
  if (bad) { fprintf(stderr, "a case failed\n"); return 1; }
  printf("uncertainty sanitize run: ok\n");
  return 0;
}
