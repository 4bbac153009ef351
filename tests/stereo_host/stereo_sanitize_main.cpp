// TEST INFRASTRUCTURE: stand-alone program around the host build of the stereo calibration mathematics, compiled by
// tests/test_stereo_host.py with -fsanitize=address,undefined and run on the CPU.  Every table and every output is a heap block of
// exactly its size, so a corner read or a view block stored outside it stops the program.  Three cameras (5 and 4 Brown-Conrady
// coefficients, one Kannala-Brandt) see two boards in three frames; pixels that are not finite are planted, one slot keeps a single
// board row in one camera (collinear: dropped), one start pose is marked invalid, one camera sees nothing in a frame, a padded
// board row is masked, both summation orders run, and the optional outputs are left out in turn.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "stereo_host.cpp"

static const int C = 3, F = 3, B = 2, P = 30, REAL = 25;     // a 5 x 5 board in rows padded to 30
static const int NP = 4;

static void pinhole(const double* cam, const double* X, double* uv) {      // (observations near the model's: the run checks memory)
  uv[0] = cam[0] * X[0] / X[2] + cam[2];
  uv[1] = cam[1] * X[1] / X[2] + cam[3];
}

static int run(bool with_optional, bool with_board_valid, int max_iterations, int min_common) {
  const int nd = 5, stride = 5 + nd;
  double* cams = (double*)calloc((size_t)C * stride, sizeof(double));
  const double blocks[3][10] = {{400.0, 405.0, 200.0, 150.0, 0.0, -0.02, 0.01, 1e-3, -1e-3, -0.002},
                                {410.0, 400.0, 198.0, 152.0, 0.0, -0.01, 0.02, 1e-3, 1e-3, 0.0},
                                {390.0, 395.0, 201.0, 149.0, 0.0, 0.005, 0.001, -0.0005, 0.0001, 0.0}};
  for (int c = 0; c < C; ++c)
    for (int i = 0; i < stride; ++i) cams[c * stride + i] = blocks[c][i];
  int32_t* cam_nd = (int32_t*)malloc(C * sizeof(int32_t));
  uint8_t* fish = (uint8_t*)malloc(C);
  cam_nd[0] = 5; cam_nd[1] = 4; cam_nd[2] = 4;
  fish[0] = 0; fish[1] = 0; fish[2] = 1;
  double* board_points = (double*)calloc((size_t)B * P * 3, sizeof(double));
  uint8_t* board_valid = (uint8_t*)calloc((size_t)B * P, 1);
  for (int b = 0; b < B; ++b)
    for (int j = 0; j < REAL; ++j) {
      board_points[((size_t)b * P + j) * 3] = 0.04 * (j % 5);
      board_points[((size_t)b * P + j) * 3 + 1] = 0.04 * (j / 5);
      board_valid[(size_t)b * P + j] = 1;
    }
  double* points = (double*)calloc((size_t)C * F * B * P * 2, sizeof(double));
  uint8_t* valid = (uint8_t*)calloc((size_t)C * F * B * P, 1);
  double* view_poses = (double*)calloc((size_t)C * F * B * 16, sizeof(double));
  uint8_t* view_valid = (uint8_t*)malloc((size_t)C * F * B);
  unsigned s = 2468u;
  for (int c = 0; c < C; ++c)
    for (int f = 0; f < F; ++f)
      for (int b = 0; b < B; ++b) {
        const size_t view = ((size_t)c * F + f) * B + b;
        double* T = view_poses + 16 * view;
        for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
        T[3] = 0.3 * b - 0.25 + 0.01 * f - 0.1 * (c - 1);
        T[7] = 0.35 * b - 0.3;
        T[11] = 1.0 + 0.05 * f;
        view_valid[view] = 1;
        for (int j = 0; j < P; ++j) {
          const size_t slot = view * P + j;
          const double* X = board_points + ((size_t)b * P + j) * 3;
          const double Xc[3] = {X[0] + T[3], X[1] + T[7], X[2] + T[11]};
          pinhole(cams + c * stride, Xc, points + 2 * slot);
          s = s * 1664525u + 1013904223u;
          valid[slot] = (s >> 28) != 0 && (with_board_valid || j < REAL);   // one in sixteen is not seen; the padded slots claim to be
        }
      }
  // camera 2 sees nothing in frame 2; camera 1 keeps one board row of slot (0, 1); the start pose of camera 0 in slot (1, 0) is invalid
  for (int b = 0; b < B; ++b)
    for (int j = 0; j < P; ++j) valid[(((size_t)2 * F + 2) * B + b) * P + j] = 0;
  for (int j = 0; j < P; ++j) valid[(((size_t)1 * F + 0) * B + 1) * P + j] = j < 5;
  view_valid[((size_t)0 * F + 1) * B + 0] = 0;
  points[2 * ((((size_t)0 * F + 0) * B + 0) * P + 3)] = NAN;
  points[2 * ((((size_t)1 * F + 1) * B + 1) * P + 4) + 1] = INFINITY;
  int32_t* pairs = (int32_t*)malloc((size_t)NP * 2 * sizeof(int32_t));
  const int32_t list[NP][2] = {{0, 1}, {1, 2}, {0, 2}, {2, 0}};
  for (int k = 0; k < NP; ++k) { pairs[2 * k] = list[k][0]; pairs[2 * k + 1] = list[k][1]; }
  double* T = (double*)malloc((size_t)NP * 16 * sizeof(double));
  uint8_t* status = (uint8_t*)malloc((size_t)NP);
  double* cov = with_optional ? (double*)malloc((size_t)NP * 36 * sizeof(double)) : nullptr;
  double* sse = with_optional ? (double*)malloc((size_t)NP * sizeof(double)) : nullptr;
  int32_t* n_views = with_optional ? (int32_t*)malloc((size_t)NP * sizeof(int32_t)) : nullptr;
  int32_t* n_points = with_optional ? (int32_t*)malloc((size_t)NP * sizeof(int32_t)) : nullptr;
  int32_t* iters = with_optional ? (int32_t*)malloc((size_t)NP * sizeof(int32_t)) : nullptr;
  double* vposes = with_optional ? (double*)malloc((size_t)NP * F * B * 16 * sizeof(double)) : nullptr;
  double* vsse = with_optional ? (double*)malloc((size_t)NP * F * B * 2 * sizeof(double)) : nullptr;
  mcba_stereo_problem p = {};
  p.cams.C = C; p.cams.cameras = cams; p.cams.n_dist = nd; p.cams.camera_n_dist = cam_nd; p.cams.is_fisheye = fish;
  p.F = F; p.B = B; p.P = P;
  p.board_points = board_points; p.board_valid = with_board_valid ? board_valid : nullptr;
  p.points = points; p.valid = valid; p.view_poses = view_poses; p.view_valid = view_valid;
  p.n_pairs = NP; p.pairs = pairs; p.min_common = min_common; p.max_iterations = max_iterations;
  p.sigma_px = with_optional ? 0.0 : 0.05;
  int rc = 0;
  for (int order = 0; order < 2 && rc == 0; ++order) {
    sh_set_device_order(order);
    rc = sh_stereo_calibrate(&p, T, cov, sse, n_views, n_points, iters, vposes, vsse, status);
    if (rc != 0) fprintf(stderr, "sh_stereo_calibrate: %s\n", sh_last_error());
    for (int k = 0; k < NP && rc == 0; ++k)
      if (status[k] != MCBA_STEREO_OK && status[k] != MCBA_STEREO_NOT_CONVERGED) { fprintf(stderr, "pair %d has status %d\n", k, status[k]); rc = 1; }
    // pair (0, 1): 6 slots less the invalid start pose and the collinear one
    if (rc == 0 && n_views && n_views[0] != 4) { fprintf(stderr, "pair 0 has %d views\n", n_views[0]); rc = 1; }
    if (rc == 0 && n_views && n_views[1] != 3) { fprintf(stderr, "pair 1 has %d views\n", n_views[1]); rc = 1; }
  }
  sh_set_device_order(0);
  free(cams); free(cam_nd); free(fish); free(board_points); free(board_valid); free(points); free(valid); free(view_poses);
  free(view_valid); free(pairs); free(T); free(status); free(cov); free(sse); free(n_views); free(n_points); free(iters); free(vposes);
  free(vsse);
  return rc;
}

int main() {
  int bad = 0;
  bad += run(true, true, 0, 0);
  bad += run(false, true, 1000, 4);
  bad += run(true, false, 1, 3);
  // no pair: no array is touched
  mcba_stereo_problem p = {};
  bad += sh_stereo_calibrate(&p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (bad) { fprintf(stderr, "a call failed\n"); return 1; }
  printf("stereo sanitize run: ok\n");
  return 0;
}
