// TEST INFRASTRUCTURE: stand-alone program around the host build of the rig localisation mathematics, compiled by
// tests/test_localize_host.py with -fsanitize=address,undefined and run on the CPU.  Every table and every output is a heap block of
// exactly its size, so a record read or an error stored outside it stops the program.  Three cameras (5 and 4 Brown-Conrady
// coefficients, one Kannala-Brandt) see two boards from four rig poses, static and with rolling shutter, with and without start
// poses; pixels that are not finite are planted, one frame has no observation and one has two, a padded board row is masked, and
// the optional outputs are left out in turn.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "localize_host.cpp"

static const int C = 3, F = 4, B = 2, P = 30, REAL = 25;     // a 5 x 5 board in rows padded to 30

static void pinhole(const double* cam, const double* X, double* uv) {      // (observations near the model's: the run checks memory)
  uv[0] = cam[0] * X[0] / X[2] + cam[2];
  uv[1] = cam[1] * X[1] / X[2] + cam[3];
}

static void identity(double* T) {
  for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
}

static int run(bool rolling, bool with_init, bool with_optional, int max_iterations) {
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
  double* camera_poses = (double*)malloc((size_t)C * 16 * sizeof(double));
  double* board_poses = (double*)malloc((size_t)B * 16 * sizeof(double));
  double* init = (double*)malloc((size_t)F * 16 * sizeof(double));
  double* heights = (double*)malloc(C * sizeof(double));
  for (int c = 0; c < C; ++c) {
    identity(camera_poses + 16 * c);
    camera_poses[16 * c + 3] = -0.1 * (c - 1);
    heights[c] = 300.0;
  }
  for (int b = 0; b < B; ++b) {
    identity(board_poses + 16 * b);
    board_poses[16 * b + 3] = 0.3 * b - 0.25;
    board_poses[16 * b + 7] = 0.35 * b - 0.3;      // (the two boards cover image rows 30 .. 95 and 170 .. 235 of 300)
  }
  for (int f = 0; f < F; ++f) {
    identity(init + 16 * f);
    init[16 * f + 3] = 0.01 * f;
    init[16 * f + 11] = 1.0 + 0.05 * f;
  }
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
  unsigned s = 1357u;
  for (int c = 0; c < C; ++c)
    for (int f = 0; f < F; ++f)
      for (int b = 0; b < B; ++b)
        for (int j = 0; j < P; ++j) {
          const size_t slot = (((size_t)c * F + f) * B + b) * P + j;
          const double* X = board_points + ((size_t)b * P + j) * 3;
          const double Xc[3] = {X[0] + board_poses[16 * b + 3] + init[16 * f + 3] + camera_poses[16 * c + 3], X[1] + board_poses[16 * b + 7],
                                X[2] + init[16 * f + 11]};
          pinhole(cams + c * stride, Xc, points + 2 * slot);
          s = s * 1664525u + 1013904223u;
          valid[slot] = (s >> 28) != 0;                 // one in sixteen is not seen -- and the padded slots claim to be
        }
  // frame 2 has no observation, frame 3 has two; planted pixels that are not finite
  for (int c = 0; c < C; ++c)
    for (int b = 0; b < B; ++b)
      for (int j = 0; j < P; ++j) {
        valid[(((size_t)c * F + 2) * B + b) * P + j] = 0;
        valid[(((size_t)c * F + 3) * B + b) * P + j] = (c == 1 && b == 0 && j < 2) ? 1 : 0;
      }
  points[2 * ((((size_t)0 * F + 0) * B + 0) * P + 3)] = NAN;
  points[2 * ((((size_t)1 * F + 1) * B + 1) * P + 4) + 1] = INFINITY;
  double* poses = (double*)malloc((size_t)F * 16 * sizeof(double));
  uint8_t* status = (uint8_t*)malloc((size_t)F);
  const int KC = rolling ? 78 : 21;
  double* poses_end = with_optional ? (double*)malloc((size_t)F * 16 * sizeof(double)) : nullptr;
  double* cov = with_optional ? (double*)malloc((size_t)F * KC * sizeof(double)) : nullptr;
  double* sse = with_optional ? (double*)malloc((size_t)F * sizeof(double)) : nullptr;
  int32_t* n_obs = with_optional ? (int32_t*)malloc((size_t)F * sizeof(int32_t)) : nullptr;
  int32_t* iters = with_optional ? (int32_t*)malloc((size_t)F * sizeof(int32_t)) : nullptr;
  double* err = with_optional ? (double*)malloc((size_t)C * F * B * P * sizeof(double)) : nullptr;
  mcba_rig_pose_problem p = {};
  p.cams.C = C; p.cams.cameras = cams; p.cams.n_dist = nd; p.cams.camera_n_dist = cam_nd; p.cams.is_fisheye = fish;
  p.F = F; p.B = B; p.P = P;
  p.camera_poses = camera_poses; p.board_poses = board_poses; p.board_points = board_points; p.board_valid = board_valid;
  p.points = points; p.valid = valid;
  p.init = with_init ? init : nullptr;
  p.rolling = rolling ? 1 : 0;
  p.image_heights = rolling ? heights : nullptr;
  p.sigma_px = with_optional ? 0.0 : 0.05;
  p.max_iterations = max_iterations;
  int rc = lh_rig_poses(&p, poses, poses_end, cov, sse, n_obs, iters, err, status);
  if (rc != 0) fprintf(stderr, "lh_rig_poses: %s\n", lh_last_error());
  // (the pinhole observations are several pixels off the distorted and fisheye models: a large-residual problem that converges
  //  linearly -- within the cap of 100, not within the default 20 under rolling shutter)
  const bool full = max_iterations == 100;
  for (int f = 0; f < 2 && rc == 0; ++f)
    if (status[f] != MCBA_RIG_OK && status[f] != MCBA_RIG_NOT_CONVERGED) { fprintf(stderr, "frame %d has status %d\n", f, status[f]); rc = 1; }
  if (rc == 0 && full && (status[0] != MCBA_RIG_OK || status[1] != MCBA_RIG_OK)) {
    fprintf(stderr, "frames 0 and 1 have status %d and %d\n", status[0], status[1]);
    rc = 1;
  }
  if (rc == 0 && (status[2] != MCBA_RIG_TOO_FEW || status[3] != MCBA_RIG_TOO_FEW)) {
    fprintf(stderr, "the frames without observations have status %d and %d\n", status[2], status[3]);
    rc = 1;
  }
  free(cams); free(cam_nd); free(fish); free(camera_poses); free(board_poses); free(init); free(heights); free(board_points);
  free(board_valid); free(points); free(valid); free(poses); free(status); free(poses_end); free(cov); free(sse); free(n_obs);
  free(iters); free(err);
  return rc;
}

int main() {
  int bad = 0;
  for (int rolling = 0; rolling <= 1; ++rolling)
    for (int with_init = 0; with_init <= 1; ++with_init) {
      bad += run(rolling != 0, with_init != 0, true, 0);
      bad += run(rolling != 0, with_init != 0, false, 100);
      bad += run(rolling != 0, with_init != 0, true, 1);
    }
  // an empty table touches no array
  mcba_rig_pose_problem p = {};
  const double cam[9] = {200.0, 210.0, 3.0, 2.0, 0.0, -0.3, 0.1, 0.001, -0.002};
  p.cams.C = 1; p.cams.cameras = cam; p.cams.n_dist = 4;
  p.F = 0; p.B = 2; p.P = 5;
  bad += lh_rig_poses(&p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (bad) { fprintf(stderr, "a call failed\n"); return 1; }
  printf("localize sanitize run: ok\n");
  return 0;
}
