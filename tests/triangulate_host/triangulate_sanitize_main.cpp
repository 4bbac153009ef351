// TEST INFRASTRUCTURE: stand-alone program around the host build of the triangulation mathematics, compiled by
// tests/test_triangulate_host.py with -fsanitize=address,undefined and run on the CPU.  Every table and every output is a heap block
// of exactly its size, so an observation read or an error stored outside it stops the program.  Three cameras (5 and 4 Brown-Conrady
// coefficients, one Kannala-Brandt) see a cloud of points from three places, static and with rolling shutter; pixels that are not
// finite, that no fisheye camera can have produced and that lie far outside the image are planted, views are masked, and the
// optional outputs are left out in turn.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "triangulate_host.cpp"

static const int C = 3, F = 2, M = 67;

static void pinhole(const double* cam, const double* X, double* uv) {      // (observations near the model's: the sanitizer run checks memory)
  uv[0] = cam[0] * X[0] / X[2] + cam[2];
  uv[1] = cam[1] * X[1] / X[2] + cam[3];
}

static int run(bool rolling, bool with_optional, int max_iterations) {
  const int nd = 5, stride = 5 + nd;
  double* cams = (double*)calloc((size_t)C * stride, sizeof(double));
  const double blocks[3][10] = {{200.0, 205.0, 100.0, 75.0, 0.0, -0.12, 0.3, 1e-3, -1e-3, -0.2},
                                {210.0, 200.0, 98.0, 77.0, 0.0, -0.1, 0.2, 1e-3, 1e-3, 0.0},
                                {190.0, 195.0, 101.0, 74.0, 0.0, 0.05, 0.01, -0.005, 0.001, 0.0}};
  for (int c = 0; c < C; ++c)
    for (int i = 0; i < stride; ++i) cams[c * stride + i] = blocks[c][i];
  int32_t* cam_nd = (int32_t*)malloc(C * sizeof(int32_t));
  uint8_t* fish = (uint8_t*)malloc(C);
  cam_nd[0] = 5; cam_nd[1] = 4; cam_nd[2] = 4;
  fish[0] = 0; fish[1] = 0; fish[2] = 1;
  double* views = (double*)calloc((size_t)C * F * 12, sizeof(double));
  double* views_end = (double*)calloc((size_t)C * F * 12, sizeof(double));
  double* heights = (double*)malloc(C * sizeof(double));
  uint8_t* view_valid = (uint8_t*)malloc((size_t)C * F);
  for (int c = 0; c < C; ++c) {
    heights[c] = 150.0;
    for (int f = 0; f < F; ++f) {
      double* v = views + ((size_t)c * F + f) * 12;
      v[0] = v[5] = v[10] = 1.0;                       // identity rotation, the camera 0.15 m further along x per index
      v[3] = -0.15 * (c - 1) + 0.01 * f;
      double* e = views_end + ((size_t)c * F + f) * 12;
      for (int i = 0; i < 12; ++i) e[i] = v[i];
      e[3] += 0.004;
      e[7] -= 0.003;
      view_valid[c * F + f] = (c == 1 && f == 1) ? 0 : 1;
    }
  }
  double* points = (double*)malloc((size_t)C * F * M * 2 * sizeof(double));
  uint8_t* valid = (uint8_t*)malloc((size_t)C * F * M);
  unsigned s = 2468u;
  for (int f = 0; f < F; ++f)
    for (int m = 0; m < M; ++m) {
      double X[3];
      for (int k = 0; k < 3; ++k) { s = s * 1664525u + 1013904223u; X[k] = (double)(s >> 8) / 16777216.0; }
      X[0] = -0.25 + 0.5 * X[0]; X[1] = -0.2 + 0.4 * X[1]; X[2] = 0.8 + 1.2 * X[2];
      for (int c = 0; c < C; ++c) {
        const size_t slot = ((size_t)c * F + f) * M + m;
        const double* v = views + ((size_t)c * F + f) * 12;
        const double Xc[3] = {X[0] + v[3], X[1] + v[7], X[2] + v[11]};
        pinhole(cams + c * stride, Xc, points + 2 * slot);
        s = s * 1664525u + 1013904223u;
        valid[slot] = (s >> 28) != 0;                 // one in sixteen is not seen
      }
    }
  // planted pixels: not finite, outside the fisheye model, far outside the image, a point nobody sees
  points[2 * (((size_t)0 * F + 0) * M + 3)] = NAN;
  points[2 * (((size_t)1 * F + 0) * M + 4) + 1] = INFINITY;
  points[2 * (((size_t)2 * F + 0) * M + 5)] = 5000.0;
  points[2 * (((size_t)2 * F + 0) * M + 5) + 1] = 4000.0;
  points[2 * (((size_t)0 * F + 1) * M + 6)] = -1e9;
  points[2 * (((size_t)1 * F + 0) * M + 7)] = 1e300;
  for (int c = 0; c < C; ++c) valid[((size_t)c * F + 1) * M + (M - 1)] = 0;
  double* X = (double*)malloc((size_t)F * M * 3 * sizeof(double));
  uint8_t* status = (uint8_t*)malloc((size_t)F * M);
  double* cov = with_optional ? (double*)malloc((size_t)F * M * 6 * sizeof(double)) : nullptr;
  double* sse = with_optional ? (double*)malloc((size_t)F * M * sizeof(double)) : nullptr;
  double* err = with_optional ? (double*)malloc((size_t)C * F * M * sizeof(double)) : nullptr;
  int32_t* n_views = with_optional ? (int32_t*)malloc((size_t)F * M * sizeof(int32_t)) : nullptr;
  mcba_triangulate_problem p = {};
  p.cams.C = C; p.cams.cameras = cams; p.cams.n_dist = nd; p.cams.camera_n_dist = cam_nd; p.cams.is_fisheye = fish;
  p.F = F; p.M = M;
  p.views = views;
  p.views_end = rolling ? views_end : nullptr;
  p.image_heights = rolling ? heights : nullptr;
  p.view_valid = view_valid;
  p.points = points; p.valid = valid;
  p.sigma_px = with_optional ? 0.0 : 0.05;
  p.max_iterations = max_iterations;
  int rc = th_triangulate(&p, X, cov, sse, err, n_views, status);
  if (rc != 0) fprintf(stderr, "th_triangulate: %s\n", th_last_error());
  int ok = 0;
  for (int i = 0; i < F * M; ++i) ok += status[i] == MCBA_TRI_OK;
  if (rc == 0 && max_iterations != 1 && ok < F * M / 2) { fprintf(stderr, "only %d of %d points converged\n", ok, F * M); rc = 1; }
  if (rc == 0 && status[1 * M + (M - 1)] != MCBA_TRI_TOO_FEW) { fprintf(stderr, "the unseen point has status %d\n", status[1 * M + (M - 1)]); rc = 1; }
  free(cams); free(cam_nd); free(fish); free(views); free(views_end); free(heights); free(view_valid); free(points); free(valid);
  free(X); free(status); free(cov); free(sse); free(err); free(n_views);
  return rc;
}

int main() {
  int bad = 0;
  for (int rolling = 0; rolling <= 1; ++rolling) {
    bad += run(rolling != 0, true, 0);
    bad += run(rolling != 0, false, 100);
    bad += run(rolling != 0, true, 1);
  }
  // an empty table touches no array
  mcba_triangulate_problem p = {};
  const double cam[9] = {200.0, 210.0, 3.0, 2.0, 0.0, -0.3, 0.1, 0.001, -0.002};
  p.cams.C = 1; p.cams.cameras = cam; p.cams.n_dist = 4;
  p.F = 0; p.M = 5;
  bad += th_triangulate(&p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (bad) { fprintf(stderr, "a call failed\n"); return 1; }
  printf("triangulate sanitize run: ok\n");
  return 0;
}
