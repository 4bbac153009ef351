// TEST INFRASTRUCTURE: stand-alone program around the host build of the warp mathematics, compiled by tests/test_correction_host.py
// with -fsanitize=address,undefined,float-cast-overflow and run on the CPU.  Every table is a heap block of exactly its size, so a
// control point read outside a camera's grid or a store outside an output stops the program; a non-finite coordinate that reached
// an integer conversion would stop it too.  It walks the smallest grid (1 x 1) and the largest (7 x 3, 62 control points), pixels on
// cell boundaries, on and beyond every edge, NaN and +-inf, the smallest map (1 x 1) and the refusals.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "correction_host.cpp"

static int expect_refusal(int rc, const char* text) {
  if (rc == 0 || !strstr(ch_last_error(), text)) {
    fprintf(stderr, "expected a refusal with '%s', got %d '%s'\n", text, rc, ch_last_error());
    return 1;
  }
  return 0;
}

static int run_grid(int nx, int ny) {
  const int C = 2, K = (nx + 3) * (ny + 3);
  int32_t* size = (int32_t*)malloc(C * 2 * sizeof(int32_t));
  size[0] = 200; size[1] = 150; size[2] = 7; size[3] = 5;
  double* coef = (double*)malloc((size_t)C * K * 2 * sizeof(double));
  unsigned s = 2024u;
  for (int i = 0; i < C * K * 2; ++i) {
    s = s * 1664525u + 1013904223u;
    coef[i] = ((double)(s >> 8) / 16777216.0 - 0.5) * (i < K * 2 ? 1.0 : 0.02);     // camera 1 is 7 x 5 pixels: a gentle field
  }
  mcba_field_set f = {C, size, nx, ny, coef};
  int bad = 0;
  for (int c = 0; c < C; ++c) {
    const double W = size[2 * c], H = size[2 * c + 1];
    const double xs[] = {0.0, W, -0.5, W + 0.5, -20.0, W + 20.0, W / nx, W * (nx - 1) / nx, 0.5 * W, NAN, INFINITY, -INFINITY, 1e300, -1e300};
    const double ys[] = {0.0, H, -0.5, H + 0.5, -20.0, H + 20.0, H / ny, H * (ny - 1) / ny, 0.5 * H, NAN, INFINITY, -INFINITY, 1e300, -1e300};
    const int ne = (int)(sizeof xs / sizeof xs[0]), n = ne * ne;
    double* uv = (double*)malloc((size_t)n * 2 * sizeof(double));
    double* out = (double*)malloc((size_t)n * 2 * sizeof(double));
    double* back = (double*)malloc((size_t)n * 2 * sizeof(double));
    uint8_t* status = (uint8_t*)malloc(n);
    int32_t* of = (int32_t*)malloc((size_t)n * sizeof(int32_t));
    for (int i = 0; i < n; ++i) { uv[2 * i] = xs[i / ne]; uv[2 * i + 1] = ys[i % ne]; of[i] = c; }
    bad += ch_warp_points(&f, n, of, 0, uv, out, status);
    bad += ch_warp_points(&f, n, of, 1, out, back, status);
    for (int i = 0; i < n; ++i) {
      const bool finite = isfinite(uv[2 * i]) && isfinite(uv[2 * i + 1]);
      if (finite != (status[i] == 0)) { fprintf(stderr, "status of point %d of camera %d\n", i, c); ++bad; }
      if (finite && fabs(uv[2 * i]) < 1e3 && fabs(uv[2 * i + 1]) < 1e3 &&
          !(fabs(back[2 * i] - uv[2 * i]) <= 1e-10 && fabs(back[2 * i + 1] - uv[2 * i + 1]) <= 1e-10)) {
        fprintf(stderr, "round trip of point %d of camera %d\n", i, c);
        ++bad;
      }
    }
    bad += ch_warp_points(&f, n, of, 0, uv, out, nullptr);                           // no status asked for
    free(uv); free(out); free(back); free(status); free(of);
  }
  bad += ch_warp_points(&f, 0, nullptr, 0, nullptr, nullptr, nullptr);               // n == 0
  // maps and images of the corrected cameras, the smallest ones included
  const double cam[18] = {200.0, 210.0, 100.0, 75.0, 0.0, -0.3, 0.1, 0.001, -0.002, 190.0, 190.0, 3.0, 2.0, 0.0, 0.01, 0.0, 0.0, 0.0};
  mcba_camera_set set = {C, cam, 4, nullptr, nullptr};
  const int shapes[3][2] = {{1, 1}, {7, 3}, {8, 2}};
  for (int k = 0; k < 3; ++k) {
    const int Wd = shapes[k][0], Hd = shapes[k][1], Hs = 5, Ws = 7, N = 3;
    float* maps = (float*)malloc((size_t)C * Hd * Wd * 2 * sizeof(float));
    unsigned char* src = (unsigned char*)malloc((size_t)N * Hs * Ws);
    unsigned char* dst = (unsigned char*)malloc((size_t)N * Hd * Wd);
    for (int i = 0; i < N * Hs * Ws; ++i) src[i] = (unsigned char)(i * 7);
    const int32_t of[3] = {1, 1, 0};
    bad += ch_undistort_maps_corrected(&set, &f, nullptr, nullptr, Wd, Hd, maps);
    bad += ch_undistort_images_corrected(&set, &f, nullptr, nullptr, src, N, Hs, Ws, 1, PIXEL_U8, of, Hd, Wd, 0.0, dst);
    free(maps); free(src); free(dst);
  }
  // refusals
  double one[2] = {1.0, 2.0}, o[2];
  mcba_field_set g = f;
  g.nx = 0;
  bad += expect_refusal(ch_warp_points(&g, 1, nullptr, 0, one, o, nullptr), "nx and ny must be at least 1");
  g = f; g.nx = 6; g.ny = 4;
  bad += expect_refusal(ch_warp_points(&g, 1, nullptr, 0, one, o, nullptr), "control points");
  const int32_t two[1] = {2};
  bad += expect_refusal(ch_warp_points(&f, 1, two, 0, one, o, nullptr), "names camera");
  coef[3] = 1e6;
  bad += expect_refusal(ch_warp_points(&f, 1, nullptr, 0, one, o, nullptr), "the field folds the image");
  coef[3] = NAN;
  bad += expect_refusal(ch_warp_points(&f, 1, nullptr, 0, one, o, nullptr), "not finite");
  free(size); free(coef);
  return bad;
}

int main() {
  int bad = run_grid(1, 1);
  bad += run_grid(7, 3);
  bad += run_grid(5, 4);
  if (bad) { fprintf(stderr, "a call failed\n"); return 1; }
  printf("correction sanitize run: ok\n");
  return 0;
}
