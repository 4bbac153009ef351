// TEST INFRASTRUCTURE: stand-alone program around the host build of the undistortion mathematics, compiled by
// tests/test_undistort_host.py with -fsanitize=address,undefined and run on the CPU.  Every source image and every output is a heap
// block of exactly its size, so a tap read or a store outside it stops the program.  The maps hold the edge coordinates of the
// remap (W - 1, -0.5, -2, W + 1, NaN, +-inf, +-1e30, ...) on both axes, next to coordinates spread over and around the source.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "undistort_host.cpp"

static int run_format(int channels, int dtype, int Hs, int Ws, int Hd, int Wd) {
  const int N = 2, M = 2;
  const size_t px = pixel_bytes(dtype) * channels;
  unsigned char* src = (unsigned char*)malloc((size_t)N * Hs * Ws * px);
  unsigned char* dst = (unsigned char*)malloc((size_t)N * Hd * Wd * px);
  float* maps = (float*)malloc((size_t)M * Hd * Wd * 2 * sizeof(float));
  for (size_t i = 0; i < (size_t)N * Hs * Ws * channels; ++i) {
    if (dtype == PIXEL_U8) src[i] = (unsigned char)(i * 37 + 11);
    else ((float*)src)[i] = (float)((i * 37 + 11) % 256);
  }
  const float inf = INFINITY;
  const float ex[] = {(float)Ws - 1.0f, -0.5f, -0.25f, -2.0f, (float)Ws + 1.0f, NAN, inf, -inf, 1e30f, -1e30f, 0.0f, (float)Ws - 0.5f,
                      -1.0f, (float)Ws, -2.5f, (float)Ws + 0.999f, 3.0e9f, -3.0e9f};
  const float ey[] = {(float)Hs - 1.0f, -0.5f, -0.25f, -2.0f, (float)Hs + 1.0f, NAN, inf, -inf, 1e30f, -1e30f, 0.0f, (float)Hs - 0.5f,
                      -1.0f, (float)Hs, -2.5f, (float)Hs + 0.999f, 3.0e9f, -3.0e9f};
  const int ne = (int)(sizeof ex / sizeof ex[0]);
  size_t k = 0;
  unsigned s = 12345u;
  for (size_t i = 0; i < (size_t)M * Hd * Wd; ++i) {
    float x, y;
    if (k < (size_t)ne * ne) { x = ex[k / ne]; y = ey[k % ne]; ++k; }           // every pair of edge coordinates
    else {
      s = s * 1664525u + 1013904223u; x = -4.0f + (float)(s >> 8) / 16777216.0f * (float)(Ws + 7);
      s = s * 1664525u + 1013904223u; y = -4.0f + (float)(s >> 8) / 16777216.0f * (float)(Hs + 7);
    }
    maps[2 * i] = x;
    maps[2 * i + 1] = y;
  }
  const int32_t of[2] = {1, 0};
  const int rc = uh_remap(src, N, Hs, Ws, channels, dtype, maps, M, Hd, Wd, of, 7.0, dst);
  if (rc != 0) fprintf(stderr, "uh_remap: %s\n", uh_last_error());
  free(src); free(dst); free(maps);
  return rc;
}

int main() {
  int bad = 0;
  for (int channels = 1; channels <= 3; channels += 2)
    for (int dtype = 0; dtype <= 1; ++dtype) {
      bad += run_format(channels, dtype, 5, 7, 23, 19);      // 18 x 18 edge pairs fit the 2 x 23 x 19 map entries
      bad += run_format(channels, dtype, 1, 1, 20, 20);      // a source of one pixel: every tap but one is border
    }
  // the fused form and the point calls on a camera whose zoomed-out image looks past the source
  const double cam[9] = {200.0, 210.0, 3.0, 2.0, 0.0, -0.3, 0.1, 0.001, -0.002};
  mcba_camera_set set = {1, cam, 4, nullptr, nullptr};
  const double P[9] = {20.0, 0.0, 3.0, 0.0, 21.0, 2.0, 0.0, 0.0, 1.0};
  const int Hs = 5, Ws = 7, Hd = 6, Wd = 9;
  unsigned char* src = (unsigned char*)malloc((size_t)Hs * Ws);
  unsigned char* dst = (unsigned char*)malloc((size_t)Hd * Wd);
  float* maps = (float*)malloc((size_t)Hd * Wd * 2 * sizeof(float));
  for (int i = 0; i < Hs * Ws; ++i) src[i] = (unsigned char)(i * 7);
  const int32_t of0[1] = {0};
  bad += uh_undistort_images(&set, nullptr, P, src, 1, Hs, Ws, 1, PIXEL_U8, of0, Hd, Wd, 0.0, dst);
  bad += uh_undistort_maps(&set, nullptr, P, Wd, Hd, maps);
  double* uv = (double*)malloc(4 * 2 * sizeof(double));
  double* out = (double*)malloc(4 * 2 * sizeof(double));
  uint8_t* status = (uint8_t*)malloc(4);
  const double px[8] = {0.0, 0.0, 6.0, 4.0, 1e6, -1e6, NAN, 1.0};
  for (int i = 0; i < 8; ++i) uv[i] = px[i];
  bad += uh_undistort_points(&set, 4, nullptr, uv, nullptr, P, out, status);
  free(src); free(dst); free(maps); free(uv); free(out); free(status);
  if (bad) { fprintf(stderr, "a call failed\n"); return 1; }
  printf("undistort sanitize run: ok\n");
  return 0;
}
