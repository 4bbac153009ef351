// TEST INFRASTRUCTURE: stand-alone program around the host build of the corner refinement (mcba_subpix.h) and its argument checks,
// compiled by tests/test_subpix_host.py with -fsanitize=address,undefined and run on the CPU.  Every image and every output is a heap
// block of exactly its size, so a sample or a store outside it stops the program.  Two textured images of 23 x 31 pixels in both pixel
// types serve starts on and within the window of every border and image corner for half windows 1, 5, 15, (15, 1) and (2, 15) -- most
// windows hang over the image on several sides --, starts that are not finite or lie outside, outputs left out, an empty call and calls
// that are refused.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "subpix_host.cpp"

static const int N = 2, H = 23, W = 31;

template <class Pixel>
static Pixel* make_images() {
  Pixel* im = (Pixel*)malloc((size_t)N * H * W * sizeof(Pixel));
  unsigned s = 12345u;
  for (int k = 0; k < N; ++k)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        s = s * 1664525u + 1013904223u;
        const double v = 128.0 + 90.0 * sin(0.45 * x + 0.3 * k) * cos(0.37 * y) + (double)(s >> 28);
        im[((size_t)k * H + y) * W + x] = (Pixel)v;
      }
  return im;
}

// one call over `n` corners with every array exactly its size; returns the number of complaints
static int run(const void* images, int dtype, int n, const double* xy, const int32_t* of, int wx, int wy, int zx, int zy, int max_iter,
               bool optional, int want_rc, int want_status) {
  const int m = n > 0 ? n : 1;
  double* corners = (double*)malloc((size_t)m * 2 * sizeof(double));
  for (int i = 0; i < 2 * n; ++i) corners[i] = xy[i];
  int32_t* image_of = nullptr;
  if (of) {
    image_of = (int32_t*)malloc((size_t)m * sizeof(int32_t));
    for (int i = 0; i < n; ++i) image_of[i] = of[i];
  }
  double* refined = (double*)malloc((size_t)m * 2 * sizeof(double));
  uint8_t* status = (uint8_t*)malloc((size_t)m);
  int32_t* iters = optional ? (int32_t*)malloc((size_t)m * sizeof(int32_t)) : nullptr;
  double* quality = optional ? (double*)malloc((size_t)m * sizeof(double)) : nullptr;
  const int rc = sph_refine_corners(images, N, H, W, dtype, n, corners, image_of, wx, wy, zx, zy, max_iter, 1e-4, refined, status, iters,
                                    quality);
  int bad = 0;
  if ((rc != 0) != (want_rc != 0)) { fprintf(stderr, "rc %d, expected %d: %s\n", rc, want_rc, sph_last_error()); bad = 1; }
  if (rc == 0)
    for (int k = 0; k < n; ++k) {
      if (status[k] > MCBA_SUBPIX_INVALID) { fprintf(stderr, "corner %d: status %d\n", k, status[k]); bad = 1; }
      if (want_status >= 0 && status[k] != want_status) { fprintf(stderr, "corner %d: status %d, expected %d\n", k, status[k], want_status); bad = 1; }
      const bool invalid = status[k] == MCBA_SUBPIX_INVALID;
      if (invalid || status[k] == MCBA_SUBPIX_REVERTED) {
        // (the start comes back bit for bit, NaN included)
        if (memcmp(refined + 2 * k, corners + 2 * k, 2 * sizeof(double)) != 0) { fprintf(stderr, "corner %d: the start is not returned\n", k); bad = 1; }
      } else if (fabs(refined[2 * k] - corners[2 * k]) > wx || fabs(refined[2 * k + 1] - corners[2 * k + 1]) > wy) {
        fprintf(stderr, "corner %d moved further than the window\n", k);
        bad = 1;
      }
      if (iters && (iters[k] < (invalid ? 0 : 1) || iters[k] > (invalid ? 0 : max_iter))) { fprintf(stderr, "corner %d: %d iterations\n", k, iters[k]); bad = 1; }
      if (quality && (invalid ? quality[k] == quality[k] : !(quality[k] >= 0.0))) { fprintf(stderr, "corner %d: quality %g\n", k, quality[k]); bad = 1; }
    }
  free(corners); free(image_of); free(refined); free(status); free(iters); free(quality);
  return bad;
}

int main() {
  uint8_t* u8 = make_images<uint8_t>();
  float* f32 = make_images<float>();
  // starts on and near every border and image corner
  const double xs[7] = {0.0, 0.3, 2.6, 15.5, 28.2, 29.9, 30.999}, ys[7] = {0.0, 0.7, 3.1, 11.5, 19.8, 21.6, 22.999};
  double border[98];
  int32_t of[49];
  for (int i = 0; i < 7; ++i)
    for (int j = 0; j < 7; ++j) {
      border[2 * (7 * i + j)] = xs[j];
      border[2 * (7 * i + j) + 1] = ys[i];
      of[7 * i + j] = (i + j) % N;
    }
  const double invalid[16] = {NAN, 3.0, 3.0, NAN, INFINITY, 3.0, 3.0, -INFINITY, -0.25, 3.0, 3.0, -1e-12, (double)W, 3.0, 3.0, (double)H};
  const int wins[5][2] = {{1, 1}, {5, 5}, {15, 15}, {15, 1}, {2, 15}};
  int bad = 0;
  for (int t = 0; t < 2; ++t) {
    const void* images = t == 0 ? (const void*)u8 : (const void*)f32;
    for (int k = 0; k < 5; ++k) {
      bad += run(images, t, 49, border, of, wins[k][0], wins[k][1], -1, -1, 30, true, 0, -1);
      bad += run(images, t, 49, border, nullptr, wins[k][0], wins[k][1], 0, 0, 3, false, 0, -1);      // zero zone, outputs left out
      bad += run(images, t, 8, invalid, of, wins[k][0], wins[k][1], -1, -1, 30, true, 0, MCBA_SUBPIX_INVALID);
    }
    bad += run(images, t, 0, border, nullptr, 5, 5, -1, -1, 30, true, 0, -1);                           // no corner
  }
  // refused: window, iterations, pixel type, an image index
  bad += run(u8, 0, 4, border, of, 0, 5, -1, -1, 30, true, 1, -1);
  bad += run(u8, 0, 4, border, of, 5, 16, -1, -1, 30, true, 1, -1);
  bad += run(u8, 0, 4, border, of, 5, 5, -1, -1, 0, true, 1, -1);
  bad += run(u8, 0, 4, border, of, 5, 5, -1, -1, 101, true, 1, -1);
  bad += run(u8, 2, 4, border, of, 5, 5, -1, -1, 30, true, 1, -1);
  const int32_t beyond[4] = {0, 1, 2, 0}, negative[4] = {0, -1, 0, 0};
  bad += run(u8, 0, 4, border, beyond, 5, 5, -1, -1, 30, true, 1, -1);
  bad += run(u8, 0, 4, border, negative, 5, 5, -1, -1, 30, true, 1, -1);
  // an empty call touches no array
  bad += sph_refine_corners(nullptr, 0, 0, 0, 0, 0, nullptr, nullptr, 5, 5, -1, -1, 30, 1e-4, nullptr, nullptr, nullptr, nullptr);
  free(u8); free(f32);
  if (bad) { fprintf(stderr, "a case failed\n"); return 1; }
  printf("subpix sanitize run: ok\n");
  return 0;
}
