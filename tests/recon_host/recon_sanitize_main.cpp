// TEST INFRASTRUCTURE: stand-alone program around the host build of the reconstruction-uncertainty mathematics and the driver's
// planning code, compiled by tests/test_reconstruction_uncertainty_host.py with -fsanitize=address,undefined and run on the CPU.
// Every input and every output is a heap block of exactly its size, so a read or a store outside it stops the program.  Four cameras
// (5 and 4 Brown-Conrady coefficients, one Kannala-Brandt, one 8-coefficient) serve the edge cases: both references, groups of 2, 3
// and 4, r = 0, 1, 17 and 128, masks, a point behind the cameras, a point far to one side, an unconstrained camera, the masks
// left out, an empty call and calls that are refused.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "recon_host.cpp"

static const int C = 4, ND = 8, STRIDE = 5 + ND;
static double* g_cams;
static int32_t* g_nd;
static uint8_t* g_fish;
static double* g_poses;

// one job of G cameras (slot s = camera order[s]) with W of exactly 24 * r doubles per slot, n points
static int run(int G, const int* order, int ref, int r, const double* pts, const uint64_t* masks_in, int n, int loose_slot, int want_rc,
               int want_status0) {
  mcba_recon_job job = {};
  job.G = G; job.reference = ref; job.r = r; job.n = n;
  double* W[8] = {};
  unsigned s = 99u + 7u * G + r;
  for (int k = 0; k < G && k < 8; ++k) {
    job.cameras[k] = order[k];
    job.image_w[k] = 200.0; job.image_h[k] = 150.0;
    job.unconstrained[k] = k == loose_slot ? 1 : 0;
    W[k] = r > 0 ? (double*)malloc((size_t)24 * r * sizeof(double)) : nullptr;
    const int c = order[k];
    const int own = c >= 0 && c < C ? 4 + (g_fish[c] ? 4 : g_nd[c]) : 18;
    for (int i = 0; i < 24 * r; ++i) {
      s = s * 1664525u + 1013904223u;
      const int row = i / r;
      W[k][i] = row >= own && row < 18 ? 0.0 : 1e-4 * ((double)(s >> 8) / 16777216.0 - 0.5);
    }
    job.W[k] = W[k];
  }
  const int m = n > 0 ? n : 1;
  double* points = (double*)malloc((size_t)m * 3 * sizeof(double));
  if (n > 0) memcpy(points, pts, (size_t)n * 3 * sizeof(double));
  uint64_t* masks = nullptr;
  if (masks_in) {
    masks = (uint64_t*)malloc((size_t)m * sizeof(uint64_t));
    memcpy(masks, masks_in, (size_t)n * sizeof(uint64_t));
  }
  double* cal = (double*)malloc((size_t)m * 6 * sizeof(double));
  double* noise = (double*)malloc((size_t)m * 6 * sizeof(double));
  int32_t* nv = (int32_t*)malloc((size_t)m * sizeof(int32_t));
  uint64_t* views = (uint64_t*)malloc((size_t)m * sizeof(uint64_t));
  uint8_t* status = (uint8_t*)malloc((size_t)m);
  mcba_camera_set cams = {C, g_cams, ND, g_nd, g_fish};
  const int rc = rch_reconstruction_uncertainty(&cams, g_poses, 1, &job, points, masks, 0.25, 0.0, cal, noise, nv, views, status);
  int bad = 0;
  if ((rc != 0) != (want_rc != 0)) { fprintf(stderr, "rc %d, expected %d: %s\n", rc, want_rc, rch_last_error()); bad = 1; }
  if (rc == 0 && n > 0 && want_status0 >= 0 && status[0] != want_status0) {
    fprintf(stderr, "G %d ref %d r %d: status %d, expected %d\n", G, ref, r, status[0], want_status0);
    bad = 1;
  }
  if (rc == 0 && n > 0 && want_status0 == MCBA_RECON_OK) {
    if (!(cal[0] >= 0.0) || !(cal[3] >= 0.0) || !(cal[5] >= 0.0) || !(noise[0] > 0.0)) { fprintf(stderr, "a variance is negative or NaN\n"); bad = 1; }
    if (r == 0)
      for (int i = 0; i < 6; ++i)
        if (cal[i] != 0.0) { fprintf(stderr, "not exactly 0\n"); bad = 1; }
  }
  if (rc == 0 && n > 0 && want_status0 > 0 && (cal[0] == cal[0] || noise[0] == noise[0])) { fprintf(stderr, "no NaN with status %d\n", want_status0); bad = 1; }
  if (rc == 0 && n > 0) {           // the rows of the same point, in a block of exactly 3 x 24 G
    double* Gm = (double*)malloc((size_t)3 * 24 * G * sizeof(double));
    int32_t st = -1;
    if (rch_query_rows(&cams, g_poses, &job, points, masks ? masks[0] : ~(uint64_t)0, 0.0, Gm, &st) != 0) { fprintf(stderr, "query_rows: %s\n", rch_last_error()); bad = 1; }
    free(Gm);
  }
  for (int k = 0; k < 8; ++k) free(W[k]);
  free(points); free(masks); free(cal); free(noise); free(nv); free(views); free(status);
  return bad;
}

int main() {
  g_cams = (double*)calloc((size_t)C * STRIDE, sizeof(double));
  const double blocks[4][13] = {{200.0, 205.0, 100.0, 75.0, 0.0, -0.12, 0.3, 1e-3, -1e-3, -0.2, 0.0, 0.0, 0.0},
                                {210.0, 200.0, 98.0, 77.0, 0.0, -0.1, 0.2, 1e-3, 1e-3, 0.0, 0.0, 0.0, 0.0},
                                {190.0, 195.0, 101.0, 74.0, 0.0, 0.05, 0.01, -0.005, 0.001, 0.0, 0.0, 0.0, 0.0},
                                {205.0, 204.0, 99.0, 76.0, 0.0, -0.1, 0.1, 1e-3, -1e-3, 0.05, 0.02, 0.01, 0.005}};
  for (int c = 0; c < C; ++c)
    for (int i = 0; i < STRIDE; ++i) g_cams[c * STRIDE + i] = blocks[c][i];
  g_nd = (int32_t*)malloc(C * sizeof(int32_t));
  g_fish = (uint8_t*)malloc(C);
  g_nd[0] = 5; g_nd[1] = 4; g_nd[2] = 4; g_nd[3] = 8;
  g_fish[0] = 0; g_fish[1] = 0; g_fish[2] = 1; g_fish[3] = 0;
  g_poses = (double*)calloc((size_t)C * 12, sizeof(double));
  for (int c = 0; c < C; ++c) {
    double* T = g_poses + 12 * c;
    T[0] = T[5] = T[10] = 1.0;
    T[3] = -0.1 * (c - 1.5);
  }
  const double pts[12] = {0.0, 0.0, 1.5, 0.1, -0.05, 2.5, 0.0, 0.0, -1.0, 0.9, 0.0, 1.5};
  const double behind[3] = {0.0, 0.0, -1.0};
  const double side[3] = {0.93, 0.0, 1.5};         // far to one side: fewer than two cameras have it in their image
  const uint64_t all[4] = {~(uint64_t)0, 3, 5, 6}, one[1] = {2};
  const int o4[4] = {0, 1, 2, 3}, o3[3] = {3, 1, 0}, o2[2] = {2, 0}, twice[3] = {0, 1, 0}, beyond[2] = {0, 4}, o9[9] = {0, 1, 2, 3, 0, 1, 2, 3, 0};
  const double nonfinite[3] = {0.0, NAN, 1.0};
  int bad = 0;
  const int ranks[4] = {0, 1, 17, 128};
  for (int k = 0; k < 4; ++k) {
    bad += run(4, o4, -1, ranks[k], pts, nullptr, 4, -1, 0, MCBA_RECON_OK);
    bad += run(4, o4, 2, ranks[k], pts, all, 4, -1, 0, MCBA_RECON_OK);
    bad += run(3, o3, 3, ranks[k], pts, all, 2, -1, 0, MCBA_RECON_OK);
    bad += run(2, o2, -1, ranks[k], pts, nullptr, 2, -1, 0, MCBA_RECON_OK);
  }
  bad += run(4, o4, -1, 5, behind, nullptr, 1, -1, 0, MCBA_RECON_TOO_FEW);
  bad += run(4, o4, 0, 5, side, nullptr, 1, -1, 0, MCBA_RECON_TOO_FEW);
  bad += run(4, o4, 1, 5, pts, one, 1, -1, 0, MCBA_RECON_TOO_FEW);                     // the mask leaves one camera
  bad += run(3, o3, -1, 5, pts, nullptr, 1, 1, 0, MCBA_RECON_UNCONSTRAINED);
  bad += run(3, o3, 1, 5, pts, all + 2, 1, 1, 0, MCBA_RECON_UNCONSTRAINED);            // the reference camera, masked out of the views
  bad += run(4, o4, -1, 5, pts, nullptr, 0, -1, 0, -1);                                // no point
  bad += run(1, o4, -1, 5, pts, nullptr, 1, -1, 1, -1);                                // refused: G
  bad += run(9, o9, -1, 5, pts, nullptr, 1, -1, 1, -1);
  bad += run(2, o2, 1, 5, pts, nullptr, 1, -1, 1, -1);                                 // refused: the reference is not in the group
  bad += run(3, twice, -1, 5, pts, nullptr, 1, -1, 1, -1);                             // refused: a camera twice
  bad += run(2, beyond, -1, 5, pts, nullptr, 1, -1, 1, -1);                            // refused: a camera that does not exist
  bad += run(2, o2, -1, 129, pts, nullptr, 0, -1, 1, -1);                              // refused: r
  bad += run(2, o2, -1, 5, nonfinite, nullptr, 1, -1, 1, -1);                          // refused: points
  // an empty call touches no array
  mcba_camera_set cams = {C, g_cams, ND, g_nd, g_fish};
  bad += rch_reconstruction_uncertainty(&cams, nullptr, 0, nullptr, nullptr, nullptr, 1.0, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr);
  free(g_cams); free(g_nd); free(g_fish); free(g_poses);
  if (bad) { fprintf(stderr, "a case failed\n"); return 1; }
  printf("reconstruction sanitize run: ok\n");
  return 0;
}
