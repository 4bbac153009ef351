// TEST INFRASTRUCTURE: stand-alone program around the host build of the pair mathematics (mcba_recon.h: pair_query) and the driver's
// planning code for the pair list, compiled by tests/test_length_uncertainty_host.py with -fsanitize=address,undefined and run on the
// CPU.  Every input and every output is a heap block of exactly its size, so a read or a store outside it stops the program.  Four
// cameras (5 and 4 Brown-Conrady coefficients, one Kannala-Brandt, one 8-coefficient) serve the edge cases: both references, groups of
// 2, 3 and 4, r = 0, 1, 17 and 128, pairs (first, last), (last, first) and (k, k), an end behind the cameras, masks, every output left
// out in turn, two jobs whose pairs index their own points, no pair at all, and pair lists that are refused.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "length_host.cpp"

static const int C = 4, ND = 8, STRIDE = 5 + ND;
static double* g_cams;
static int32_t* g_nd;
static uint8_t* g_fish;
static double* g_poses;

struct JobSpec {
  int G;
  const int* order;
  int ref, r, n, k;          // n points, k pairs
};

static void fill_job(mcba_recon_job& job, const JobSpec& sp, double** W) {
  job = mcba_recon_job();
  job.G = sp.G; job.reference = sp.ref; job.r = sp.r; job.n = sp.n;
  unsigned s = 99u + 7u * sp.G + sp.r;
  for (int k = 0; k < sp.G && k < 8; ++k) {
    job.cameras[k] = sp.order[k];
    job.image_w[k] = 200.0; job.image_h[k] = 150.0;
    W[k] = sp.r > 0 ? (double*)malloc((size_t)24 * sp.r * sizeof(double)) : nullptr;
    const int c = sp.order[k];
    const int own = c >= 0 && c < C ? 4 + (g_fish[c] ? 4 : g_nd[c]) : 18;
    for (int i = 0; i < 24 * sp.r; ++i) {
      s = s * 1664525u + 1013904223u;
      const int row = i / sp.r;
      W[k][i] = row >= own && row < 18 ? 0.0 : 1e-4 * ((double)(s >> 8) / 16777216.0 - 0.5);
    }
    job.W[k] = W[k];
  }
}

// n_jobs jobs over their points and pairs, every array exactly its size; leave_out: the output that is passed as null (-1: none).
// want_status: of every pair, or null
static int run(int n_jobs, const JobSpec* specs, const double* pts, const uint64_t* masks_in, const int64_t* pairs_in, int leave_out,
               int want_rc, const int* want_status) {
  mcba_recon_job jobs[2];
  double* W[2][8] = {};
  int n = 0, K = 0;
  int64_t n_pairs[2] = {0, 0};
  for (int j = 0; j < n_jobs; ++j) {
    fill_job(jobs[j], specs[j], W[j]);
    n += specs[j].n;
    K += specs[j].k;
    n_pairs[j] = specs[j].k;
  }
  const int m = n > 0 ? n : 1, Km = K > 0 ? K : 1;
  double* points = (double*)malloc((size_t)m * 3 * sizeof(double));
  if (n > 0) memcpy(points, pts, (size_t)n * 3 * sizeof(double));
  uint64_t* masks = nullptr;
  if (masks_in) {
    masks = (uint64_t*)malloc((size_t)m * sizeof(uint64_t));
    memcpy(masks, masks_in, (size_t)n * sizeof(uint64_t));
  }
  int64_t* pairs = (int64_t*)malloc((size_t)Km * 2 * sizeof(int64_t));
  if (K > 0) memcpy(pairs, pairs_in, (size_t)K * 2 * sizeof(int64_t));
  int64_t* counts = (int64_t*)malloc((size_t)(n_jobs > 0 ? n_jobs : 1) * sizeof(int64_t));
  for (int j = 0; j < n_jobs; ++j) counts[j] = n_pairs[j];
  double* cal = leave_out == 0 ? nullptr : (double*)malloc((size_t)Km * 6 * sizeof(double));
  double* cross = leave_out == 1 ? nullptr : (double*)malloc((size_t)Km * 9 * sizeof(double));
  double* noise = leave_out == 2 ? nullptr : (double*)malloc((size_t)Km * 6 * sizeof(double));
  double* length = leave_out == 3 ? nullptr : (double*)malloc((size_t)Km * sizeof(double));
  double* var_cal = leave_out == 4 ? nullptr : (double*)malloc((size_t)Km * sizeof(double));
  double* var_noise = leave_out == 5 ? nullptr : (double*)malloc((size_t)Km * sizeof(double));
  uint64_t* va = leave_out == 6 ? nullptr : (uint64_t*)malloc((size_t)Km * sizeof(uint64_t));
  uint64_t* vb = leave_out == 7 ? nullptr : (uint64_t*)malloc((size_t)Km * sizeof(uint64_t));
  uint8_t* status = leave_out == 8 ? nullptr : (uint8_t*)malloc((size_t)Km);
  mcba_camera_set cams = {C, g_cams, ND, g_nd, g_fish};
  const int rc = lph_reconstruction_pairs(&cams, g_poses, n_jobs, jobs, points, masks, counts, pairs, 0.25, 0.0, cal, cross, noise, length,
                                          var_cal, var_noise, va, vb, status);
  int bad = 0;
  if ((rc != 0) != (want_rc != 0)) { fprintf(stderr, "rc %d, expected %d: %s\n", rc, want_rc, lph_last_error()); bad = 1; }
  if (rc == 0 && want_status && status)
    for (int k = 0; k < K; ++k) {
      if (status[k] != want_status[k]) { fprintf(stderr, "pair %d: status %d, expected %d\n", k, status[k], want_status[k]); bad = 1; }
      const bool same = pairs[2 * k] == pairs[2 * k + 1], ok = status[k] == MCBA_RECON_OK;
      if (cal && ok && (!(cal[6 * k] >= 0.0) || !(cal[6 * k + 3] >= 0.0) || !(cal[6 * k + 5] >= 0.0))) { fprintf(stderr, "a variance is negative or NaN\n"); bad = 1; }
      if (cal && !ok && cal[6 * k] == cal[6 * k]) { fprintf(stderr, "no NaN with status %d\n", status[k]); bad = 1; }
      if (cal && noise && ok && same)
        for (int i = 0; i < 6; ++i)
          if (cal[6 * k + i] != 0.0 || noise[6 * k + i] != 0.0) { fprintf(stderr, "a == b is not exactly 0\n"); bad = 1; }
      if (var_cal && ok && same && var_cal[k] == var_cal[k]) { fprintf(stderr, "a length of 0 has a variance\n"); bad = 1; }
      if (var_cal && ok && !same && !(var_cal[k] >= 0.0)) { fprintf(stderr, "the variance of a length is negative or NaN\n"); bad = 1; }
      if (length && !(length[k] >= 0.0)) { fprintf(stderr, "a length is negative or NaN\n"); bad = 1; }
    }
  for (int j = 0; j < 2; ++j)
    for (int k = 0; k < 8; ++k) free(W[j][k]);
  free(points); free(masks); free(pairs); free(counts); free(cal); free(cross); free(noise); free(length); free(var_cal); free(var_noise);
  free(va); free(vb); free(status);
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
  // points 0, 1, 3: in front of every camera; point 2: behind them
  const double pts[12] = {0.0, 0.0, 1.5, 0.1, -0.05, 2.5, 0.0, 0.0, -1.0, 0.01, 0.0, 1.5};
  const uint64_t all[4] = {~(uint64_t)0, 3, 5, 6};
  const int o4[4] = {0, 1, 2, 3}, o3[3] = {3, 1, 0}, o2[2] = {2, 0};
  const int OK = MCBA_RECON_OK, TF = MCBA_RECON_TOO_FEW;
  // (first, last), (last, first), (k, k), an end behind the cameras on either side, a failed point with itself
  const int64_t pairs[14] = {0, 3, 3, 0, 1, 1, 0, 2, 2, 1, 2, 2, 1, 3};
  const int want[7] = {OK, OK, OK, TF, TF, TF, OK};
  int bad = 0;
  const int ranks[4] = {0, 1, 17, 128};
  for (int k = 0; k < 4; ++k) {
    const JobSpec a = {4, o4, -1, ranks[k], 4, 7}, b = {4, o4, 2, ranks[k], 4, 7}, c = {3, o3, 3, ranks[k], 4, 7}, d = {2, o2, -1, ranks[k], 4, 7};
    bad += run(1, &a, pts, nullptr, pairs, -1, 0, want);
    bad += run(1, &b, pts, all, pairs, -1, 0, nullptr);
    bad += run(1, &c, pts, nullptr, pairs, -1, 0, want);
    bad += run(1, &d, pts, nullptr, pairs, -1, 0, want);
  }
  const JobSpec one = {4, o4, 1, 5, 4, 7};
  for (int out = 0; out < 9; ++out) bad += run(1, &one, pts, nullptr, pairs, out, 0, want);    // every output left out in turn
  // two jobs: 3 points and 1 point; the second job's pair (0, 0) is ITS point 0, and index 1 does not exist there
  const JobSpec two[2] = {{4, o4, -1, 5, 3, 2}, {2, o2, 0, 3, 1, 1}};
  const int64_t own[6] = {0, 1, 2, 0, 0, 0}, beyond[6] = {0, 1, 2, 0, 0, 1};
  const int want_two[3] = {OK, TF, OK};
  bad += run(2, two, pts, nullptr, own, -1, 0, want_two);
  bad += run(2, two, pts, nullptr, beyond, -1, 1, nullptr);
  const JobSpec none = {4, o4, -1, 5, 4, 0};
  bad += run(1, &none, pts, nullptr, nullptr, -1, 0, nullptr);                                  // no pair
  const int64_t past[2] = {0, 4}, negative[2] = {-1, 0};
  const JobSpec single = {4, o4, -1, 5, 4, 1};
  bad += run(1, &single, pts, nullptr, past, -1, 1, nullptr);                                   // refused: an index past the job's points
  bad += run(1, &single, pts, nullptr, negative, -1, 1, nullptr);                               // refused: a negative index
  const JobSpec wide = {2, o2, -1, 129, 4, 1};
  bad += run(1, &wide, pts, nullptr, pairs, -1, 1, nullptr);                                    // refused: r
  // an empty call touches no array
  mcba_camera_set cams = {C, g_cams, ND, g_nd, g_fish};
  bad += lph_reconstruction_pairs(&cams, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 1.0, 0.0, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  free(g_cams); free(g_nd); free(g_fish); free(g_poses);
  if (bad) { fprintf(stderr, "a case failed\n"); return 1; }
  printf("length sanitize run: ok\n");
  return 0;
}
