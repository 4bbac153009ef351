// mcba_recon_driver.h -- host side of mcba_reconstruction_uncertainty that does not touch the device: argument checks and refusals,
// the job records of mcba_recon.h, the jobs' factors [24 G][ldw] zero-padded and one after the other, and where each job's points
// and tiles start; for mcba_reconstruction_pairs the same jobs and where each job's pairs and pair tiles start (plan_pairs).  Shared by
// the driver (mcba_recon.hip) and the host builds of the mathematics (tests/recon_host, tests/length_host), so that both refuse the
// same calls with the same messages.
#pragma once
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/mcba.h"
#include "mcba_recon.h"
#include "mcba_undistort_driver.h"

namespace mcba {
namespace recon {

static_assert(MAX_G == MCBA_RECON_MAX_CAMERAS && MAX_R == MCBA_RIG_MAX_R && KC == MCBA_RIG_COLUMNS, "mcba.h states the widest job");
static_assert(ST_OK == MCBA_RECON_OK && ST_TOO_FEW == MCBA_RECON_TOO_FEW && ST_DEGENERATE == MCBA_RECON_DEGENERATE &&
              ST_UNCONSTRAINED == MCBA_RECON_UNCONSTRAINED, "mcba.h states the status bytes");

constexpr int TILE = 16;          // points a wavefront serves at a time

struct Plan {
  std::vector<double> recs;         // [n_jobs][JR_STRIDE]
  std::vector<double> wdev;         // the factors
  std::vector<int64_t> w_first;     // [n_jobs]
  std::vector<int64_t> first;       // [n_jobs + 1] first point of every job
  std::vector<int64_t> tile_first;  // [n_jobs + 1]
  int64_t n_points = 0;
  int max_group = 0;
};

inline bool finite_arg(double v) { return v - v == 0.0; }

// the jobs of either entry (`who` names it in the messages); outputs_there: no output the entry requires is null
inline bool plan_jobs_of(const char* who, const mcba_camera_set* cams, const double* camera_poses, int32_t n_jobs,
                         const mcba_recon_job* jobs, const double* points, double sigma2, double margin, bool outputs_there, Plan& out,
                         std::string& err) {
  const std::string w(who);
  undistort::CameraPlan plan;
  if (!undistort::plan_cameras(cams, who, plan, err)) return false;
  const int C = cams->C;
  char msg[320];
  if (n_jobs < 0) { err = w + ": negative n_jobs"; return false; }
  if (n_jobs > 0 && (!jobs || !camera_poses)) { err = w + ": null argument"; return false; }
  if (!(sigma2 > 0.0) || !finite_arg(sigma2)) { err = w + ": sigma2 must be positive and finite"; return false; }
  if (!finite_arg(margin)) { err = w + ": margin must be finite"; return false; }
  if (n_jobs > 0)
    for (int i = 0; i < 12 * C; ++i)
      if (!finite_arg(camera_poses[i])) { err = w + ": camera_poses are not finite"; return false; }
  for (int c = 0; c < C; ++c) {
    double* e = plan.cam.data() + (size_t)c * CAM_STRIDE;
    e[CAM_ISFISH] = plan.cam_fish[c] ? 1.0 : 0.0;
    e[uncertainty::REC_ND] = (double)plan.cam_nd[c];
  }
  out.recs.assign((size_t)n_jobs * JR_STRIDE, 0.0);
  out.wdev.clear();
  out.w_first.assign((size_t)n_jobs, 0);
  out.first.assign((size_t)n_jobs + 1, 0);
  out.tile_first.assign((size_t)n_jobs + 1, 0);
  out.max_group = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const mcba_recon_job& job = jobs[j];
    const int G = job.G, r = job.r;
    if (G < 2 || G > MAX_G) {
      snprintf(msg, sizeof msg, "%s: job %d: G = %d: a group has 2 .. MCBA_RECON_MAX_CAMERAS = %d cameras", who, j, G, MAX_G);
      err = msg;
      return false;
    }
    if (r < 0 || r > MAX_R) {
      snprintf(msg, sizeof msg, "%s: job %d: r = %d: the factor of a group has 0 .. MCBA_RIG_MAX_R = %d columns; pass a smaller group",
               who, j, r, MAX_R);
      err = msg;
      return false;
    }
    if (job.n < 0) { snprintf(msg, sizeof msg, "%s: job %d: n is negative", who, j); err = msg; return false; }
    int ref_slot = -1;
    for (int s = 0; s < G; ++s) {
      const int c = job.cameras[s];
      if (c < 0 || c >= C) { snprintf(msg, sizeof msg, "%s: job %d: cameras[%d] = %d of %d", who, j, s, c, C); err = msg; return false; }
      for (int t = 0; t < s; ++t)
        if (job.cameras[t] == c) {
          snprintf(msg, sizeof msg, "%s: job %d: cameras[%d] = %d is repeated", who, j, s, c);
          err = msg;
          return false;
        }
      if (c == job.reference) ref_slot = s;
    }
    if (job.reference >= 0 && ref_slot < 0) {
      snprintf(msg, sizeof msg, "%s: job %d: reference %d is not a camera of the group", who, j, job.reference);
      err = msg;
      return false;
    }
    const int ldw = padded_columns(r);
    double* rec = out.recs.data() + (size_t)j * JR_STRIDE;
    rec[JR_G] = (double)G; rec[JR_REF] = (double)ref_slot; rec[JR_R] = (double)r; rec[JR_LDW] = (double)ldw; rec[JR_MARGIN] = margin;
    out.w_first[j] = (int64_t)out.wdev.size();
    out.wdev.resize(out.wdev.size() + (size_t)KC * G * ldw, 0.0);
    double* Wj = out.wdev.data() + out.w_first[j];
    for (int s = 0; s < G; ++s) {
      const int c = job.cameras[s];
      double* sl = rec + JR_SLOT + s * SL_STRIDE;
      const double* e = plan.cam.data() + (size_t)c * CAM_STRIDE;
      for (int i = 0; i < CAM_STRIDE; ++i) sl[i] = e[i];
      for (int i = 0; i < 12; ++i) sl[SL_POSE + i] = camera_poses[12 * (size_t)c + i];
      if (!(job.image_w[s] > 0.0) || !(job.image_h[s] > 0.0) || !finite_arg(job.image_w[s]) || !finite_arg(job.image_h[s])) {
        snprintf(msg, sizeof msg, "%s: job %d: image_w, image_h of slot %d must be positive", who, j, s); err = msg; return false;
      }
      sl[SL_W_IMG] = job.image_w[s]; sl[SL_H_IMG] = job.image_h[s];
      sl[SL_LOOSE] = job.unconstrained[s] ? 1.0 : 0.0;
      if (r > 0 && !job.W[s]) { snprintf(msg, sizeof msg, "%s: job %d: W[%d] is null", who, j, s); err = msg; return false; }
      for (int k = 0; k < KC; ++k)
        for (int q = 0; q < r; ++q) {
          const double v = job.W[s][(size_t)k * r + q];
          if (!finite_arg(v)) { snprintf(msg, sizeof msg, "%s: job %d: W[%d] is not finite", who, j, s); err = msg; return false; }
          if (k >= 4 + plan.cam_nd[c] && k < KI && v != 0.0) {
            snprintf(msg, sizeof msg, "%s: job %d: row %d of W[%d] belongs to a coefficient the camera does not have", who, j, k, s);
            err = msg;
            return false;
          }
          Wj[(size_t)(KC * s + k) * ldw + q] = v;
        }
    }
    out.first[j + 1] = out.first[j] + job.n;
    out.tile_first[j + 1] = out.tile_first[j] + (job.n + TILE - 1) / TILE;
    if (job.n > 0 && G > out.max_group) out.max_group = G;
  }
  out.n_points = out.first[n_jobs];
  if (out.n_points > 0 && (!points || !outputs_there)) { err = w + ": null argument"; return false; }
  for (int64_t i = 0; i < 3 * out.n_points; ++i)
    if (!finite_arg(points[i])) {
      snprintf(msg, sizeof msg, "%s: points: point %lld is not finite", who, (long long)(i / 3));
      err = msg;
      return false;
    }
  return true;
}

inline bool plan_jobs(const mcba_camera_set* cams, const double* camera_poses, int32_t n_jobs, const mcba_recon_job* jobs,
                      const double* points, double sigma2, double margin, const double* cov_cal, const double* cov_noise,
                      const int32_t* n_views, const uint64_t* views, const uint8_t* status, Plan& out, std::string& err) {
  return plan_jobs_of("mcba_reconstruction_uncertainty", cams, camera_poses, n_jobs, jobs, points, sigma2, margin,
                      cov_cal && cov_noise && n_views && views && status, out, err);
}

// ---- mcba_reconstruction_pairs: the jobs as above (every output may be left out) and where each job's pairs and pair tiles start
constexpr int PAIR_TILE = 8;      // pairs a wavefront serves at a time: the a ends in rows 0 .. 7 of the tile, the b ends in 8 .. 15
constexpr const char* PAIRS_ENTRY = "mcba_reconstruction_pairs";

struct PairPlan {
  Plan jobs;                        // (its tile_first counts point tiles and is not used)
  std::vector<int64_t> pair_first;  // [n_jobs + 1] first pair of every job
  std::vector<int64_t> tile_first;  // [n_jobs + 1] first pair tile of every job
  int64_t n_pairs = 0;
  int max_group = 0;                // the widest group among the jobs that have a pair
};

inline bool plan_pairs(const mcba_camera_set* cams, const double* camera_poses, int32_t n_jobs, const mcba_recon_job* jobs,
                       const double* points, const int64_t* n_pairs, const int64_t* pairs, double sigma2, double margin, PairPlan& out,
                       std::string& err) {
  const std::string w(PAIRS_ENTRY);
  if (!plan_jobs_of(PAIRS_ENTRY, cams, camera_poses, n_jobs, jobs, points, sigma2, margin, true, out.jobs, err)) return false;
  if (n_jobs > 0 && !n_pairs) { err = w + ": n_pairs is null"; return false; }
  char msg[320];
  out.pair_first.assign((size_t)n_jobs + 1, 0);
  out.tile_first.assign((size_t)n_jobs + 1, 0);
  out.max_group = 0;
  for (int j = 0; j < n_jobs; ++j) {
    if (n_pairs[j] < 0) { snprintf(msg, sizeof msg, "%s: job %d: n_pairs is negative", PAIRS_ENTRY, j); err = msg; return false; }
    out.pair_first[j + 1] = out.pair_first[j] + n_pairs[j];
    out.tile_first[j + 1] = out.tile_first[j] + (n_pairs[j] + PAIR_TILE - 1) / PAIR_TILE;
    if (n_pairs[j] > 0 && jobs[j].G > out.max_group) out.max_group = jobs[j].G;
  }
  out.n_pairs = out.pair_first[n_jobs];
  if (out.n_pairs > 0 && !pairs) { err = w + ": pairs is null"; return false; }
  for (int j = 0; j < n_jobs; ++j)
    for (int64_t k = 2 * out.pair_first[j]; k < 2 * out.pair_first[j + 1]; ++k)
      if (pairs[k] < 0 || pairs[k] >= jobs[j].n) {
        snprintf(msg, sizeof msg, "%s: pairs: pair %lld (%lld of job %d): index %lld is outside [0, n = %lld)", PAIRS_ENTRY,
                 (long long)(k / 2), (long long)(k / 2 - out.pair_first[j]), j, (long long)pairs[k], (long long)jobs[j].n);
        err = msg;
        return false;
      }
  return true;
}

}  // namespace recon
}  // namespace mcba
