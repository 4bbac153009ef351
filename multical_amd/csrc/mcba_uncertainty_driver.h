// mcba_uncertainty_driver.h -- host side of mcba_projection_uncertainty that does not touch the device: argument checks, the job
// records (camera entries, R_ba | t_ba, W^T in the fixed column order of mcba_uncertainty.h) and where each job's queries, tiles and
// pixels start.  Shared by the driver (mcba_uncertainty.hip) and the host build of the mathematics (tests/uncertainty_host), so that
// both refuse the same calls with the same messages.
#pragma once
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/mcba.h"
#include "mcba_uncertainty.h"
#include "mcba_undistort_driver.h"

namespace mcba {
namespace uncertainty {

static_assert(KP == MCBA_UNC_MAX_K, "mcba.h states the widest job");
static_assert(ST_OK == MCBA_UNC_OK && ST_NOT_CONVERGED == MCBA_UNC_NOT_CONVERGED && ST_BEHIND == MCBA_UNC_BEHIND &&
              ST_UNCONSTRAINED == MCBA_UNC_UNCONSTRAINED, "mcba.h states the status bytes");

constexpr int TILE = 256;         // queries a workgroup serves at a time

struct Plan {
  std::vector<double> recs;       // [n_jobs][REC_STRIDE]
  std::vector<int64_t> first;     // [n_jobs + 1] first output slot of every job
  std::vector<int64_t> tile_first;  // [n_jobs + 1] first tile of every job
  std::vector<int64_t> uv_first;  // [n_jobs] first pixel of a list job in `uv`, -1: a grid
  std::vector<double> grid;       // [n_jobs][4] u0 v0 du dv
  std::vector<int32_t> grid_w;    // [n_jobs]
  std::vector<double> uv;         // the lists, one after the other
  int64_t n_queries = 0;
};

inline bool finite_arg(double v) { return v - v == 0.0; }

// column of the record that row k of a job's W goes to
inline int record_column(int k, int ki_b, bool has_a) {
  if (k < ki_b) return COL_CAM_B + k;
  k -= ki_b;
  if (k < 6) return COL_POSE_B + k;
  k -= 6;
  if (!has_a) return -1;
  if (k < 6) return COL_POSE_A + k;
  return COL_CAM_A + (k - 6);
}

inline bool plan_jobs(const mcba_camera_set* cams, const double* camera_poses, int32_t n_jobs, const mcba_uncertainty_job* jobs,
                      const double* cov, const uint8_t* status, Plan& out, std::string& err) {
  const char* who = "mcba_projection_uncertainty";
  const std::string w(who);
  undistort::CameraPlan plan;
  if (!undistort::plan_cameras(cams, who, plan, err)) return false;
  const int C = cams->C;
  if (n_jobs < 0) { err = w + ": negative n_jobs"; return false; }
  if (n_jobs > 0 && (!jobs || !camera_poses)) { err = w + ": null argument"; return false; }
  for (int c = 0; c < C; ++c) {
    double* e = plan.cam.data() + (size_t)c * CAM_STRIDE;
    e[CAM_ISFISH] = plan.cam_fish[c] ? 1.0 : 0.0;
    e[REC_ND] = (double)plan.cam_nd[c];
  }
  out.recs.assign((size_t)n_jobs * REC_STRIDE, 0.0);
  out.first.assign((size_t)n_jobs + 1, 0);
  out.tile_first.assign((size_t)n_jobs + 1, 0);
  out.uv_first.assign((size_t)n_jobs, -1);
  out.grid.assign((size_t)n_jobs * 4, 0.0);
  out.grid_w.assign((size_t)n_jobs, 0);
  out.uv.clear();
  char msg[240];
  for (int j = 0; j < n_jobs; ++j) {
    const mcba_uncertainty_job& job = jobs[j];
    const int b = job.camera, a = job.reference;
    if (b < 0 || b >= C) { snprintf(msg, sizeof msg, "%s: job %d: camera %d of %d", who, j, b, C); err = msg; return false; }
    if (a >= C) { snprintf(msg, sizeof msg, "%s: job %d: reference %d of %d", who, j, a, C); err = msg; return false; }
    const bool has_a = a >= 0;
    if (!finite_arg(job.inv_distance) || job.inv_distance < 0.0) {
      snprintf(msg, sizeof msg, "%s: job %d: inv_distance must be finite and >= 0", who, j);
      err = msg;
      return false;
    }
    const int ki_b = 4 + plan.cam_nd[b], ki_a = has_a ? 4 + plan.cam_nd[a] : 0;
    const int K = ki_b + 6 + (has_a ? 6 + ki_a : 0);
    if (job.K != K) {
      snprintf(msg, sizeof msg, "%s: job %d: K = %d, the columns of these cameras are %d", who, j, job.K, K);
      err = msg;
      return false;
    }
    if (job.r < 0 || job.r > MAX_RANK) {
      snprintf(msg, sizeof msg, "%s: job %d: r = %d, W has 0 .. %d columns", who, j, job.r, MAX_RANK);
      err = msg;
      return false;
    }
    if (job.r > 0 && !job.W) { snprintf(msg, sizeof msg, "%s: job %d: W is null", who, j); err = msg; return false; }
    int64_t n = 0;
    if (job.grid_w > 0) {
      if (job.grid_h <= 0 || !finite_arg(job.u0) || !finite_arg(job.v0) || !finite_arg(job.du) || !finite_arg(job.dv)) {
        snprintf(msg, sizeof msg, "%s: job %d: a grid needs grid_h > 0 and finite u0, v0, du, dv", who, j);
        err = msg;
        return false;
      }
      n = (int64_t)job.grid_w * job.grid_h;
      out.grid_w[j] = job.grid_w;
      out.grid[4 * j] = job.u0; out.grid[4 * j + 1] = job.v0; out.grid[4 * j + 2] = job.du; out.grid[4 * j + 3] = job.dv;
    } else {
      if (job.grid_w < 0 || job.n < 0) { snprintf(msg, sizeof msg, "%s: job %d: negative size", who, j); err = msg; return false; }
      if (job.n > 0 && !job.uv) { snprintf(msg, sizeof msg, "%s: job %d: uv is null", who, j); err = msg; return false; }
      n = job.n;
      out.uv_first[j] = (int64_t)(out.uv.size() / 2);
      out.uv.insert(out.uv.end(), job.uv, job.uv + 2 * n);
    }
    out.first[j + 1] = out.first[j] + n;
    out.tile_first[j + 1] = out.tile_first[j] + (n + TILE - 1) / TILE;
    // the record
    double* rec = out.recs.data() + (size_t)j * REC_STRIDE;
    const double* eb = plan.cam.data() + (size_t)b * CAM_STRIDE;
    for (int i = 0; i < CAM_STRIDE; ++i) rec[REC_CAM_B + i] = eb[i];
    rec[REC_RHO] = job.inv_distance;
    rec[REC_HAS_A] = has_a ? 1.0 : 0.0;
    rec[REC_RANK] = (double)job.r;
    if (has_a) {
      const double* ea = plan.cam.data() + (size_t)a * CAM_STRIDE;
      for (int i = 0; i < CAM_STRIDE; ++i) rec[REC_CAM_A + i] = ea[i];
      const double* Tb = camera_poses + 16 * (size_t)b;
      const double* Ta = camera_poses + 16 * (size_t)a;
      for (int i = 0; i < 3; ++i) {          // R_ba = R_b R_a^T, t_ba = t_b - R_ba t_a
        for (int k = 0; k < 3; ++k)
          rec[REC_R + 3 * i + k] = Tb[4 * i] * Ta[4 * k] + Tb[4 * i + 1] * Ta[4 * k + 1] + Tb[4 * i + 2] * Ta[4 * k + 2];
        rec[REC_T + i] = Tb[4 * i + 3] - (rec[REC_R + 3 * i] * Ta[3] + rec[REC_R + 3 * i + 1] * Ta[7] + rec[REC_R + 3 * i + 2] * Ta[11]);
      }
      for (int i = 0; i < 12; ++i)
        if (!finite_arg(rec[REC_R + i])) { snprintf(msg, sizeof msg, "%s: job %d: camera_poses are not finite", who, j); err = msg; return false; }
    }
    if (a == b) {                            // the point is where camera b itself sees it: exactly 0, whatever W says
      rec[REC_RANK] = 0.0;
      continue;
    }
    int loose = 0;
    for (int k = 0; k < K; ++k) loose += job.unconstrained && job.unconstrained[k] ? 1 : 0;
    if (loose + job.r > MAX_RANK) {
      snprintf(msg, sizeof msg, "%s: job %d: %d unconstrained columns and r = %d, together at most %d", who, j, loose, job.r, MAX_RANK);
      err = msg;
      return false;
    }
    rec[REC_LOOSE] = (double)loose;
    int unit = 0;
    for (int k = 0; k < K; ++k) {
      const int col = record_column(k, ki_b, has_a);
      if (job.unconstrained && job.unconstrained[k]) rec[REC_W + (unit++) * KP + col] = 1.0;
      for (int c = 0; c < job.r; ++c) {
        const double v = job.W[(size_t)k * job.r + c];
        if (!finite_arg(v)) { snprintf(msg, sizeof msg, "%s: job %d: W is not finite", who, j); err = msg; return false; }
        rec[REC_W + (loose + c) * KP + col] = v;
      }
    }
  }
  out.n_queries = out.first[n_jobs];
  if (out.n_queries > 0 && (!cov || !status)) { err = w + ": null argument"; return false; }
  return true;
}

}  // namespace uncertainty
}  // namespace mcba
