// mcba_projdiff_driver.h -- host side of mcba_projection_diff that does not touch the device: argument checks, the job records (the
// camera entries of both calibrations, R_ba | t_ba of both), where each job's queries, tiles, pixels, fit pixels and rays start, and
// the fit records of the jobs that do not fit.  Shared by the driver (mcba_projdiff.hip) and the host build of the mathematics
// (tests/projdiff_host), so that both refuse the same calls with the same messages.
#pragma once
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/mcba.h"
#include "mcba_projdiff.h"
#include "mcba_undistort_driver.h"

namespace mcba {
namespace projdiff {

static_assert(ST_OK == MCBA_PDIFF_OK && ST_NOT_CONVERGED == MCBA_PDIFF_NOT_CONVERGED && ST_BEHIND == MCBA_PDIFF_BEHIND &&
              ST_NO_FIT == MCBA_PDIFF_NO_FIT, "mcba.h states the status bytes");
static_assert(FIT_OK == MCBA_PDIFF_FIT_OK && FIT_TOO_FEW == MCBA_PDIFF_FIT_TOO_FEW && FIT_NOT_CONVERGED == MCBA_PDIFF_FIT_NOT_CONVERGED &&
              FIT_DEGENERATE == MCBA_PDIFF_FIT_DEGENERATE, "mcba.h states the fit statuses");
static_assert(MODE_NONE == MCBA_PDIFF_MODE_NONE && MODE_ROTATION == MCBA_PDIFF_MODE_ROTATION && MODE_RIGID == MCBA_PDIFF_MODE_RIGID &&
              MAX_FIT_PIXELS == MCBA_PDIFF_MAX_FIT, "mcba.h states the fit modes");

constexpr int TILE = 256;         // queries a workgroup serves at a time

struct Plan {
  std::vector<double> recs;         // [n_jobs][REC_STRIDE]
  std::vector<double> fit;          // [n_jobs][FIT_STRIDE] the identity; the fit kernel overwrites those of the jobs that fit
  std::vector<int64_t> first;       // [n_jobs + 1] first output slot of every job
  std::vector<int64_t> tile_first;  // [n_jobs + 1] first tile of every job
  std::vector<PixelSet> queries;    // [n_jobs]
  std::vector<int32_t> fit_jobs;    // the jobs that fit
  std::vector<int64_t> ray_first;   // [fit_jobs + 1] first fit pixel of each in the scratch buffer
  std::vector<PixelSet> fit_pixels; // [fit_jobs]
  std::vector<Focus> focus;         // [fit_jobs]
  std::vector<double> uv;           // the lists (queries and fit pixels), one after the other
  int64_t n_queries = 0;
};

inline bool finite_arg(double v) { return undistort::finite_d(v); }

// a grid or a list -> a PixelSet and its size; false: refused (msg)
inline bool plan_pixels(const char* who, int j, const char* what, int32_t gw, int32_t gh, double u0, double v0, double du, double dv,
                        int64_t n_list, const double* list, std::vector<double>& uv, PixelSet& set, int64_t& n, std::string& err) {
  char msg[240];
  set = PixelSet{-1, 0, 0.0, 0.0, 0.0, 0.0};
  if (gw > 0) {
    if (gh <= 0 || !finite_arg(u0) || !finite_arg(v0) || !finite_arg(du) || !finite_arg(dv)) {
      snprintf(msg, sizeof msg, "%s: job %d: a %sgrid needs a height > 0 and finite u0, v0, du, dv", who, j, what);
      err = msg;
      return false;
    }
    n = (int64_t)gw * gh;
    set.grid_w = gw; set.u0 = u0; set.v0 = v0; set.du = du; set.dv = dv;
    return true;
  }
  if (gw < 0 || n_list < 0) { snprintf(msg, sizeof msg, "%s: job %d: negative %ssize", who, j, what); err = msg; return false; }
  if (n_list > 0 && !list) { snprintf(msg, sizeof msg, "%s: job %d: %suv is null", who, j, what); err = msg; return false; }
  n = n_list;
  set.list = (int64_t)(uv.size() / 2);
  uv.insert(uv.end(), list, list + 2 * n_list);
  return true;
}

// R_ba | t_ba of one calibration into rec[at ..]
inline void relative_pose(const double* poses, int b, int a, double* out) {
  const double* Tb = poses + 16 * (size_t)b;
  const double* Ta = poses + 16 * (size_t)a;
  for (int i = 0; i < 3; ++i) {          // R_ba = R_b R_a^T, t_ba = t_b - R_ba t_a
    for (int k = 0; k < 3; ++k) out[3 * i + k] = Tb[4 * i] * Ta[4 * k] + Tb[4 * i + 1] * Ta[4 * k + 1] + Tb[4 * i + 2] * Ta[4 * k + 2];
    out[9 + i] = Tb[4 * i + 3] - (out[3 * i] * Ta[3] + out[3 * i + 1] * Ta[7] + out[3 * i + 2] * Ta[11]);
  }
}

inline bool plan_jobs(const mcba_camera_set* cams0, const double* poses0, const mcba_camera_set* cams1, const double* poses1,
                      int32_t n_jobs, const mcba_projdiff_job* jobs, const double* diff, const uint8_t* status, Plan& out,
                      std::string& err) {
  const char* who = "mcba_projection_diff";
  const std::string w(who);
  undistort::CameraPlan plan[2];
  if (!undistort::plan_cameras(cams0, who, plan[0], err) || !undistort::plan_cameras(cams1, who, plan[1], err)) return false;
  const int C = cams0->C;
  char msg[240];
  if (cams1->C != C) { snprintf(msg, sizeof msg, "%s: %d and %d cameras", who, C, cams1->C); err = msg; return false; }
  if (n_jobs < 0) { err = w + ": negative n_jobs"; return false; }
  if (n_jobs > 0 && !jobs) { err = w + ": null argument"; return false; }
  for (int k = 0; k < 2; ++k)
    for (int c = 0; c < C; ++c) {
      double* e = plan[k].cam.data() + (size_t)c * CAM_STRIDE;
      e[CAM_ISFISH] = plan[k].cam_fish[c] ? 1.0 : 0.0;
      e[REC_ND] = (double)plan[k].cam_nd[c];
    }
  out.recs.assign((size_t)n_jobs * REC_STRIDE, 0.0);
  out.fit.assign((size_t)n_jobs * FIT_STRIDE, 0.0);
  out.first.assign((size_t)n_jobs + 1, 0);
  out.tile_first.assign((size_t)n_jobs + 1, 0);
  out.queries.assign((size_t)n_jobs, PixelSet{-1, 0, 0.0, 0.0, 0.0, 0.0});
  out.fit_jobs.clear();
  out.ray_first.assign(1, 0);
  out.fit_pixels.clear();
  out.focus.clear();
  out.uv.clear();
  for (int j = 0; j < n_jobs; ++j) {
    const mcba_projdiff_job& job = jobs[j];
    const int b = job.camera, a = job.reference;
    if (b < 0 || b >= C) { snprintf(msg, sizeof msg, "%s: job %d: camera %d of %d", who, j, b, C); err = msg; return false; }
    if (a >= C) { snprintf(msg, sizeof msg, "%s: job %d: reference %d of %d", who, j, a, C); err = msg; return false; }
    const bool has_a = a >= 0;
    if (!finite_arg(job.inv_distance) || job.inv_distance < 0.0) {
      snprintf(msg, sizeof msg, "%s: job %d: inv_distance must be finite and >= 0", who, j);
      err = msg;
      return false;
    }
    if (has_a && (!poses0 || !poses1)) { err = w + ": null argument"; return false; }
    const int mode = has_a ? MODE_NONE : job.fit;
    if (mode != MODE_NONE && mode != MODE_ROTATION && mode != MODE_RIGID) {
      snprintf(msg, sizeof msg, "%s: job %d: fit mode %d", who, j, mode);
      err = msg;
      return false;
    }
    if (mode == MODE_RIGID && job.inv_distance == 0.0) {
      snprintf(msg, sizeof msg, "%s: job %d: a rigid fit needs a finite distance", who, j);
      err = msg;
      return false;
    }
    int64_t n = 0;
    if (!plan_pixels(who, j, "", job.grid_w, job.grid_h, job.u0, job.v0, job.du, job.dv, job.n, job.uv, out.uv, out.queries[j], n, err))
      return false;
    out.first[j + 1] = out.first[j] + n;
    out.tile_first[j + 1] = out.tile_first[j] + (n + TILE - 1) / TILE;
    double* rec = out.recs.data() + (size_t)j * REC_STRIDE;
    for (int i = 0; i < CAM_STRIDE; ++i) {
      rec[REC_B0 + i] = plan[0].cam[(size_t)b * CAM_STRIDE + i];
      rec[REC_B1 + i] = plan[1].cam[(size_t)b * CAM_STRIDE + i];
    }
    rec[REC_RHO] = job.inv_distance;
    rec[REC_HAS_A] = has_a ? 1.0 : 0.0;
    rec[REC_MODE] = (double)mode;
    rec[REC_SAME] = a == b ? 1.0 : 0.0;
    if (has_a) {
      for (int i = 0; i < CAM_STRIDE; ++i) {
        rec[REC_A0 + i] = plan[0].cam[(size_t)a * CAM_STRIDE + i];
        rec[REC_A1 + i] = plan[1].cam[(size_t)a * CAM_STRIDE + i];
      }
      relative_pose(poses0, b, a, rec + REC_RT0);
      relative_pose(poses1, b, a, rec + REC_RT1);
      for (int i = 0; i < 24; ++i)
        if (!finite_arg(rec[REC_RT0 + i])) { snprintf(msg, sizeof msg, "%s: job %d: camera poses are not finite", who, j); err = msg; return false; }
    }
    fit_identity(out.fit.data() + (size_t)j * FIT_STRIDE);
    if (mode == MODE_NONE) continue;
    PixelSet set;
    int64_t nf = 0;
    if (!plan_pixels(who, j, "fit ", job.fit_grid_w, job.fit_grid_h, job.fit_u0, job.fit_v0, job.fit_du, job.fit_dv, job.fit_n,
                     job.fit_uv, out.uv, set, nf, err))
      return false;
    if (nf > MAX_FIT_PIXELS) {
      snprintf(msg, sizeof msg, "%s: job %d: fit grid of %lld pixels, at most %d are served", who, j, (long long)nf, MAX_FIT_PIXELS);
      err = msg;
      return false;
    }
    if (!finite_arg(job.focus_radius) || (job.focus_radius > 0.0 && (!finite_arg(job.focus_u) || !finite_arg(job.focus_v)))) {
      snprintf(msg, sizeof msg, "%s: job %d: the focus disc must be finite", who, j);
      err = msg;
      return false;
    }
    out.fit_jobs.push_back(j);
    out.fit_pixels.push_back(set);
    out.focus.push_back(Focus{job.focus_u, job.focus_v, job.focus_radius});
    out.ray_first.push_back(out.ray_first.back() + nf);
  }
  out.n_queries = out.first[n_jobs];
  if (out.n_queries > 0 && (!diff || !status)) { err = w + ": null argument"; return false; }
  return true;
}

// transform [n_jobs,6] and fit_info [n_jobs,5] (either may be null) from the fit records
inline void split_fit(const double* fit, int n_jobs, double* transform, double* fit_info) {
  for (int j = 0; j < n_jobs; ++j) {
    const double* f = fit + (size_t)j * FIT_STRIDE;
    if (transform)
      for (int i = 0; i < 6; ++i) transform[6 * (size_t)j + i] = f[i];
    if (fit_info)
      for (int i = 0; i < 5; ++i) fit_info[5 * (size_t)j + i] = f[FIT_NFIT + i];
  }
}

}  // namespace projdiff
}  // namespace mcba
