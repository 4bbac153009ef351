// TEST INFRASTRUCTURE: g++ build of the projection-difference mathematics (multical_amd/csrc/mcba_projdiff.h) behind the signature
// of mcba_projection_diff: the first pass, the fit through the header's SerialBackend and the map as plain loops over jobs, fit
// pixels and queries.  The argument checks and the job records come from the same driver header the API uses.  phd_fit_planted
// drives the header's fit function on targets of the caller's making.
#include <string>
#include <vector>

#include "../../multical_amd/csrc/mcba_projdiff_driver.h"

using namespace mcba;
using namespace mcba::projdiff;

static thread_local std::string g_error;

// the first pass of fitting job g of the plan
static std::vector<double> first_pass(const Plan& plan, size_t g) {
  const int j = plan.fit_jobs[g];
  const int64_t n = plan.ray_first[g + 1] - plan.ray_first[g];
  std::vector<double> rays((size_t)n * RAY_STRIDE + 1);
  for (int64_t i = 0; i < n; ++i) {
    double u, v;
    pixel_of(plan.fit_pixels[g], plan.uv.data(), i, u, v);
    fit_ray(plan.recs.data() + (size_t)j * REC_STRIDE, plan.focus[g], u, v, rays.data() + (size_t)i * RAY_STRIDE);
  }
  return rays;
}

extern "C" {

const char* phd_last_error(void) { return g_error.c_str(); }

int32_t phd_projection_diff(const mcba_camera_set* cams0, const double* poses0, const mcba_camera_set* cams1, const double* poses1,
                            int32_t n_jobs, const mcba_projdiff_job* jobs, double* transform, double* fit_info, double* diff,
                            double* magnitude, double* landing, uint8_t* status) {
  Plan plan;
  if (!plan_jobs(cams0, poses0, cams1, poses1, n_jobs, jobs, diff, status, plan, g_error)) return 1;
  if (plan.n_queries > 0) {
    for (size_t g = 0; g < plan.fit_jobs.size(); ++g) {
      const int j = plan.fit_jobs[g];
      const std::vector<double> rays = first_pass(plan, g);
      fit_job(plan.recs.data() + (size_t)j * REC_STRIDE, rays.data(), (int)(plan.ray_first[g + 1] - plan.ray_first[g]),
              plan.fit.data() + (size_t)j * FIT_STRIDE);
    }
  }
  split_fit(plan.fit.data(), n_jobs, transform, fit_info);
  for (int j = 0; j < n_jobs; ++j) {
    const double* rec = plan.recs.data() + (size_t)j * REC_STRIDE;
    double xf[XF_STRIDE];
    stage_transform(rec, plan.fit.data() + (size_t)j * FIT_STRIDE, xf);
    const int64_t n = plan.first[j + 1] - plan.first[j];
    for (int64_t i = 0; i < n; ++i) {
      double u, v;
      pixel_of(plan.queries[j], plan.uv.data(), i, u, v);
      Result r;
      query(rec, xf, u, v, r);
      const size_t slot = (size_t)(plan.first[j] + i);
      diff[2 * slot] = r.du; diff[2 * slot + 1] = r.dv;
      if (magnitude) magnitude[slot] = r.mag;
      if (landing) { landing[2 * slot] = r.lu; landing[2 * slot + 1] = r.lv; }
      status[slot] = (uint8_t)r.status;
    }
  }
  return 0;
}

// The header's fit function on planted targets: the fit pixels of `job` (one intrinsics job that fits) keep their rays under
// calibration 0, and the pixel each is compared with becomes project_b^1(R(omega*) n + rho tau*), planted = omega* | tau*.
// fit [FIT_STRIDE]: the fit record; valid [n_fit_pixels] (or null): which fit pixels took part.
int32_t phd_fit_planted(const mcba_camera_set* cams0, const mcba_camera_set* cams1, const mcba_projdiff_job* job, const double* planted,
                        double* fit, uint8_t* valid) {
  Plan plan;
  mcba_projdiff_job one = *job;
  one.grid_w = 0; one.n = 0; one.uv = nullptr;
  if (!plan_jobs(cams0, nullptr, cams1, nullptr, 1, &one, nullptr, nullptr, plan, g_error)) return 1;
  if (plan.fit_jobs.empty()) { g_error = "phd_fit_planted: the job does not fit"; return 1; }
  std::vector<double> rays = first_pass(plan, 0);
  const int n = (int)plan.ray_first[1];
  const double* rec = plan.recs.data();
  double pe[POSE_STRIDE];
  pose_entry(planted, pe);
  for (int i = 0; i < n; ++i) {
    double* ray = rays.data() + (size_t)i * RAY_STRIDE;
    if (valid) valid[i] = ray[RAY_OK] != 0.0 ? 1 : 0;
    if (ray[RAY_OK] == 0.0) continue;
    double X[3], uv[2];
    mat3_vec(pe + POSE_R, ray + RAY_N, X);
    for (int k = 0; k < 3; ++k) X[k] += rec[REC_RHO] * pe[POSE_T + k];
    const double* cam = rec + REC_B1;
    undistort::project_any(cam, (int)cam[REC_ND], cam[CAM_ISFISH] != 0.0, X, uv);
    ray[RAY_UV] = uv[0];
    ray[RAY_UV + 1] = uv[1];
  }
  fit_job(rec, rays.data(), n, fit);
  return 0;
}

}
