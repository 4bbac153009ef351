// TEST INFRASTRUCTURE: g++ build of the projection-uncertainty mathematics (multical_amd/csrc/mcba_uncertainty.h) behind the
// signature of mcba_projection_uncertainty, one plain loop over jobs and queries, and the row pair J of one query for the tests.
// The argument checks and the job records come from the same driver header the API uses.
#include <string>
#include <vector>

#include "../../multical_amd/csrc/mcba_uncertainty_driver.h"

using namespace mcba;
using namespace mcba::uncertainty;

static thread_local std::string g_error;

extern "C" {

const char* unh_last_error(void) { return g_error.c_str(); }

int32_t unh_projection_uncertainty(const mcba_camera_set* cams, const double* camera_poses, int32_t n_jobs,
                                   const mcba_uncertainty_job* jobs, double* cov, double* std, uint8_t* status) {
  Plan plan;
  if (!plan_jobs(cams, camera_poses, n_jobs, jobs, cov, status, plan, g_error)) return 1;
  for (int j = 0; j < n_jobs; ++j) {
    const double* rec = plan.recs.data() + (size_t)j * REC_STRIDE;
    const int64_t n = plan.first[j + 1] - plan.first[j];
    for (int64_t i = 0; i < n; ++i) {
      double u, v;
      if (plan.uv_first[j] < 0) {
        grid_pixel(i, plan.grid_w[j], plan.grid[4 * j], plan.grid[4 * j + 1], plan.grid[4 * j + 2], plan.grid[4 * j + 3], u, v);
      } else {
        u = plan.uv[2 * (size_t)(plan.uv_first[j] + i)];
        v = plan.uv[2 * (size_t)(plan.uv_first[j] + i) + 1];
      }
      Result r;
      query(rec, u, v, r);
      const size_t slot = (size_t)(plan.first[j] + i);
      cov[3 * slot] = r.uu; cov[3 * slot + 1] = r.uv; cov[3 * slot + 2] = r.vv;
      if (std) std[slot] = r.std;
      status[slot] = (uint8_t)r.status;
    }
  }
  return 0;
}

// J [2][job->K] of the query (u, v) of one job, in the row order of the job's W; *status: MCBA_UNC_* of the pieces
int32_t unh_query_rows(const mcba_camera_set* cams, const double* camera_poses, const mcba_uncertainty_job* job, double u, double v,
                       double* J, int32_t* status) {
  Plan plan;
  mcba_uncertainty_job one = *job;
  one.grid_w = 0; one.n = 0; one.uv = nullptr;
  if (!plan_jobs(cams, camera_poses, 1, &one, nullptr, nullptr, plan, g_error)) return 1;
  double Jp[2 * KP];
  *status = query_rows(plan.recs.data(), u, v, Jp);
  const bool has_a = job->reference >= 0;
  const int ki_b = has_a ? job->K - 12 - (int)plan.recs[REC_CAM_A + REC_ND] - 4 : job->K - 6;
  for (int k = 0; k < job->K; ++k) {
    const int col = record_column(k, ki_b, has_a);
    J[k] = Jp[col];
    J[job->K + k] = Jp[KP + col];
  }
  return 0;
}

}
