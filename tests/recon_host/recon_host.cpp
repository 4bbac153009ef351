// TEST INFRASTRUCTURE: g++ build of the reconstruction-uncertainty mathematics (multical_amd/csrc/mcba_recon.h) behind the signature
// of mcba_reconstruction_uncertainty, one plain loop over jobs and points, and the rows G = -H^-1 [B_1 .. B_G] of one point for the
// tests.  The argument checks and the job records come from the same driver header the API uses.
#include <string>
#include <vector>

#include "../../multical_amd/csrc/mcba_recon_driver.h"

using namespace mcba;
using namespace mcba::recon;

static thread_local std::string g_error;

extern "C" {

const char* rch_last_error(void) { return g_error.c_str(); }

int32_t rch_reconstruction_uncertainty(const mcba_camera_set* cams, const double* camera_poses, int32_t n_jobs, const mcba_recon_job* jobs,
                                       const double* points, const uint64_t* masks, double sigma2, double margin, double* cov_cal,
                                       double* cov_noise, int32_t* n_views, uint64_t* views, uint8_t* status) {
  Plan plan;
  if (!plan_jobs(cams, camera_poses, n_jobs, jobs, points, sigma2, margin, cov_cal, cov_noise, n_views, views, status, plan, g_error))
    return 1;
  for (int j = 0; j < n_jobs; ++j) {
    const double* rec = plan.recs.data() + (size_t)j * JR_STRIDE;
    const double* Wj = plan.wdev.data() + plan.w_first[j];
    for (int64_t at = plan.first[j]; at < plan.first[j + 1]; ++at) {
      Result r;
      query(rec, Wj, points + 3 * at, masks ? masks[at] : ~(uint64_t)0, sigma2, r);
      for (int i = 0; i < 6; ++i) { cov_cal[6 * at + i] = r.cov_cal[i]; cov_noise[6 * at + i] = r.cov_noise[i]; }
      n_views[at] = r.n_views;
      views[at] = r.views;
      status[at] = (uint8_t)r.status;
    }
  }
  return 0;
}

// G [3][24 job->G] of the point X of one job (the columns of slot s at 24 s); *status: MCBA_RECON_*
int32_t rch_query_rows(const mcba_camera_set* cams, const double* camera_poses, const mcba_recon_job* job, const double* X, uint64_t mask,
                       double margin, double* Gm, int32_t* status) {
  Plan plan;
  mcba_recon_job one = *job;
  one.n = 0; one.r = 0;
  if (!plan_jobs(cams, camera_poses, 1, &one, nullptr, 1.0, margin, nullptr, nullptr, nullptr, nullptr, nullptr, plan, g_error)) return 1;
  *status = query_rows(plan.recs.data(), X, mask, Gm);
  return 0;
}

}
