// TEST INFRASTRUCTURE: g++ build of the pair mathematics of multical_amd/csrc/mcba_recon.h (pair_query) behind the signature of
// mcba_reconstruction_pairs, one plain loop over jobs and pairs.  The argument checks, the job records and the pair tables come from
// the same driver header the API uses, so that both refuse the same calls with the same messages.
#include <string>
#include <vector>

#include "../../multical_amd/csrc/mcba_recon_driver.h"

using namespace mcba;
using namespace mcba::recon;

static thread_local std::string g_error;

extern "C" {

const char* lph_last_error(void) { return g_error.c_str(); }

int32_t lph_reconstruction_pairs(const mcba_camera_set* cams, const double* camera_poses, int32_t n_jobs, const mcba_recon_job* jobs,
                                 const double* points, const uint64_t* masks, const int64_t* n_pairs, const int64_t* pairs,
                                 double sigma2, double margin, double* cov_diff_cal, double* cross_cal, double* cov_diff_noise,
                                 double* length, double* length_var_cal, double* length_var_noise, uint64_t* views_a,
                                 uint64_t* views_b, uint8_t* status) {
  PairPlan plan;
  if (!plan_pairs(cams, camera_poses, n_jobs, jobs, points, n_pairs, pairs, sigma2, margin, plan, g_error)) return 1;
  for (int j = 0; j < n_jobs; ++j) {
    const double* rec = plan.jobs.recs.data() + (size_t)j * JR_STRIDE;
    const double* Wj = plan.jobs.wdev.data() + plan.jobs.w_first[j];
    for (int64_t k = plan.pair_first[j]; k < plan.pair_first[j + 1]; ++k) {
      const int64_t a = plan.jobs.first[j] + pairs[2 * k], b = plan.jobs.first[j] + pairs[2 * k + 1];
      PairResult r;
      pair_query(rec, Wj, points + 3 * a, points + 3 * b, masks ? masks[a] : ~(uint64_t)0, masks ? masks[b] : ~(uint64_t)0, a == b, sigma2, r);
      for (int i = 0; i < 6; ++i) {
        if (cov_diff_cal) cov_diff_cal[6 * k + i] = r.cov_diff_cal[i];
        if (cov_diff_noise) cov_diff_noise[6 * k + i] = r.cov_diff_noise[i];
      }
      for (int i = 0; i < 9; ++i)
        if (cross_cal) cross_cal[9 * k + i] = r.cross_cal[i];
      if (length) length[k] = r.length;
      if (length_var_cal) length_var_cal[k] = r.length_var_cal;
      if (length_var_noise) length_var_noise[k] = r.length_var_noise;
      if (views_a) views_a[k] = r.views_a;
      if (views_b) views_b[k] = r.views_b;
      if (status) status[k] = (uint8_t)r.status;
    }
  }
  return 0;
}

}
