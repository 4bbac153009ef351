// translation unit of k_reconstruction_uncertainty and k_reconstruction_pairs (mcba_recon_kernels.h) and the host drivers of
// mcba_reconstruction_uncertainty and mcba_reconstruction_pairs
#include "mcba_host.h"
#include "mcba_recon_driver.h"
#include "mcba_recon_kernels.h"

namespace mcba {
namespace recon {

void recon_launch(const KernelArgs& a, long long tiles, int max_group, hipStream_t st) {
  if (tiles <= 0) return;
  const int grid = host::capped_grid(tiles, RC_MAX_GRID);
  if (max_group <= 4) hipLaunchKernelGGL(k_reconstruction_uncertainty<4>, dim3(grid), dim3(RC_THREADS), 0, st, a);
  else hipLaunchKernelGGL(k_reconstruction_uncertainty<8>, dim3(grid), dim3(RC_THREADS), 0, st, a);
}

void recon_pairs_launch(const PairKernelArgs& a, long long tiles, int max_group, hipStream_t st) {
  if (tiles <= 0) return;
  const int grid = host::capped_grid(tiles, RC_MAX_GRID);
  if (max_group <= 4) hipLaunchKernelGGL(k_reconstruction_pairs<4>, dim3(grid), dim3(RC_THREADS), 0, st, a);
  else hipLaunchKernelGGL(k_reconstruction_pairs<8>, dim3(grid), dim3(RC_THREADS), 0, st, a);
}

}  // namespace recon
}  // namespace mcba

using namespace mcba;
using namespace mcba::host;

static_assert(recon::TILE == recon::RC_TILE && recon::PAIR_TILE == recon::RP_TILE, "a tile of the plan is what a wavefront serves");
static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(unsigned long long) == sizeof(uint64_t), "the tables are uploaded as planned");

// uploads | event-timed kernel | downloads | whole call; points launched
MCBA_TIMING_GETTER(mcba_debug_reconstruction_uncertainty_ms, g_recon_timing, 4)
// the same slots; pairs launched
MCBA_TIMING_GETTER(mcba_debug_reconstruction_pairs_ms, g_recon_pairs_timing, 4)

extern "C" {

namespace {
void run_recon(const mcba_camera_set* cams, const double* camera_poses, int32_t n_jobs, const mcba_recon_job* jobs, const double* points,
               const uint64_t* masks, double sigma2, double margin, double* cov_cal, double* cov_noise, int32_t* n_views,
               uint64_t* views, uint8_t* status) {
  DeviceCall call(g_recon_timing);   // (before the buffers: see the type)
  call.tm.reset();
  recon::Plan plan;
  std::string msg;
  if (!recon::plan_jobs(cams, camera_poses, n_jobs, jobs, points, sigma2, margin, cov_cal, cov_noise, n_views, views, status, plan, msg))
    throw Error(msg);
  if (plan.n_points == 0) return;    // nothing is launched, the device is not touched
  const size_t N = (size_t)plan.n_points;
  DevBuf<double> d_recs, d_w, d_points, d_cal, d_noise;
  DevBuf<int64_t> d_w_first, d_first, d_tile_first;
  DevBuf<uint64_t> d_masks, d_views;
  DevBuf<int32_t> d_n;
  DevBuf<uint8_t> d_status;
  call.open(2);
  upload_vector(d_recs, plan.recs, call.st);
  upload_vector(d_w, plan.wdev, call.st);
  upload_vector(d_w_first, plan.w_first, call.st);
  upload_vector(d_first, plan.first, call.st);
  upload_vector(d_tile_first, plan.tile_first, call.st);
  upload_async(d_points, points, N * 3, call.st);
  if (masks) upload_async(d_masks, masks, N, call.st);
  d_cal.alloc(N * 6, false);
  d_noise.alloc(N * 6, false);
  d_n.alloc(N, false);
  d_views.alloc(N, false);
  d_status.alloc(N, false);
  recon::KernelArgs a{};
  a.n_jobs = n_jobs;
  a.recs = d_recs.p;
  a.wdev = d_w.p;
  a.w_first = (const long long*)d_w_first.p;
  a.first = (const long long*)d_first.p;
  a.tile_first = (const long long*)d_tile_first.p;
  a.points = d_points.p;
  a.masks = masks ? (const unsigned long long*)d_masks.p : nullptr;
  a.sigma2 = sigma2;
  a.cov_cal = d_cal.p;
  a.cov_noise = d_noise.p;
  a.n_views = d_n.p;
  a.views = (unsigned long long*)d_views.p;
  a.status = d_status.p;
  call.mark(0);
  recon::recon_launch(a, (long long)plan.tile_first[n_jobs], plan.max_group, call.st);
  call.mark(1);
  call.end_kernels("k_reconstruction_uncertainty");
  download_async(cov_cal, d_cal.p, N * 6, call.st);
  download_async(cov_noise, d_noise.p, N * 6, call.st);
  download_async(n_views, d_n.p, N, call.st);
  download_async(views, d_views.p, N, call.st);
  download_async(status, d_status.p, N, call.st);
  call.finish(plan.n_points);
}

void run_recon_pairs(const mcba_camera_set* cams, const double* camera_poses, int32_t n_jobs, const mcba_recon_job* jobs,
                     const double* points, const uint64_t* masks, const int64_t* n_pairs, const int64_t* pairs, double sigma2,
                     double margin, double* cov_diff_cal, double* cross_cal, double* cov_diff_noise, double* length,
                     double* length_var_cal, double* length_var_noise, uint64_t* views_a, uint64_t* views_b, uint8_t* status) {
  DeviceCall call(g_recon_pairs_timing);   // (before the buffers: see the type)
  call.tm.reset();
  recon::PairPlan plan;
  std::string msg;
  if (!recon::plan_pairs(cams, camera_poses, n_jobs, jobs, points, n_pairs, pairs, sigma2, margin, plan, msg)) throw Error(msg);
  if (plan.n_pairs == 0) return;           // nothing is launched, the device is not touched
  const size_t N = (size_t)plan.jobs.n_points, K = (size_t)plan.n_pairs;
  DevBuf<double> d_recs, d_w, d_points;
  DevBuf<int64_t> d_w_first, d_first, d_pair_first, d_tile_first, d_pairs;
  DevBuf<uint64_t> d_masks;
  call.open(2);
  upload_vector(d_recs, plan.jobs.recs, call.st);
  upload_vector(d_w, plan.jobs.wdev, call.st);
  upload_vector(d_w_first, plan.jobs.w_first, call.st);
  upload_vector(d_first, plan.jobs.first, call.st);
  upload_vector(d_pair_first, plan.pair_first, call.st);
  upload_vector(d_tile_first, plan.tile_first, call.st);
  upload_async(d_points, points, N * 3, call.st);
  if (masks) upload_async(d_masks, masks, N, call.st);
  upload_async(d_pairs, pairs, K * 2, call.st);
  OutBuf<double> o_cal(cov_diff_cal, K * 6), o_cross(cross_cal, K * 9), o_noise(cov_diff_noise, K * 6), o_length(length, K),
      o_var_cal(length_var_cal, K), o_var_noise(length_var_noise, K);
  OutBuf<uint64_t> o_views_a(views_a, K), o_views_b(views_b, K);
  OutBuf<uint8_t> o_status(status, K);
  recon::PairKernelArgs a{};
  a.n_jobs = n_jobs;
  a.recs = d_recs.p;
  a.wdev = d_w.p;
  a.w_first = (const long long*)d_w_first.p;
  a.first = (const long long*)d_first.p;
  a.pair_first = (const long long*)d_pair_first.p;
  a.tile_first = (const long long*)d_tile_first.p;
  a.points = d_points.p;
  a.masks = masks ? (const unsigned long long*)d_masks.p : nullptr;
  a.pairs = (const long long*)d_pairs.p;
  a.sigma2 = sigma2;
  a.cov_diff_cal = o_cal.dev();
  a.cross_cal = o_cross.dev();
  a.cov_diff_noise = o_noise.dev();
  a.length = o_length.dev();
  a.length_var_cal = o_var_cal.dev();
  a.length_var_noise = o_var_noise.dev();
  a.views_a = (unsigned long long*)o_views_a.dev();
  a.views_b = (unsigned long long*)o_views_b.dev();
  a.status = o_status.dev();
  call.mark(0);
  recon::recon_pairs_launch(a, (long long)plan.tile_first[n_jobs], plan.max_group, call.st);
  call.mark(1);
  call.end_kernels("k_reconstruction_pairs");
  o_cal.fetch(call.st);
  o_cross.fetch(call.st);
  o_noise.fetch(call.st);
  o_length.fetch(call.st);
  o_var_cal.fetch(call.st);
  o_var_noise.fetch(call.st);
  o_views_a.fetch(call.st);
  o_views_b.fetch(call.st);
  o_status.fetch(call.st);
  call.finish(plan.n_pairs);
}
}  // namespace

int32_t mcba_reconstruction_pairs(const mcba_camera_set* cams, const double* camera_poses, int32_t n_jobs, const mcba_recon_job* jobs,
                                  const double* points, const uint64_t* masks, const int64_t* n_pairs, const int64_t* pairs,
                                  double sigma2, double margin, double* cov_diff_cal, double* cross_cal, double* cov_diff_noise,
                                  double* length, double* length_var_cal, double* length_var_noise, uint64_t* views_a,
                                  uint64_t* views_b, uint8_t* status) {
  API_BEGIN
  run_recon_pairs(cams, camera_poses, n_jobs, jobs, points, masks, n_pairs, pairs, sigma2, margin, cov_diff_cal, cross_cal,
                  cov_diff_noise, length, length_var_cal, length_var_noise, views_a, views_b, status);
  API_END
}

int32_t mcba_reconstruction_uncertainty(const mcba_camera_set* cams, const double* camera_poses, int32_t n_jobs,
                                        const mcba_recon_job* jobs, const double* points, const uint64_t* masks, double sigma2,
                                        double margin, double* cov_cal, double* cov_noise, int32_t* n_views, uint64_t* views,
                                        uint8_t* status) {
  API_BEGIN
  run_recon(cams, camera_poses, n_jobs, jobs, points, masks, sigma2, margin, cov_cal, cov_noise, n_views, views, status);
  API_END
}

}  // extern "C"
