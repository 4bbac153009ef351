// translation unit of k_reconstruction_uncertainty (mcba_recon_kernels.h) and the host driver of mcba_reconstruction_uncertainty
#include "mcba_host.h"
#include "mcba_recon_driver.h"
#include "mcba_recon_kernels.h"

namespace mcba {
namespace recon {

void recon_launch(const KernelArgs& a, long long tiles, int max_group, hipStream_t st) {
  if (tiles <= 0) return;
  const int grid = (int)(tiles > RC_MAX_GRID ? RC_MAX_GRID : tiles);
  if (max_group <= 4) hipLaunchKernelGGL(k_reconstruction_uncertainty<4>, dim3(grid), dim3(RC_THREADS), 0, st, a);
  else hipLaunchKernelGGL(k_reconstruction_uncertainty<8>, dim3(grid), dim3(RC_THREADS), 0, st, a);
}

}  // namespace recon
}  // namespace mcba

using namespace mcba;
using namespace mcba::host;

static_assert(recon::TILE == recon::RC_TILE, "a tile of the plan is what a wavefront serves");
static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(unsigned long long) == sizeof(uint64_t), "the tables are uploaded as planned");

// uploads | event-timed kernel | downloads | whole call; points launched
MCBA_TIMING_GETTER(mcba_debug_reconstruction_uncertainty_ms, g_recon_timing, 4)

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
}  // namespace

int32_t mcba_reconstruction_uncertainty(const mcba_camera_set* cams, const double* camera_poses, int32_t n_jobs,
                                        const mcba_recon_job* jobs, const double* points, const uint64_t* masks, double sigma2,
                                        double margin, double* cov_cal, double* cov_noise, int32_t* n_views, uint64_t* views,
                                        uint8_t* status) {
  API_BEGIN
  run_recon(cams, camera_poses, n_jobs, jobs, points, masks, sigma2, margin, cov_cal, cov_noise, n_views, views, status);
  API_END
}

}  // extern "C"
