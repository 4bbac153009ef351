// translation unit of k_projection_uncertainty (mcba_uncertainty_kernels.h) and the host driver of mcba_projection_uncertainty
#include "mcba_host.h"
#include "mcba_uncertainty_driver.h"
#include "mcba_uncertainty_kernels.h"

namespace mcba {
namespace uncertainty {

void uncertainty_launch(const KernelArgs& a, long long tiles, hipStream_t st) {
  if (tiles <= 0) return;
  const int grid = host::capped_grid(tiles, UNC_MAX_GRID);
  hipLaunchKernelGGL(k_projection_uncertainty, dim3(grid), dim3(UNC_THREADS), 0, st, a);
}

}  // namespace uncertainty
}  // namespace mcba

using namespace mcba;
using namespace mcba::host;

static_assert(uncertainty::TILE == uncertainty::UNC_THREADS, "a tile of the plan is what a workgroup serves");
static_assert(sizeof(long long) == sizeof(int64_t), "the job tables are uploaded as they are planned");

// uploads | event-timed kernel | downloads | whole call; queries launched
MCBA_TIMING_GETTER(mcba_debug_projection_uncertainty_ms, g_uncertainty_timing, 4)

extern "C" {

namespace {
void run_uncertainty(const mcba_camera_set* cams, const double* camera_poses, int32_t n_jobs, const mcba_uncertainty_job* jobs,
                     double* cov, double* std, uint8_t* status) {
  DeviceCall call(g_uncertainty_timing);   // (before the buffers: see the type)
  call.tm.reset();
  uncertainty::Plan plan;
  std::string msg;
  if (!uncertainty::plan_jobs(cams, camera_poses, n_jobs, jobs, cov, status, plan, msg)) throw Error(msg);
  if (plan.n_queries == 0) return;         // nothing is launched, the device is not touched
  const size_t N = (size_t)plan.n_queries;
  DevBuf<double> d_recs, d_grid, d_uv, d_cov;
  DevBuf<int64_t> d_first, d_tile_first, d_uv_first;
  DevBuf<int32_t> d_grid_w;
  DevBuf<uint8_t> d_status;
  call.open(2);
  upload_vector(d_recs, plan.recs, call.st);
  upload_vector(d_first, plan.first, call.st);
  upload_vector(d_tile_first, plan.tile_first, call.st);
  upload_vector(d_uv_first, plan.uv_first, call.st);
  upload_vector(d_grid, plan.grid, call.st);
  upload_vector(d_grid_w, plan.grid_w, call.st);
  upload_vector(d_uv, plan.uv, call.st);
  d_cov.alloc(N * 3, false);
  d_status.alloc(N, false);
  OutBuf<double> o_std(std, N);
  uncertainty::KernelArgs a{};
  a.n_jobs = n_jobs;
  a.recs = d_recs.p;
  a.first = (const long long*)d_first.p;
  a.tile_first = (const long long*)d_tile_first.p;
  a.uv_first = (const long long*)d_uv_first.p;
  a.grid = d_grid.p;
  a.grid_w = d_grid_w.p;
  a.uv = d_uv.p;
  a.cov = d_cov.p;
  a.std = o_std.dev();
  a.status = d_status.p;
  call.mark(0);
  uncertainty::uncertainty_launch(a, (long long)plan.tile_first[n_jobs], call.st);
  call.mark(1);
  call.end_kernels("k_projection_uncertainty");
  download_async(cov, d_cov.p, N * 3, call.st);
  download_async(status, d_status.p, N, call.st);
  o_std.fetch(call.st);
  call.finish(plan.n_queries);
}
}  // namespace

int32_t mcba_projection_uncertainty(const mcba_camera_set* cams, const double* camera_poses, int32_t n_jobs,
                                    const mcba_uncertainty_job* jobs, double* cov, double* std, uint8_t* status) {
  API_BEGIN
  run_uncertainty(cams, camera_poses, n_jobs, jobs, cov, std, status);
  API_END
}

}  // extern "C"
