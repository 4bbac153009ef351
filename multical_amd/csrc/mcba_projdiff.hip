// translation unit of k_projdiff_fit and k_projdiff_map (mcba_projdiff_kernels.h) and the host driver of mcba_projection_diff
#include "mcba_host.h"
#include "mcba_projdiff_driver.h"
#include "mcba_projdiff_kernels.h"

namespace mcba {
namespace projdiff {

hipError_t fit_launch(const FitArgs& a, int n_fit_jobs, hipStream_t st) {
  if (n_fit_jobs <= 0) return hipSuccess;
  const size_t bytes = fit_lds_bytes();      // 82 KiB: above the default limit of a launch
  const hipError_t e = hipFuncSetAttribute((const void*)k_projdiff_fit, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_projdiff_fit, dim3(n_fit_jobs), dim3(PD_THREADS), bytes, st, a);
  return hipGetLastError();
}

void map_launch(const MapArgs& a, long long tiles, hipStream_t st) {
  if (tiles <= 0) return;
  const int grid = host::capped_grid(tiles, PD_MAX_GRID);
  hipLaunchKernelGGL(k_projdiff_map, dim3(grid), dim3(PD_THREADS), 0, st, a);
}

}  // namespace projdiff
}  // namespace mcba

using namespace mcba;
using namespace mcba::host;

static_assert(projdiff::TILE == projdiff::PD_THREADS, "a tile of the plan is what a workgroup serves");
static_assert(sizeof(long long) == sizeof(int64_t), "the job tables are uploaded as they are planned");

// uploads | fit kernel | map kernel (HIP events) | downloads | whole call; queries launched
MCBA_TIMING_GETTER(mcba_debug_projection_diff_ms, g_projdiff_timing, 5)

extern "C" {

namespace {
void run_projdiff(const mcba_camera_set* cams0, const double* poses0, const mcba_camera_set* cams1, const double* poses1,
                  int32_t n_jobs, const mcba_projdiff_job* jobs, double* transform, double* fit_info, double* diff, double* magnitude,
                  double* landing, uint8_t* status) {
  DeviceCall call(g_projdiff_timing);   // (before the buffers: see the type)
  call.tm.reset();
  projdiff::Plan plan;
  std::string msg;
  if (!projdiff::plan_jobs(cams0, poses0, cams1, poses1, n_jobs, jobs, diff, status, plan, msg)) throw Error(msg);
  if (plan.n_queries == 0) {               // nothing is launched, the device is not touched: the records of jobs without a fit
    projdiff::split_fit(plan.fit.data(), n_jobs, transform, fit_info);
    return;
  }
  const size_t N = (size_t)plan.n_queries, n_fit_jobs = plan.fit_jobs.size();
  const size_t n_rays = (size_t)plan.ray_first.back();
  DevBuf<double> d_recs, d_fit, d_uv, d_rays, d_diff;
  DevBuf<int64_t> d_first, d_tile_first, d_ray_first;
  DevBuf<int32_t> d_fit_jobs;
  DevBuf<projdiff::PixelSet> d_queries, d_fit_pixels;
  DevBuf<projdiff::Focus> d_focus;
  DevBuf<uint8_t> d_status;
  call.open(3);
  const hipStream_t st = call.st;
  upload_vector(d_recs, plan.recs, st);
  upload_vector(d_fit, plan.fit, st);
  upload_vector(d_first, plan.first, st);
  upload_vector(d_tile_first, plan.tile_first, st);
  upload_vector(d_queries, plan.queries, st);
  upload_vector(d_uv, plan.uv, st);
  if (n_fit_jobs > 0) {
    upload_vector(d_fit_jobs, plan.fit_jobs, st);
    upload_vector(d_ray_first, plan.ray_first, st);
    upload_vector(d_fit_pixels, plan.fit_pixels, st);
    upload_vector(d_focus, plan.focus, st);
    d_rays.alloc(n_rays * projdiff::RAY_STRIDE, false);
  }
  d_diff.alloc(N * 2, false);
  d_status.alloc(N, false);
  OutBuf<double> o_mag(magnitude, N), o_landing(landing, N * 2);
  call.mark(0);
  if (n_fit_jobs > 0) {
    projdiff::FitArgs f{};
    f.recs = d_recs.p;
    f.fit_jobs = d_fit_jobs.p;
    f.ray_first = (const long long*)d_ray_first.p;
    f.fit_pixels = d_fit_pixels.p;
    f.focus = d_focus.p;
    f.uv = d_uv.p;
    f.rays = d_rays.p;
    f.fit = d_fit.p;
    const hipError_t e = projdiff::fit_launch(f, (int)n_fit_jobs, st);
    if (e != hipSuccess) throw Error(std::string("kernel launch failed (k_projdiff_fit): ") + hipGetErrorString(e));
  }
  call.mark(1);
  projdiff::MapArgs a{};
  a.n_jobs = n_jobs;
  a.recs = d_recs.p;
  a.fit = d_fit.p;
  a.first = (const long long*)d_first.p;
  a.tile_first = (const long long*)d_tile_first.p;
  a.queries = d_queries.p;
  a.uv = d_uv.p;
  a.diff = d_diff.p;
  a.magnitude = o_mag.dev();
  a.landing = o_landing.dev();
  a.status = d_status.p;
  projdiff::map_launch(a, (long long)plan.tile_first[n_jobs], st);
  call.mark(2);
  call.end_kernels("k_projdiff_map");
  std::vector<double> fit(plan.fit.size());
  download_async(fit.data(), d_fit.p, fit.size(), st);
  download_async(diff, d_diff.p, N * 2, st);
  download_async(status, d_status.p, N, st);
  o_mag.fetch(st);
  o_landing.fetch(st);
  HIP_OK(hipStreamSynchronize(st));
  projdiff::split_fit(fit.data(), n_jobs, transform, fit_info);
  call.finish(plan.n_queries);
}
}  // namespace

int32_t mcba_projection_diff(const mcba_camera_set* cams0, const double* poses0, const mcba_camera_set* cams1, const double* poses1,
                             int32_t n_jobs, const mcba_projdiff_job* jobs, double* transform, double* fit_info, double* diff,
                             double* magnitude, double* landing, uint8_t* status) {
  API_BEGIN
  run_projdiff(cams0, poses0, cams1, poses1, n_jobs, jobs, transform, fit_info, diff, magnitude, landing, status);
  API_END
}

}  // extern "C"
