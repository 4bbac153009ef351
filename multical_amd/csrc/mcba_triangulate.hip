// translation unit of k_triangulate (mcba_triangulate_kernels.h) and the host driver of mcba_triangulate
#include "mcba_host.h"
#include "mcba_triangulate_driver.h"
#include "mcba_triangulate_kernels.h"

namespace mcba {
namespace triangulate {

void triangulate_launch(const KernelArgs& a, hipStream_t st) {
  const long long rounds = (long long)a.t.F * ((a.M + TRI_THREADS - 1) / TRI_THREADS);
  if (rounds <= 0) return;
  const int grid = host::capped_grid(rounds, TRI_MAX_GRID);
  hipLaunchKernelGGL(k_triangulate, dim3(grid), dim3(TRI_THREADS), lds_bytes(a.t.C), st, a);
}

}  // namespace triangulate
}  // namespace mcba

using namespace mcba;
using namespace mcba::host;

// uploads | event-timed kernel | downloads | whole call; points launched
MCBA_TIMING_GETTER(mcba_debug_triangulate_ms, g_triangulate_timing, 4)

extern "C" {

namespace {
void run_triangulate(const mcba_triangulate_problem* p, double* X, double* cov, double* sse, double* err, int32_t* n_views,
                     uint8_t* status) {
  DeviceCall call(g_triangulate_timing);   // (before the buffers: see the type)
  call.tm.reset();
  std::vector<double> cam;
  std::string msg;
  int64_t n_points = 0;
  if (!triangulate::plan_problem(p, X, status, cam, &n_points, msg)) throw Error(msg);
  if (n_points == 0) return;             // nothing is launched, the device is not touched
  const size_t C = (size_t)p->cams.C, F = (size_t)p->F, N = (size_t)n_points;
  DevBuf<double> d_cam, d_views, d_end, d_points, d_X;
  DevBuf<uint8_t> d_view_valid, d_valid, d_status;
  call.open(2);
  triangulate::KernelArgs a{};
  upload_async(d_cam, cam.data(), cam.size(), call.st);
  upload_async(d_views, p->views, C * F * 12, call.st);
  if (p->views_end) upload_async(d_end, p->views_end, C * F * 12, call.st);
  if (p->view_valid) upload_async(d_view_valid, p->view_valid, C * F, call.st);
  upload_async(d_points, p->points, C * N * 2, call.st);
  upload_async(d_valid, p->valid, C * N, call.st);
  d_X.alloc(N * 3, false);
  d_status.alloc(N, false);
  OutBuf<double> o_cov(cov, N * 6), o_sse(sse, N), o_err(err, C * N);
  OutBuf<int32_t> o_n(n_views, N);
  a.t.C = p->cams.C; a.t.F = p->F;
  a.t.cam = d_cam.p; a.t.views = d_views.p;
  a.t.views_end = p->views_end ? d_end.p : nullptr;
  a.t.view_valid = p->view_valid ? d_view_valid.p : nullptr;
  a.M = p->M;
  a.points = d_points.p; a.valid = d_valid.p;
  a.rolling = p->views_end ? 1 : 0;
  a.sigma_px = p->sigma_px;
  a.max_iter = triangulate::clamp_iterations(p->max_iterations);
  a.X = d_X.p; a.status = d_status.p;
  a.cov = o_cov.dev(); a.sse = o_sse.dev(); a.err = o_err.dev(); a.n_views = o_n.dev();
  call.mark(0);
  triangulate::triangulate_launch(a, call.st);
  call.mark(1);
  call.end_kernels("k_triangulate");
  download_async(X, d_X.p, N * 3, call.st);
  download_async(status, d_status.p, N, call.st);
  o_cov.fetch(call.st);
  o_sse.fetch(call.st);
  o_err.fetch(call.st);
  o_n.fetch(call.st);
  call.finish(n_points);
}
}  // namespace

int32_t mcba_triangulate(const mcba_triangulate_problem* p, double* X, double* cov, double* sse, double* err, int32_t* n_views,
                         uint8_t* status) {
  API_BEGIN
  run_triangulate(p, X, cov, sse, err, n_views, status);
  API_END
}

}  // extern "C"
