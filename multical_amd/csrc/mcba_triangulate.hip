// translation unit of k_triangulate (mcba_triangulate_kernels.h) and the host driver of mcba_triangulate
#include "mcba_host.h"
#include "mcba_triangulate_driver.h"
#include "mcba_triangulate_kernels.h"

namespace mcba {
namespace triangulate {

void triangulate_launch(const KernelArgs& a, hipStream_t st) {
  const long long rounds = (long long)a.t.F * ((a.M + TRI_THREADS - 1) / TRI_THREADS);
  if (rounds <= 0) return;
  const int grid = (int)(rounds > TRI_MAX_GRID ? TRI_MAX_GRID : rounds);
  hipLaunchKernelGGL(k_triangulate, dim3(grid), dim3(TRI_THREADS), lds_bytes(a.t.C), st, a);
}

}  // namespace triangulate
}  // namespace mcba

using namespace mcba;
using namespace mcba::host;

namespace {
template <class T>
void download_async(T* host, const DevBuf<T>& d, size_t n, hipStream_t st) {
  HIP_OK(hipMemcpyAsync(host, d.p, n * sizeof(T), hipMemcpyDeviceToHost, st));
}
}  // namespace

extern "C" {

namespace {
thread_local CallTiming g_triangulate_timing;   // uploads | event-timed kernel | downloads | whole call; points launched

// the scaffold plus the two events around the kernel (members: they go before the DeviceCall they derive from does)
struct TriangulateCall : DeviceCall {
  double t_up = 0.0;
  hipEvent_t ev[2] = {nullptr, nullptr};

  TriangulateCall() : DeviceCall(g_triangulate_timing) { tm.reset(); }
  void open() {
    DeviceCall::open();
    HIP_OK(hipEventCreate(&ev[0]));
    HIP_OK(hipEventCreate(&ev[1]));
    t_up = now_seconds();
  }
  ~TriangulateCall() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  void begin_kernel() {      // uploads are complete; the kernel runs between the two events
    HIP_OK(hipStreamSynchronize(st));
    tm.ms[0] = (now_seconds() - t_up) * 1e3;
    HIP_OK(hipEventRecord(ev[0], st));
  }
  double end_kernel(const char* what) {
    check_launch(what);
    HIP_OK(hipEventRecord(ev[1], st));
    HIP_OK(hipStreamSynchronize(st));
    float ms = 0.0f;
    HIP_OK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    tm.ms[1] = (double)ms;
    return now_seconds();
  }
  void finish(double t_down, int64_t points) {
    HIP_OK(hipStreamSynchronize(st));
    const double t = now_seconds();
    tm.ms[2] = (t - t_down) * 1e3;
    tm.ms[3] = (t - this->t[0]) * 1e3;
    tm.count = points;
    DeviceCall::finish();
  }
};

void run_triangulate(const mcba_triangulate_problem* p, double* X, double* cov, double* sse, double* err, int32_t* n_views,
                     uint8_t* status) {
  TriangulateCall call;   // (before the buffers: see host::DeviceCall)
  std::vector<double> cam;
  std::string msg;
  int64_t n_points = 0;
  if (!triangulate::plan_problem(p, X, status, cam, &n_points, msg)) throw Error(msg);
  if (n_points == 0) return;             // nothing is launched, the device is not touched
  const size_t C = (size_t)p->cams.C, F = (size_t)p->F, N = (size_t)n_points;
  DevBuf<double> d_cam, d_views, d_end, d_points, d_X, d_cov, d_sse, d_err;
  DevBuf<uint8_t> d_view_valid, d_valid, d_status;
  DevBuf<int32_t> d_n;
  call.open();
  triangulate::KernelArgs a{};
  upload_async(d_cam, cam.data(), cam.size(), call.st);
  upload_async(d_views, p->views, C * F * 12, call.st);
  if (p->views_end) upload_async(d_end, p->views_end, C * F * 12, call.st);
  if (p->view_valid) upload_async(d_view_valid, p->view_valid, C * F, call.st);
  upload_async(d_points, p->points, C * N * 2, call.st);
  upload_async(d_valid, p->valid, C * N, call.st);
  d_X.alloc(N * 3, false);
  d_status.alloc(N, false);
  if (cov) d_cov.alloc(N * 6, false);
  if (sse) d_sse.alloc(N, false);
  if (err) d_err.alloc(C * N, false);
  if (n_views) d_n.alloc(N, false);
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
  a.cov = cov ? d_cov.p : nullptr; a.sse = sse ? d_sse.p : nullptr; a.err = err ? d_err.p : nullptr;
  a.n_views = n_views ? d_n.p : nullptr;
  call.begin_kernel();
  triangulate::triangulate_launch(a, call.st);
  const double t_down = call.end_kernel("k_triangulate");
  download_async(X, d_X, N * 3, call.st);
  download_async(status, d_status, N, call.st);
  if (cov) download_async(cov, d_cov, N * 6, call.st);
  if (sse) download_async(sse, d_sse, N, call.st);
  if (err) download_async(err, d_err, C * N, call.st);
  if (n_views) download_async(n_views, d_n, N, call.st);
  call.finish(t_down, n_points);
}
}  // namespace

int32_t mcba_triangulate(const mcba_triangulate_problem* p, double* X, double* cov, double* sse, double* err, int32_t* n_views,
                         uint8_t* status) {
  API_BEGIN
  run_triangulate(p, X, cov, sse, err, n_views, status);
  API_END
}

}  // extern "C"

MCBA_TIMING_GETTER(mcba_debug_triangulate_ms, g_triangulate_timing)
