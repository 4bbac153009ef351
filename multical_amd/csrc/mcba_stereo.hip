// translation unit of k_stereo_pair (mcba_stereo_kernels.h) and the host driver of mcba_stereo_calibrate
#include "mcba_host.h"
#include "mcba_stereo_driver.h"
#include "mcba_stereo_kernels.h"

namespace mcba {
namespace stereo {

hipError_t stereo_pair_launch(const StereoArgs& a, int n_launched, hipStream_t st) {
  if (n_launched <= 0) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute((const void*)k_stereo_pair, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PAIR_LDS_BYTES);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_stereo_pair, dim3(n_launched), dim3(PAIR_THREADS), PAIR_LDS_BYTES, st, a);
  return hipGetLastError();
}

}  // namespace stereo
}  // namespace mcba

using namespace mcba;
using namespace mcba::host;

// host preparation | uploads | kernel (HIP events around the launch) | downloads + scatter; pairs launched
MCBA_TIMING_GETTER(mcba_debug_stereo_calibrate_ms, g_stereo_timing, 4)

extern "C" {

namespace {
void run_stereo(const mcba_stereo_problem* p, double* T, double* cov, double* sse, int32_t* n_views, int32_t* n_points,
                int32_t* iterations, double* view_poses_out, double* view_sse, uint8_t* status) {
  DeviceCall call(g_stereo_timing);   // (before the buffers: see the type)
  call.tm.reset();
  stereo::Plan plan;
  std::string msg;
  if (!stereo::plan_problem(p, T, status, plan, msg)) throw Error(msg);
  stereo::fill_unsolved(p, plan, T, cov, sse, n_views, n_points, iterations, view_poses_out, view_sse, status);
  const size_t nl = plan.n_launched(), nvw = plan.total_views();
  if (nl == 0) return call.record();   // no pair has a view: nothing is launched, the device is not touched
  call.tm.reset((int64_t)nl);
  const size_t C = (size_t)plan.C, FB = (size_t)plan.F * plan.B, P = (size_t)plan.P;
  std::vector<int32_t> np(nl);
  for (size_t i = 0; i < nl; ++i) np[i] = plan.n_points[(size_t)plan.launched[i]];
  call.open(2);
  const hipStream_t st = call.st;
  DevBuf<double> d_recs, d_board, d_points, d_vposes, d_ws(nvw * stereo::VB_STRIDE), d_T(nl * 16);
  DevBuf<uint8_t> d_bvalid, d_valid, d_status(nl);
  DevBuf<int32_t> d_desc, d_first, d_slot, d_ncommon, d_np;
  OutBuf<double> o_cov(cov, nl * 36), o_sse(sse, nl);
  OutBuf<int32_t> o_iters(iterations, nl);
  upload_vector(d_recs, plan.recs, st);
  upload_async(d_board, p->board_points, (size_t)plan.B * P * 3, st);
  if (p->board_valid) upload_async(d_bvalid, p->board_valid, (size_t)plan.B * P, st);
  upload_async(d_points, p->points, C * FB * P * 2, st);   // (one table for all pairs: nothing is duplicated per pair)
  upload_async(d_valid, p->valid, C * FB * P, st);
  upload_async(d_vposes, p->view_poses, C * FB * 16, st);
  upload_vector(d_desc, plan.desc, st);
  upload_vector(d_first, plan.first, st);
  upload_vector(d_slot, plan.slot, st);
  upload_vector(d_ncommon, plan.n_common, st);
  upload_vector(d_np, np, st);
  call.mark(0);
  stereo::StereoArgs a{};
  a.t = stereo::Tables{plan.F, plan.B, plan.P, d_recs.p, d_board.p, p->board_valid ? d_bvalid.p : nullptr, d_points.p, d_valid.p, d_vposes.p};
  a.max_iter = plan.max_iter;
  a.sigma_px = p->sigma_px;
  a.desc = d_desc.p; a.first = d_first.p; a.slot = d_slot.p; a.n_common = d_ncommon.p; a.n_points = d_np.p;
  a.ws = d_ws.p; a.T = d_T.p; a.cov = o_cov.dev(); a.sse = o_sse.dev(); a.iters = o_iters.dev(); a.status = d_status.p;
  const hipError_t e = stereo::stereo_pair_launch(a, (int)nl, st);
  if (e != hipSuccess) throw Error(std::string("kernel launch failed (k_stereo_pair): ") + hipGetErrorString(e));
  call.mark(1);
  call.end_kernels("k_stereo_pair");
  const bool views_out = view_poses_out || view_sse;
  std::vector<double> h_T(nl * 16), h_cov(cov ? nl * 36 : 0), h_sse(sse ? nl : 0), h_ws(views_out ? nvw * stereo::VB_STRIDE : 0);
  std::vector<int32_t> h_iters(iterations ? nl : 0);
  std::vector<uint8_t> h_status(nl);
  download_async(h_T.data(), d_T.p, nl * 16, st);
  download_async(h_status.data(), d_status.p, nl, st);
  o_cov.fetch(st, h_cov.data());
  o_sse.fetch(st, h_sse.data());
  o_iters.fetch(st, h_iters.data());
  if (views_out) download_async(h_ws.data(), d_ws.p, nvw * stereo::VB_STRIDE, st);
  HIP_OK(hipStreamSynchronize(st));
  for (size_t i = 0; i < nl; ++i) {
    const size_t k = (size_t)plan.launched[i];
    memcpy(T + 16 * k, h_T.data() + 16 * i, 16 * sizeof(double));
    if (cov) memcpy(cov + 36 * k, h_cov.data() + 36 * i, 36 * sizeof(double));
    if (sse) sse[k] = h_sse[i];
    if (iterations) iterations[k] = h_iters[i];
    status[k] = h_status[i];
  }
  if (views_out) stereo::scatter_views(plan, h_ws.data(), h_status.data(), view_poses_out, view_sse);
  call.finish_prepared((int64_t)nl);
}
}  // namespace

int32_t mcba_stereo_calibrate(const mcba_stereo_problem* p, double* T, double* cov, double* sse, int32_t* n_views, int32_t* n_points,
                              int32_t* iterations, double* view_poses_out, double* view_sse, uint8_t* status) {
  API_BEGIN
  run_stereo(p, T, cov, sse, n_views, n_points, iterations, view_poses_out, view_sse, status);
  API_END
}

}  // extern "C"
