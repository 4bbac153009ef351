// translation unit of k_view_pose (mcba_pnp_kernels.h): the three register-array sizes, camera family switched at run time;
// and the host driver of mcba_view_poses
#include "mcba_host.h"
#include "mcba_pnp_driver.h"
#include "mcba_pnp_kernels.h"

namespace mcba {
namespace pnp {

void view_pose_launch(const ViewPoseArgs& a, hipStream_t st) {
  if (a.n_active <= 0) return;
  const dim3 grid((a.n_active + VIEW_POSE_THREADS / 64 - 1) / (VIEW_POSE_THREADS / 64)), block(VIEW_POSE_THREADS);
  switch (view_pose_npl(a.P)) {
    case 2: hipLaunchKernelGGL(k_view_pose<2>, grid, block, 0, st, a); break;
    case 6: hipLaunchKernelGGL(k_view_pose<6>, grid, block, 0, st, a); break;
    case 16: hipLaunchKernelGGL(k_view_pose<16>, grid, block, 0, st, a); break;
    default: break;   // (refused by the caller)
  }
}

}  // namespace pnp
}  // namespace mcba

using namespace mcba;
using namespace mcba::host;

// plan + gather | uploads | kernel | downloads + scatter; active views
MCBA_TIMING_GETTER(mcba_debug_view_poses_ms, g_view_pose_timing, 4)

extern "C" {

namespace {
void view_poses(const mcba_view_pose_problem& p, double* poses, double* sse, int32_t* n_used, uint8_t* status) {
  DeviceCall call(g_view_pose_timing);   // (before the buffers: see the type)
  pnp::ViewPlan plan;
  std::string err;
  if (!pnp::plan_views(p, plan, err)) throw Error(err);
  REQUIRE(pnp::view_pose_npl(p.P) > 0, "mcba_view_poses: boards of more than 1024 corners are not served");
  pnp::fill_invalid(p, plan, poses, sse, n_used, status);
  const size_t na = plan.active.size(), P = (size_t)p.P;
  call.tm.reset((int64_t)na);
  if (na == 0) return call.record();   // nothing to estimate: nothing is launched, the device is not touched
  call.open();
  const hipStream_t st = call.st;
  pnp::ActiveRows rows(na, P, p.init_poses != nullptr);
  PinnedBuf pinned(rows.bytes());
  rows.gather(pinned.p, plan.active, P, p.points, p.valid, p.init_poses);
  // d_out: pose [na][16] | sse [na]; d_int: n_used [na] | iterations [na]
  DevBuf<double> d_px(na * P * 2), d_in, d_board((size_t)p.B * P * 3), d_cam(plan.cam.size()), d_planes(plan.planes.size()), d_out(na * 17);
  DevBuf<uint8_t> d_ok(na * P), d_fish((size_t)p.C), d_status(na);
  DevBuf<int32_t> d_desc(2 * na), d_nd((size_t)p.C), d_int(na * 2);
  if (p.init_poses) d_in.alloc(na * 16, false);
  call.stamp();
  upload_async(d_px, rows.px, na * P * 2, st);   // (the buffers are sized above: nothing is allocated here)
  upload_async(d_ok, rows.ok, na * P, st);
  if (p.init_poses) upload_async(d_in, rows.in, na * 16, st);
  upload_async(d_board, p.board_points, (size_t)p.B * P * 3, st);
  upload_async(d_cam, plan.cam.data(), plan.cam.size(), st);
  upload_async(d_planes, plan.planes.data(), plan.planes.size(), st);
  upload_async(d_desc, plan.desc.data(), 2 * na, st);
  upload_async(d_nd, plan.cam_nd.data(), (size_t)p.C, st);
  upload_async(d_fish, plan.cam_fish.data(), (size_t)p.C, st);
  HIP_OK(hipStreamSynchronize(st));
  call.stamp();
  pnp::ViewPoseArgs a;
  a.n_active = (int)na; a.P = p.P; a.max_iter = plan.max_iter;
  a.pixel = d_px.p; a.valid = d_ok.p; a.desc = d_desc.p; a.init = p.init_poses ? d_in.p : nullptr; a.board = d_board.p;
  a.cam = d_cam.p; a.cam_nd = d_nd.p; a.cam_fish = d_fish.p; a.planes = d_planes.p;
  a.pose = d_out.p; a.sse = d_out.p + na * 16; a.n_used = d_int.p; a.iters = d_int.p + na; a.status = d_status.p;
  pnp::view_pose_launch(a, st);
  check_launch("k_view_pose");
  HIP_OK(hipStreamSynchronize(st));
  call.stamp();
  std::vector<double> h_out(na * 17);
  std::vector<int32_t> h_int(na * 2);
  std::vector<uint8_t> h_status(na);
  download_async(h_out.data(), d_out.p, na * 17, st);
  download_async(h_int.data(), d_int.p, na * 2, st);
  download_async(h_status.data(), d_status.p, na, st);
  HIP_OK(hipStreamSynchronize(st));
  for (size_t k = 0; k < na; ++k) {
    const size_t v = (size_t)plan.active[k];
    memcpy(poses + v * 16, h_out.data() + k * 16, 16 * sizeof(double));
    sse[v] = h_out[na * 16 + k];
    n_used[v] = h_int[k];
    status[v] = h_status[k];
    if (p.lm_iterations) p.lm_iterations[v] = h_int[na + k];
  }
  call.record();
  const double* ms = call.tm.ms;
  if (getenv("MCBA_TIMING"))
    fprintf(stderr, "[view_poses] %lld of %lld views, %d corners a row: plan + gather %.2f ms, uploads (%.1f MB) %.2f ms, kernel %.2f ms, "
            "downloads + scatter %.2f ms\n", (long long)na, (long long)plan.status.size(), p.P, ms[0],
            (double)rows.bytes() / 1e6, ms[1], ms[2], ms[3]);
  call.finish();
}
}  // namespace

int32_t mcba_view_poses(const mcba_view_pose_problem* p, double* poses, double* sse, int32_t* n_used, uint8_t* status) {
  API_BEGIN
  REQUIRE(p && poses && sse && n_used && status, "null argument");
  view_poses(*p, poses, sse, n_used, status);
  API_END
}

}  // extern "C"
