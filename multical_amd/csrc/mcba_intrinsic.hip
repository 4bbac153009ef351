// translation unit of the intrinsic calibration kernels (mcba_intrinsic_kernels.h): the homography kernel in the three
// register-array sizes of k_view_pose, the focal start, and k_calibrate_camera for every camera family; and the host driver of
// mcba_calibrate_intrinsics (its start poses come from pnp::view_pose_launch of mcba_pnp.hip)
#include "mcba_host.h"
#include "mcba_intrinsic_driver.h"
#include "mcba_intrinsic_kernels.h"

namespace mcba {
namespace intr {

hipError_t intrinsic_start_launch(const IntrinsicArgs& a, int n_views, int C, hipStream_t st) {
  if (n_views <= 0) return hipSuccess;
  const dim3 grid((n_views + pnp::VIEW_POSE_THREADS / 64 - 1) / (pnp::VIEW_POSE_THREADS / 64)), block(pnp::VIEW_POSE_THREADS);
  switch (pnp::view_pose_npl(a.P)) {
    case 2: hipLaunchKernelGGL(k_intrinsic_homography<2>, grid, block, 0, st, a, n_views); break;
    case 6: hipLaunchKernelGGL(k_intrinsic_homography<6>, grid, block, 0, st, a, n_views); break;
    case 16: hipLaunchKernelGGL(k_intrinsic_homography<16>, grid, block, 0, st, a, n_views); break;
    default: return hipErrorInvalidValue;   // (refused by the caller)
  }
  hipLaunchKernelGGL(k_intrinsic_focal, dim3(C), dim3(64), 0, st, a);
  return hipGetLastError();
}

template <int ND, bool FISH>
static hipError_t launch_family(const IntrinsicArgs& a, int n_cameras, hipStream_t st) {
  // 124.5 KiB of LDS for the one workgroup a camera gets: above the default limit of a launch
  const hipError_t e = hipFuncSetAttribute((const void*)k_calibrate_camera<ND, FISH>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)CAL_LDS_BYTES);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_calibrate_camera<ND, FISH>), dim3(n_cameras), dim3(CAL_THREADS), CAL_LDS_BYTES, st, a);
  return hipGetLastError();
}

hipError_t calibrate_camera_launch(const IntrinsicArgs& a, int nd, bool fisheye, int n_cameras, hipStream_t st) {
  if (n_cameras <= 0) return hipSuccess;
  if (fisheye) return launch_family<4, true>(a, n_cameras, st);
  switch (nd) {
    case 4: return launch_family<4, false>(a, n_cameras, st);
    case 5: return launch_family<5, false>(a, n_cameras, st);
    case 8: return launch_family<8, false>(a, n_cameras, st);
    case 12: return launch_family<12, false>(a, n_cameras, st);
    case 14: return launch_family<14, false>(a, n_cameras, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace intr
}  // namespace mcba

using namespace mcba;
using namespace mcba::host;

// plan + gather | uploads | kernels | downloads + scatter; active views
MCBA_TIMING_GETTER(mcba_debug_calibrate_intrinsics_ms, g_intrinsic_timing, 4)

extern "C" {

namespace {
void calibrate_intrinsics(const mcba_intrinsic_problem& p, double* cameras, double* poses, double* sse, int32_t* n_used,
                          uint8_t* view_status, uint8_t* camera_status) {
  DeviceCall call(g_intrinsic_timing);   // (before the buffers: see the type)
  intr::IntrinsicPlan plan;
  std::string err;
  if (!intr::plan_intrinsics(p, plan, err)) throw Error(err);
  REQUIRE(pnp::view_pose_npl(p.P) > 0, "mcba_calibrate_intrinsics: boards of more than 1024 corners are not served");
  intr::fill_unsolved(p, plan, cameras, poses, sse, n_used, view_status, camera_status);
  const size_t na = plan.active.size(), P = (size_t)p.P, nc = (size_t)p.C;
  call.tm.reset((int64_t)na);
  if (na == 0) return call.record();   // no camera to solve: nothing is uploaded or launched, the device is not touched
  call.open();
  const hipStream_t st = call.st;
  pnp::ActiveRows rows(na, P, plan.warm);   // (camera-major here: a camera's views are one run)
  PinnedBuf pinned(rows.bytes());
  rows.gather(pinned.p, plan.active, P, p.points, p.valid, p.init_poses);
  std::vector<double> h_blk(nc * intr::BLK, 0.0);
  if (plan.warm)
    for (size_t c = 0; c < nc; ++c)
      for (int i = 0; i < 5 + p.n_dist; ++i) h_blk[c * intr::BLK + i] = p.init_cameras[c * (5 + (size_t)p.n_dist) + i];
  std::vector<int32_t> h_group;
  for (const auto& g : plan.group_cameras) h_group.insert(h_group.end(), g.begin(), g.end());
  DevBuf<double> d_px(na * P * 2), d_pose(na * 16), d_board((size_t)p.B * P * 3), d_planes(plan.planes.size()), d_mask(plan.mask.size()),
      d_size(2 * nc), d_hv(na * 10), d_blk(nc * intr::BLK), d_entry(nc * CAM_STRIDE), d_sse(na), d_ws(na * intr::VB_STRIDE);
  DevBuf<uint8_t> d_ok(na * P), d_fa(nc), d_fish(nc), d_vstatus(na), d_cstatus(nc);
  // d_int: n_used [na] | iterations of the start poses [na] | usable views [na] | LM passes [C]
  DevBuf<int32_t> d_desc(2 * na), d_first(nc + 1), d_nd(nc), d_int(3 * na + nc), d_group(h_group.size());
  call.stamp();
  upload_async(d_px, rows.px, na * P * 2, st);   // (the buffers are sized above: nothing is allocated here)
  upload_async(d_ok, rows.ok, na * P, st);
  if (plan.warm) upload_async(d_pose, rows.in, na * 16, st);
  upload_async(d_board, p.board_points, (size_t)p.B * P * 3, st);
  upload_async(d_planes, plan.planes.data(), plan.planes.size(), st);
  upload_async(d_mask, plan.mask.data(), plan.mask.size(), st);
  upload_async(d_size, plan.image_size.data(), 2 * nc, st);
  upload_async(d_blk, h_blk.data(), h_blk.size(), st);
  upload_async(d_fa, plan.cam_fa.data(), nc, st);
  upload_async(d_fish, plan.cam_fish.data(), nc, st);
  upload_async(d_cstatus, plan.cam_status.data(), nc, st);
  upload_async(d_desc, plan.desc.data(), 2 * na, st);
  upload_async(d_first, plan.cam_first.data(), nc + 1, st);
  upload_async(d_nd, plan.cam_nd.data(), nc, st);
  upload_async(d_group, h_group.data(), h_group.size(), st);
  HIP_OK(hipMemsetAsync(d_vstatus.p, 0, na, st));                       // (warm start: every view is usable)
  HIP_OK(hipMemsetAsync(d_int.p, 0, (3 * na + nc) * sizeof(int32_t), st));
  HIP_OK(hipStreamSynchronize(st));
  call.stamp();
  intr::IntrinsicArgs a;
  a.P = p.P; a.max_iter = plan.max_iter; a.warm = plan.warm ? 1 : 0;
  a.pixel = d_px.p; a.valid = d_ok.p; a.desc = d_desc.p; a.board = d_board.p; a.planes = d_planes.p; a.cam_first = d_first.p;
  a.cam_fa = d_fa.p; a.cam_fish = d_fish.p; a.cam_nd = d_nd.p; a.mask = d_mask.p; a.image_size = d_size.p; a.Hv = d_hv.p;
  a.blk = d_blk.p; a.cam_entry = d_entry.p; a.pose = d_pose.p; a.vstatus = d_vstatus.p; a.sse = d_sse.p; a.n_used = d_int.p;
  a.ws = d_ws.p; a.ulist = d_int.p + 2 * na; a.cam_iters = d_int.p + 3 * na; a.cam_status = d_cstatus.p; a.group = d_group.p;
  if (!plan.warm) {
    // homographies and the focal start, then the start pose of every view with that camera: k_view_pose on the resident rows
    HIP_OK(intr::intrinsic_start_launch(a, (int)na, p.C, st));
    pnp::ViewPoseArgs vp;
    vp.n_active = (int)na; vp.P = p.P; vp.max_iter = 50;
    vp.pixel = d_px.p; vp.valid = d_ok.p; vp.desc = d_desc.p; vp.init = nullptr; vp.board = d_board.p;
    vp.cam = d_entry.p; vp.cam_nd = d_nd.p; vp.cam_fish = d_fish.p; vp.planes = d_planes.p;
    vp.pose = d_pose.p; vp.sse = d_sse.p; vp.n_used = d_int.p; vp.iters = d_int.p + na; vp.status = d_vstatus.p;
    pnp::view_pose_launch(vp, st);
    check_launch("k_view_pose (intrinsic start)");
  }
  size_t g0 = 0;
  for (size_t g = 0; g < plan.groups.size(); ++g) {   // one launch per camera family: a rig may mix them
    a.group = d_group.p + g0;
    HIP_OK(intr::calibrate_camera_launch(a, plan.groups[g].first, plan.groups[g].second != 0, (int)plan.group_cameras[g].size(), st));
    g0 += plan.group_cameras[g].size();
  }
  HIP_OK(hipStreamSynchronize(st));
  call.stamp();
  std::vector<double> h_pose(na * 16), h_sse(na);
  std::vector<int32_t> h_int(3 * na + nc);
  std::vector<uint8_t> h_vstatus(na), h_cstatus(nc);
  download_async(h_blk.data(), d_blk.p, h_blk.size(), st);
  download_async(h_pose.data(), d_pose.p, na * 16, st);
  download_async(h_sse.data(), d_sse.p, na, st);
  download_async(h_int.data(), d_int.p, h_int.size(), st);
  download_async(h_vstatus.data(), d_vstatus.p, na, st);
  download_async(h_cstatus.data(), d_cstatus.p, nc, st);
  HIP_OK(hipStreamSynchronize(st));
  for (int c = 0; c < p.C; ++c) {
    if (plan.cam_first[c + 1] == plan.cam_first[c]) continue;   // (not solved: fill_unsolved has said so)
    camera_status[c] = h_cstatus[c];
    if (p.lm_iterations) p.lm_iterations[c] = h_int[3 * na + c];
    if (!intr::camera_has_result(h_cstatus[c])) {
      intr::drop_camera_views(plan, c, poses, sse, n_used, view_status);
      continue;
    }
    for (int i = 0; i < 5 + plan.cam_nd[c]; ++i) cameras[(size_t)c * (5 + p.n_dist) + i] = h_blk[(size_t)c * intr::BLK + i];
    for (int k = plan.cam_first[c]; k < plan.cam_first[c + 1]; ++k) {
      const size_t v = (size_t)plan.active[k];
      view_status[v] = h_vstatus[k];
      if (h_vstatus[k] != (uint8_t)pnp::ST_OK) continue;
      memcpy(poses + v * 16, h_pose.data() + (size_t)k * 16, 16 * sizeof(double));
      sse[v] = h_sse[k];
      n_used[v] = h_int[k];
    }
  }
  call.record();
  const double* ms = call.tm.ms;
  if (getenv("MCBA_TIMING"))
    fprintf(stderr, "[calibrate_intrinsics] %lld views of %d cameras, %d corners a row: plan + gather %.2f ms, uploads (%.1f MB) %.2f ms, "
            "kernels %.2f ms, downloads + scatter %.2f ms\n", (long long)na, p.C, p.P, ms[0], (double)rows.bytes() / 1e6,
            ms[1], ms[2], ms[3]);
  call.finish();
}
}  // namespace

int32_t mcba_calibrate_intrinsics(const mcba_intrinsic_problem* p, double* cameras, double* poses, double* sse, int32_t* n_used,
                                  uint8_t* view_status, uint8_t* camera_status) {
  API_BEGIN
  REQUIRE(p && cameras && poses && sse && n_used && view_status && camera_status, "null argument");
  calibrate_intrinsics(*p, cameras, poses, sse, n_used, view_status, camera_status);
  API_END
}

}  // extern "C"
