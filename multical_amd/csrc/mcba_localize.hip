// translation unit of k_rig_pose (mcba_localize_kernels.h) and the host driver of mcba_rig_poses (its start poses come from
// pnp::view_pose_launch of mcba_pnp.hip: their output stays on the device)
#include "mcba_host.h"
#include "mcba_localize_driver.h"
#include "mcba_localize_kernels.h"

namespace mcba {
namespace localize {

static_assert(MAX_VIEW_CORNERS == 1024, "the largest board pnp::view_pose_npl serves");

template <bool ROLLING>
static hipError_t launch(const RigPoseArgs& a, hipStream_t st) {
  const size_t bytes = rig_lds_bytes(a.C);   // 84 KiB + 544 bytes a camera: above the default limit of a launch
  const hipError_t e = hipFuncSetAttribute((const void*)k_rig_pose<ROLLING>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_rig_pose<ROLLING>), dim3(a.F), dim3(RIG_THREADS), bytes, st, a);
  return hipGetLastError();
}

hipError_t rig_pose_launch(const RigPoseArgs& a, bool rolling, hipStream_t st) {
  if (a.F <= 0) return hipSuccess;
  return rolling ? launch<true>(a, st) : launch<false>(a, st);
}

}  // namespace localize
}  // namespace mcba

using namespace mcba;
using namespace mcba::host;

// uploads | start kernel | refinement kernel (HIP events) | downloads | whole call; frames launched
MCBA_TIMING_GETTER(mcba_debug_rig_poses_ms, g_rig_pose_timing, 5)

extern "C" {

namespace {
void run_rig_poses(const mcba_rig_pose_problem* p, double* poses, double* poses_end, double* cov, double* sse, int32_t* n_obs,
                   int32_t* iters, double* err, uint8_t* status) {
  DeviceCall call(g_rig_pose_timing);   // (before the buffers: see the type)
  call.tm.reset();
  localize::Plan plan;
  std::string msg;
  bool empty = true;
  if (!localize::plan_problem(p, poses, status, plan, &empty, msg)) throw Error(msg);
  if (empty || plan.n_records() == 0) {   // nothing is launched, the device is not touched
    localize::fill_empty(p, plan.K, poses, poses_end, cov, sse, n_obs, iters, status);
    if (err && !empty) localize::scatter_errors(plan, nullptr, err);
    return;
  }
  const size_t F = (size_t)plan.F, N = plan.n_records(), nv = plan.n_views(), P = (size_t)plan.P, KC = (size_t)localize::n_cov(plan.K);
  if (n_obs)
    for (size_t f = 0; f < F; ++f) n_obs[f] = plan.first[f + 1] - plan.first[f];
  DevBuf<double> d_recs, d_uv, d_W, d_init, d_init_end, d_cam_inv, d_board_inv, d_poses;
  DevBuf<double> d_vpx, d_board, d_vcam, d_planes, d_vpose, d_vsse;
  DevBuf<int32_t> d_first, d_ocam, d_owpt, d_vfirst, d_vdesc, d_vnd, d_vn, d_vit;
  DevBuf<uint8_t> d_status, d_vok, d_vfish, d_vstatus;
  call.open(3);
  const hipStream_t st = call.st;
  upload_vector(d_recs, plan.recs, st);
  upload_vector(d_uv, plan.uv, st);
  upload_vector(d_W, plan.W, st);
  upload_vector(d_first, plan.first, st);
  upload_vector(d_ocam, plan.ocam, st);
  upload_vector(d_owpt, plan.owpt, st);
  std::vector<double> vpx;
  std::vector<uint8_t> vok;
  if (p->init) {
    upload_async(d_init, p->init, F * 16, st);
    if (p->init_end && plan.rolling) upload_async(d_init_end, p->init_end, F * 16, st);
  } else {
    upload_vector(d_vfirst, plan.view_first, st);
    upload_vector(d_cam_inv, plan.cam_inv, st);
    upload_vector(d_board_inv, plan.board_inv, st);
    if (nv > 0) {
      vpx.resize(nv * P * 2);
      vok.resize(nv * P);
      localize::gather_views(p, plan, vpx.data(), vok.data());
      upload_vector(d_vpx, vpx, st);
      upload_vector(d_vok, vok, st);
      upload_vector(d_vdesc, plan.view_desc, st);
      upload_async(d_board, p->board_points, (size_t)plan.B * P * 3, st);
      upload_vector(d_vcam, plan.cams.cam, st);
      upload_vector(d_vnd, plan.cams.cam_nd, st);
      upload_vector(d_vfish, plan.cams.cam_fish, st);
      upload_vector(d_planes, plan.planes, st);
    }
    d_vpose.alloc(nv * 16, false);
    d_vsse.alloc(nv, false);
    d_vn.alloc(nv, false);
    d_vit.alloc(nv, false);
    d_vstatus.alloc(nv, false);
  }
  d_poses.alloc(F * 16, false);
  d_status.alloc(F, false);
  OutBuf<double> o_poses_end(poses_end, F * 16), o_cov(cov, F * KC), o_sse(sse, F), o_err(err, N);   // (err: by record, see below)
  OutBuf<int32_t> o_iters(iters, F);
  call.mark(0);
  if (!p->init && nv > 0) {
    pnp::ViewPoseArgs v;
    v.n_active = (int)nv; v.P = plan.P; v.max_iter = 50;
    v.pixel = d_vpx.p; v.valid = d_vok.p; v.desc = d_vdesc.p; v.init = nullptr; v.board = d_board.p;
    v.cam = d_vcam.p; v.cam_nd = d_vnd.p; v.cam_fish = d_vfish.p; v.planes = d_planes.p;
    v.pose = d_vpose.p; v.sse = d_vsse.p; v.n_used = d_vn.p; v.iters = d_vit.p; v.status = d_vstatus.p;
    pnp::view_pose_launch(v, st);
    check_launch("k_view_pose");
  }
  call.mark(1);
  localize::RigPoseArgs a{};
  a.C = plan.C; a.F = plan.F; a.max_iter = plan.max_iter;
  a.sigma_px = p->sigma_px;
  a.recs = d_recs.p; a.first = d_first.p; a.uv = d_uv.p; a.ocam = d_ocam.p; a.owpt = d_owpt.p; a.W = d_W.p;
  a.init = p->init ? d_init.p : nullptr;
  a.init_end = (p->init && p->init_end && plan.rolling) ? d_init_end.p : nullptr;
  a.view_first = d_vfirst.p; a.view_desc = d_vdesc.p; a.view_pose = d_vpose.p; a.view_n = d_vn.p; a.view_status = d_vstatus.p;
  a.cam_inv = d_cam_inv.p; a.board_inv = d_board_inv.p;
  a.poses = d_poses.p; a.status = d_status.p;
  a.poses_end = o_poses_end.dev(); a.cov = o_cov.dev(); a.sse = o_sse.dev(); a.iters = o_iters.dev(); a.err = o_err.dev();
  const hipError_t e = localize::rig_pose_launch(a, plan.rolling, st);
  if (e != hipSuccess) throw Error(std::string("kernel launch failed (k_rig_pose): ") + hipGetErrorString(e));
  call.mark(2);
  call.end_kernels("k_rig_pose");
  std::vector<double> err_rec(err ? N : 0);
  download_async(poses, d_poses.p, F * 16, st);
  download_async(status, d_status.p, F, st);
  o_poses_end.fetch(st);
  o_cov.fetch(st);
  o_sse.fetch(st);
  o_iters.fetch(st);
  o_err.fetch(st, err_rec.data());
  HIP_OK(hipStreamSynchronize(st));
  if (err) localize::scatter_errors(plan, err_rec.data(), err);
  call.finish((int64_t)F);
}
}  // namespace

int32_t mcba_rig_poses(const mcba_rig_pose_problem* p, double* poses, double* poses_end, double* cov, double* sse, int32_t* n_obs,
                       int32_t* iters, double* err, uint8_t* status) {
  API_BEGIN
  run_rig_poses(p, poses, poses_end, cov, sse, n_obs, iters, err, status);
  API_END
}

}  // extern "C"
