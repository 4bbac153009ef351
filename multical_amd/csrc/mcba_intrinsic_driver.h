// mcba_intrinsic_driver.h -- host side of mcba_calibrate_intrinsics that does not touch the device: argument checks, column masks,
// board plane frames, the compacted list of active views per camera and the (nd, fisheye) launch groups.  Shared by the driver
// (mcba_intrinsic.hip) and the host build of the mathematics (tests/intrinsic_host), so that both walk the same views.
#pragma once
#include <stdio.h>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mcba.h"
#include "mcba_intrinsic.h"
#include "mcba_pnp_driver.h"

namespace mcba {
namespace intr {

struct IntrinsicPlan {
  std::vector<int32_t> cam_nd;        // [C] the camera's own coefficient count
  std::vector<uint8_t> cam_fish, cam_fa;
  std::vector<double> mask;           // [C][MAX_KI] 1 = column estimated, 0 = held
  std::vector<double> image_size;     // [C][2]
  std::vector<double> planes;         // [B][PLANE_STRIDE]
  std::vector<int32_t> active;        // views of the cameras that are solved, ascending (camera-major)
  std::vector<int32_t> desc;          // [active][2] camera, board
  std::vector<int32_t> cam_first;     // [C + 1] range of every camera in `active`
  std::vector<uint8_t> view_status;   // [C F B] MASKED / TOO_FEW of the views that are not used (else OK)
  std::vector<uint8_t> cam_status;    // [C] MASKED / TOO_FEW_VIEWS of the cameras that are not solved (else OK)
  std::vector<std::pair<int, int>> groups;          // distinct (nd, fisheye) of the cameras that are solved
  std::vector<std::vector<int32_t>> group_cameras;  // their cameras
  bool warm = false;
  int max_iter = 100;
};

inline bool plan_intrinsics(const mcba_intrinsic_problem& p, IntrinsicPlan& out, std::string& err) {
  const char* me = "mcba_calibrate_intrinsics";
  auto fail = [&](const std::string& m) { err = std::string(me) + ": " + m; return false; };
  if (p.C <= 0 || p.F <= 0 || p.B <= 0 || p.P <= 0) return fail("C, F, B, P must be positive");
  if (!p.points || !p.valid || !p.board_points || !p.image_sizes) return fail("null table");
  if (p.n_dist < 4 || p.n_dist > MAX_DIST) return fail("n_dist must be 4 .. 14");
  if ((p.init_cameras != nullptr) != (p.init_poses != nullptr)) return fail("init_cameras and init_poses go together");
  const long long views = (long long)p.C * p.F * p.B;
  if (views >= (1ll << 31) / VB_STRIDE || (long long)p.P > (1 << 20)) return fail("table too large");
  out.warm = p.init_cameras != nullptr;
  out.cam_nd.resize(p.C);
  out.cam_fish.resize(p.C);
  out.cam_fa.resize(p.C);
  out.mask.assign((size_t)p.C * MAX_KI, 0.0);
  out.image_size.assign(p.image_sizes, p.image_sizes + 2 * (size_t)p.C);
  for (int c = 0; c < p.C; ++c) {
    const bool fish = p.is_fisheye && p.is_fisheye[c];
    const int nd = fish ? 4 : (p.camera_n_dist ? p.camera_n_dist[c] : p.n_dist);
    if (nd > p.n_dist || !pnp::supported_model(nd, fish)) {
      char msg[160];
      snprintf(msg, sizeof msg, "camera %d: %d distortion coefficients (4, 5, 8, 12, 14; fisheye 4) in blocks of %d", c, nd, p.n_dist);
      return fail(msg);
    }
    if (!(p.image_sizes[2 * c] > 0.0) || !(p.image_sizes[2 * c + 1] > 0.0)) return fail("image sizes must be positive");
    out.cam_nd[c] = nd;
    out.cam_fish[c] = fish ? 1 : 0;
    out.cam_fa[c] = (p.fix_aspect && p.fix_aspect[c]) ? 1 : 0;
    double* m = out.mask.data() + (size_t)c * MAX_KI;
    for (int j = 0; j < 4; ++j) m[j] = 1.0;
    for (int k = 0; k < nd; ++k) m[4 + k] = (!p.free_dist || p.free_dist[(size_t)c * p.n_dist + k]) ? 1.0 : 0.0;
    if (out.warm) {
      const double* blk = p.init_cameras + (size_t)c * (5 + p.n_dist);
      if (!(blk[0] > 0.0) || !((out.cam_fa[c] ? blk[0] : blk[1]) > 0.0)) return fail("focal lengths of init_cameras must be positive");
    }
  }
  if (!pnp::fit_board_planes(p.board_points, p.board_sizes, p.B, p.P, !out.warm, me, "init_cameras and init_poses", out.planes, err))
    return false;
  out.view_status.assign((size_t)views, (uint8_t)pnp::ST_OK);
  out.cam_status.assign((size_t)p.C, (uint8_t)CAM_OK);
  out.active.clear();
  out.desc.clear();
  out.cam_first.assign((size_t)p.C + 1, 0);
  out.groups.clear();
  out.group_cameras.clear();
  const long long per_cam = (long long)p.F * p.B;
  for (int c = 0; c < p.C; ++c) {
    out.cam_first[c] = (int32_t)out.active.size();
    long long unmasked = 0;
    for (long long v = c * per_cam; v < (c + 1) * per_cam; ++v) {
      if (p.view_mask && !p.view_mask[v]) { out.view_status[v] = (uint8_t)pnp::ST_MASKED; continue; }
      ++unmasked;
      const uint8_t* m = p.valid + (size_t)v * p.P;
      int n = 0;
      for (int j = 0; j < p.P; ++j) n += m[j] != 0;
      if (n < pnp::MIN_CORNERS) { out.view_status[v] = (uint8_t)pnp::ST_TOO_FEW; continue; }
      out.active.push_back((int32_t)v);
      out.desc.push_back(c);
      out.desc.push_back((int32_t)(v % p.B));
    }
    const int n_active = (int)out.active.size() - out.cam_first[c];
    if (n_active < MIN_VIEWS) {          // not solved: its views leave the list
      out.cam_status[c] = (uint8_t)(unmasked == 0 ? CAM_MASKED : CAM_TOO_FEW_VIEWS);
      for (size_t k = (size_t)out.cam_first[c]; k < out.active.size(); ++k) out.view_status[out.active[k]] = (uint8_t)pnp::ST_MASKED;
      out.active.resize(out.cam_first[c]);
      out.desc.resize(2 * (size_t)out.cam_first[c]);
      continue;
    }
    const std::pair<int, int> key(out.cam_nd[c], out.cam_fish[c]);
    size_t g = 0;
    while (g < out.groups.size() && out.groups[g] != key) ++g;
    if (g == out.groups.size()) { out.groups.push_back(key); out.group_cameras.emplace_back(); }
    out.group_cameras[g].push_back(c);
  }
  out.cam_first[p.C] = (int32_t)out.active.size();
  out.max_iter = p.max_iterations > 0 ? p.max_iterations : 100;
  return true;
}

// outputs of everything that is not solved (and the default of what is)
inline void fill_unsolved(const mcba_intrinsic_problem& p, const IntrinsicPlan& plan, double* cameras, double* poses, double* sse,
                          int32_t* n_used, uint8_t* view_status, uint8_t* camera_status) {
  const size_t views = plan.view_status.size(), stride = 5 + (size_t)p.n_dist;
  for (size_t v = 0; v < views; ++v) {
    pnp::identity_pose(poses + 16 * v);
    sse[v] = 0.0;
    n_used[v] = 0;
    view_status[v] = plan.view_status[v];
  }
  for (int c = 0; c < p.C; ++c) {
    for (size_t i = 0; i < stride; ++i) cameras[c * stride + i] = p.init_cameras ? p.init_cameras[c * stride + i] : 0.0;
    camera_status[c] = plan.cam_status[c];
    if (p.lm_iterations) p.lm_iterations[c] = 0;
  }
}

// a camera that ends without a result gives its views back: identity, sse 0, n_used 0, MASKED
inline bool camera_has_result(int status) { return status == CAM_OK || status == CAM_NOT_CONVERGED; }
inline void drop_camera_views(const IntrinsicPlan& plan, int c, double* poses, double* sse, int32_t* n_used, uint8_t* view_status) {
  for (int k = plan.cam_first[c]; k < plan.cam_first[c + 1]; ++k) {
    const size_t v = (size_t)plan.active[k];
    pnp::identity_pose(poses + 16 * v);
    sse[v] = 0.0;
    n_used[v] = 0;
    view_status[v] = (uint8_t)pnp::ST_MASKED;
  }
}

}  // namespace intr
}  // namespace mcba
