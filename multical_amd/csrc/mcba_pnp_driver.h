// mcba_pnp_driver.h -- host side of mcba_view_poses that does not touch the device: argument checks, camera entries, board plane
// frames and the list of active views.  Shared by the driver (mcba_pnp.hip) and the host build of the per-view mathematics
// (tests/pnp_host), so that both walk the same views with the same inputs.
#pragma once
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/mcba.h"
#include "mcba_pnp.h"

namespace mcba {
namespace pnp {

struct ViewPlan {
  std::vector<double> cam;          // [C][CAM_STRIDE] camera_entry of every camera
  std::vector<int32_t> cam_nd;      // [C] the camera's own coefficient count
  std::vector<uint8_t> cam_fish;    // [C]
  std::vector<double> planes;       // [B][PLANE_STRIDE]
  std::vector<int32_t> active;      // views to estimate, ascending
  std::vector<int32_t> desc;        // [active][2] camera, board
  std::vector<uint8_t> status;      // [C F B] MCBA_VIEW_MASKED / TOO_FEW of the views that are not estimated (else OK)
  int max_iter = 50;
};

// The plane frame of every board ([B][PLANE_STRIDE]; board_sizes: corners of every board, or null = P).  need_planar: the call
// starts from homographies, so a board that leaves its plane by more than PLANAR_TOL of its extent is refused, with the
// arguments that would serve it (`advice`) in the message.  Shared with mcba_calibrate_intrinsics (mcba_intrinsic_driver.h).
inline bool fit_board_planes(const double* board_points, const int32_t* board_sizes, int B, int P, bool need_planar, const char* who,
                             const char* advice, std::vector<double>& planes, std::string& err) {
  planes.assign((size_t)B * PLANE_STRIDE, 0.0);
  for (int b = 0; b < B; ++b) {
    const int nb = board_sizes ? board_sizes[b] : P;
    if (nb < 0 || nb > P) { err = std::string(who) + ": board size out of range"; return false; }
    const double dev = board_plane(board_points + (size_t)b * P * 3, nb, planes.data() + (size_t)b * PLANE_STRIDE);
    if (need_planar && !(dev <= PLANAR_TOL)) {
      char msg[256];
      snprintf(msg, sizeof msg, "%s: board %d is not planar (%.3g of its extent off its plane): the homography start needs a planar "
               "target, pass %s", who, b, dev, advice);
      err = msg;
      return false;
    }
  }
  return true;
}

inline bool plan_views(const mcba_view_pose_problem& p, ViewPlan& out, std::string& err) {
  if (p.C <= 0 || p.F <= 0 || p.B <= 0 || p.P <= 0) { err = "mcba_view_poses: C, F, B, P must be positive"; return false; }
  if (!p.points || !p.valid || !p.board_points || !p.cameras) { err = "mcba_view_poses: null table"; return false; }
  if (p.n_dist < 0 || p.n_dist > MAX_DIST) { err = "mcba_view_poses: n_dist must be 0 .. 14"; return false; }
  const long long views = (long long)p.C * p.F * p.B;
  if (views >= (1ll << 31) / 16 || (long long)p.P > (1 << 20)) { err = "mcba_view_poses: table too large"; return false; }
  const int stride = 5 + p.n_dist;
  out.cam.assign((size_t)p.C * CAM_STRIDE, 0.0);
  out.cam_nd.resize(p.C);
  out.cam_fish.resize(p.C);
  for (int c = 0; c < p.C; ++c) {
    const bool fish = p.is_fisheye && p.is_fisheye[c];
    const int nd = fish ? 4 : (p.camera_n_dist ? p.camera_n_dist[c] : p.n_dist);
    if (nd > p.n_dist || !supported_model(nd, fish)) {
      char msg[160];
      snprintf(msg, sizeof msg, "mcba_view_poses: camera %d: %d distortion coefficients (4, 5, 8, 12, 14; fisheye 4) in blocks of %d",
               c, nd, p.n_dist);
      err = msg;
      return false;
    }
    const double* blk = p.cameras + (size_t)c * stride;
    const bool fa = p.fix_aspect && p.fix_aspect[c];
    if (!(blk[0] > 0.0) || !((fa ? blk[0] : blk[1]) > 0.0)) { err = "mcba_view_poses: focal lengths must be positive"; return false; }
    camera_entry(blk, nd, 0.0, fa, out.cam.data() + (size_t)c * CAM_STRIDE, fish);
    out.cam_nd[c] = nd;
    out.cam_fish[c] = fish ? 1 : 0;
  }
  if (!fit_board_planes(p.board_points, p.board_sizes, p.B, p.P, !p.init_poses, "mcba_view_poses", "init_poses", out.planes, err))
    return false;
  out.status.assign((size_t)views, (uint8_t)ST_OK);
  out.active.clear();
  out.desc.clear();
  for (long long v = 0; v < views; ++v) {
    if (p.view_mask && !p.view_mask[v]) { out.status[v] = (uint8_t)ST_MASKED; continue; }
    const uint8_t* m = p.valid + (size_t)v * p.P;
    int n = 0;
    for (int j = 0; j < p.P; ++j) n += m[j] != 0;
    if (n < MIN_CORNERS) { out.status[v] = (uint8_t)ST_TOO_FEW; continue; }
    out.active.push_back((int32_t)v);
    out.desc.push_back((int32_t)(v / ((long long)p.F * p.B)));
    out.desc.push_back((int32_t)(v % p.B));
  }
  out.max_iter = p.max_iterations > 0 ? p.max_iterations : 50;
  return true;
}

// The rows of the ACTIVE views only, gathered into one staging buffer the driver supplies (pinned: the table is about 0.3 full, and
// a pinned source is copied without the runtime's staging pass): pixels [na][P][2] | start poses [na][16] or none | valid [na][P]
struct ActiveRows {
  size_t px_bytes, in_bytes, ok_bytes;
  double *px = nullptr, *in = nullptr;
  uint8_t* ok = nullptr;
  ActiveRows(size_t na, size_t P, bool with_poses)
      : px_bytes(na * P * 2 * sizeof(double)), in_bytes(with_poses ? na * 16 * sizeof(double) : 0), ok_bytes(na * P) {}
  size_t bytes() const { return px_bytes + in_bytes + ok_bytes; }
  void gather(void* stage, const std::vector<int32_t>& active, size_t P, const double* points, const uint8_t* valid, const double* poses) {
    px = (double*)stage;
    in = (double*)((char*)stage + px_bytes);
    ok = (uint8_t*)stage + px_bytes + in_bytes;
    for (size_t k = 0; k < active.size(); ++k) {
      const size_t v = (size_t)active[k];
      memcpy(px + k * P * 2, points + v * P * 2, P * 2 * sizeof(double));
      memcpy(ok + k * P, valid + v * P, P);
      if (in_bytes) memcpy(in + k * 16, poses + v * 16, 16 * sizeof(double));
    }
  }
};

// outputs of the views that are not estimated (and the default of those that are)
inline void fill_invalid(const mcba_view_pose_problem& p, const ViewPlan& plan, double* poses, double* sse, int32_t* n_used,
                         uint8_t* status) {
  const size_t views = plan.status.size();
  for (size_t v = 0; v < views; ++v) {
    identity_pose(poses + 16 * v);
    sse[v] = 0.0;
    n_used[v] = 0;
    status[v] = plan.status[v];
    if (p.lm_iterations) p.lm_iterations[v] = 0;
  }
}

}  // namespace pnp
}  // namespace mcba
