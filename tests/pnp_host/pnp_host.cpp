// TEST INFRASTRUCTURE: g++ build of the per-view pose mathematics (multical_amd/csrc/mcba_pnp.h) behind the signature of
// mcba_view_poses, plus the reduction order as an argument: 0 = corners summed in table order, 1 = the device's order (64 lane
// partials folded by the xor butterfly).  The views, camera entries and plane frames come from the same plan_views the API uses.
#include <string>
#include <vector>

#include "../../multical_amd/csrc/mcba_pnp_driver.h"

using namespace mcba;
using namespace mcba::pnp;

static thread_local std::string g_error;

template <class Red>
static void run(const mcba_view_pose_problem& p, const ViewPlan& plan, double* poses, double* sse, int32_t* n_used, uint8_t* status) {
  const int P = p.P;
  std::vector<double> buf((size_t)5 * P);
  std::vector<uint8_t> good(P);
  HostPoints pts{buf.data(), buf.data() + P, buf.data() + 2 * P, buf.data() + 3 * P, buf.data() + 4 * P, good.data(), P};
  for (size_t k = 0; k < plan.active.size(); ++k) {
    const size_t v = (size_t)plan.active[k];
    const int c = plan.desc[2 * k], b = plan.desc[2 * k + 1];
    const double* cam = plan.cam.data() + (size_t)c * CAM_STRIDE;
    load_view(pts, 0, 1, P, p.points + v * P * 2, p.valid + v * P, p.board_points + (size_t)b * P * 3, cam, plan.cam_nd[c],
              plan.cam_fish[c] != 0);
    int n = 0, st = 0, it = 0;
    view_pose(pts, Red(), cam, plan.planes.data() + (size_t)b * PLANE_STRIDE, p.init_poses ? p.init_poses + v * 16 : nullptr,
              plan.max_iter, poses + v * 16, sse + v, &n, &st, &it);
    n_used[v] = n;
    status[v] = (uint8_t)st;
    if (p.lm_iterations) p.lm_iterations[v] = it;
  }
}

extern "C" {

const char* pnp_last_error(void) { return g_error.c_str(); }

int32_t pnp_view_poses(const mcba_view_pose_problem* p, double* poses, double* sse, int32_t* n_used, uint8_t* status,
                       int32_t pairwise) {
  try {
    ViewPlan plan;
    if (!p || !poses || !sse || !n_used || !status) { g_error = "null argument"; return 1; }
    if (!plan_views(*p, plan, g_error)) return 1;
    fill_invalid(*p, plan, poses, sse, n_used, status);
    if (pairwise) run<PairwiseReducer>(*p, plan, poses, sse, n_used, status);
    else run<SerialReducer>(*p, plan, poses, sse, n_used, status);
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}

// one pixel through the undistortion: returns 1 when it converged
int32_t pnp_undistort(const double* block, int32_t n_dist, int32_t fisheye, int32_t fix_aspect, double u, double v, double* xy) {
  double e[CAM_STRIDE];
  camera_entry(block, fisheye ? 4 : n_dist, 0.0, fix_aspect != 0, e, fisheye != 0);
  return undistort_point(e, fisheye ? 4 : n_dist, fisheye != 0, u, v, xy[0], xy[1]) ? 1 : 0;
}

}
