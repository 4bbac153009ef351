// TEST INFRASTRUCTURE: g++ build of the stereo calibration mathematics (multical_amd/csrc/mcba_stereo.h) behind the signature of
// mcba_stereo_calibrate, one plain loop over pairs through the header's SerialBackend.  The argument checks, the views of a pair and
// the scatter of the results come from the same driver header the API uses.  sh_set_device_order switches the summation order of
// the calls that follow: 0 = table order, 1 = the order of k_stereo_pair.
#include <string>
#include <vector>

#include "../../multical_amd/csrc/mcba_stereo_driver.h"

using namespace mcba;
using namespace mcba::stereo;

static thread_local std::string g_error;
static int g_device_order = 0;

namespace {

template <bool DEV>
void run(const mcba_stereo_problem* p, const Plan& plan, double* T, double* cov, double* sse, int32_t* iterations,
         double* view_poses_out, double* view_sse, uint8_t* status) {
  std::vector<double> ws(plan.total_views() * VB_STRIDE, 0.0);
  std::vector<uint8_t> st(plan.n_launched());
  for (size_t i = 0; i < plan.n_launched(); ++i) {
    const size_t k = (size_t)plan.launched[i];
    const int v0 = plan.first[i], nv = plan.first[i + 1] - v0;
    SerialBackend<DEV> be;
    be.t = host_tables(p, plan);
    be.v = PairViews{plan.desc[2 * i], plan.desc[2 * i + 1], nv, plan.slot.data() + v0, plan.n_common.data() + v0, ws.data() + (size_t)v0 * VB_STRIDE};
    int iters = 0;
    bool have = false;
    double cost = 0.0;
    const int s = solve_pair(be, plan.max_iter, &iters, &have, &cost);
    st[i] = status[k] = (uint8_t)s;
    if (iterations) iterations[k] = iters;
    if (!have) continue;
    intr::params_to_pose(be.p, T + 16 * k);
    if (sse) sse[k] = cost;
    if (cov) {
      const double s2 = pixel_variance(p->sigma_px, cost, plan.n_points[k], nv);
      for (int e = 0; e < 36; ++e) cov[36 * k + e] = s2 * be.inv[e];
    }
  }
  scatter_views(plan, ws.data(), st.data(), view_poses_out, view_sse);
}

}  // namespace

extern "C" {

const char* sh_last_error(void) { return g_error.c_str(); }

int32_t sh_set_device_order(int32_t on) {
  g_device_order = on != 0;
  return 0;
}

int32_t sh_stereo_calibrate(const mcba_stereo_problem* p, double* T, double* cov, double* sse, int32_t* n_views, int32_t* n_points,
                            int32_t* iterations, double* view_poses_out, double* view_sse, uint8_t* status) {
  try {
    Plan plan;
    if (!plan_problem(p, T, status, plan, g_error)) return 1;
    fill_unsolved(p, plan, T, cov, sse, n_views, n_points, iterations, view_poses_out, view_sse, status);
    if (g_device_order) run<true>(p, plan, T, cov, sse, iterations, view_poses_out, view_sse, status);
    else run<false>(p, plan, T, cov, sse, iterations, view_poses_out, view_sse, status);
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}

}
