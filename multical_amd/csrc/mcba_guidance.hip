// translation unit of k_view_schur, k_view_score and k_base_add (mcba_guidance_kernels.h) and the host driver of mcba_view_information
#include "mcba_host.h"
#include "mcba_guidance_driver.h"
#include "mcba_guidance_kernels.h"

namespace mcba {
namespace guidance {

void schur_launch(const SchurArgs& a, int n_launch, hipStream_t st) {
  if (n_launch <= 0) return;
  hipLaunchKernelGGL(k_view_schur, dim3(n_launch), dim3(SCHUR_THREADS), 0, st, a);
}

void score_launch(const ScoreArgs& a, hipStream_t st) {
  if (a.n_entries <= 0) return;
  hipLaunchKernelGGL(k_view_score, dim3((a.n_entries + SCORE_WAVES - 1) / SCORE_WAVES), dim3(SCORE_THREADS), 0, st, a);
}

void base_add_launch(const int32_t* winners, const int32_t* cam_r, const double* S, double* B, int rs, double inv_s2, int C,
                     hipStream_t st) {
  hipLaunchKernelGGL(k_base_add, dim3(C), dim3(64), 0, st, winners, cam_r, S, B, rs, inv_s2);
}

}  // namespace guidance
}  // namespace mcba

using namespace mcba;
using namespace mcba::host;

// uploads | k_view_schur and the scoring rounds (events) | downloads | whole call; views launched
MCBA_TIMING_GETTER(mcba_debug_view_information_ms, g_guidance_timing, 4)

namespace {

// the device back-end of guidance::greedy_rounds: the S stay on the device, a round moves its scores down and its winners up
struct DeviceRounds {
  const guidance::Plan& plan;
  hipStream_t st;
  guidance::ScoreArgs args;
  DevBuf<int32_t>& d_winners;
  const int32_t* d_cam_r;
  double* d_B;
  double* d_posterior;
  DevBuf<double>& d_scores;          // gain | focus of the list
  std::vector<double> scores;

  const double* gain() const { return scores.data(); }
  const double* focus() const { return scores.data() + plan.entries.size(); }
  void score(size_t n_entries, bool with_posterior) {
    const size_t ne = plan.entries.size();
    args.n_entries = (int)n_entries;
    args.gain = d_scores.p;
    args.focus = d_scores.p + ne;
    args.posterior = with_posterior ? d_posterior : nullptr;
    guidance::score_launch(args, st);
    check_launch("k_view_score");
    download_async(scores.data(), d_scores.p, n_entries, st);
    download_async(scores.data() + ne, d_scores.p + ne, n_entries, st);
    HIP_OK(hipStreamSynchronize(st));
  }
  void add(const int32_t* winners) {
    upload_to(d_winners.p, winners, (size_t)plan.C, st);
    guidance::base_add_launch(d_winners.p, d_cam_r, args.S, d_B, plan.rs, plan.inv_s2, plan.C, st);
    HIP_OK(hipStreamSynchronize(st));           // (`winners` is the caller's to change after this)
  }
};

void run_guidance(const mcba_camera_set* cams, const mcba_guidance_camera* info, int32_t n_boards, int32_t board_stride,
                  const int32_t* board_n, const double* board_points, double margin, double sigma2, int32_t n_views,
                  const mcba_guidance_view* views, const mcba_guidance_view* foci, int32_t n_picks, int32_t criterion,
                  const mcba_guidance_result* out) {
  DeviceCall call(g_guidance_timing);   // (before the buffers: see the type)
  call.tm.reset();
  guidance::Plan plan;
  std::string msg;
  if (!guidance::plan_views(cams, info, n_boards, board_stride, board_n, board_points, margin, sigma2, n_views, views, foci, n_picks,
                            criterion, out, plan, msg))
    throw Error(msg);
  guidance::fill_defaults(plan, out);
  if (n_views == 0 || plan.launch.empty()) return;      // nothing is launched, the device is not touched
  const size_t N = (size_t)plan.V + plan.C, rr = (size_t)plan.rs * plan.rs, ne = plan.entries.size();
  DevBuf<double> d_crecs, d_vrecs, d_uv, d_board, d_S, d_B, d_scores, d_posterior;
  DevBuf<int32_t> d_launch, d_entries, d_view_camera, d_cam_r, d_nvis, d_winners;
  DevBuf<uint8_t> d_status;
  call.open(2);
  upload_vector(d_crecs, plan.crecs, call.st);
  upload_vector(d_vrecs, plan.vrecs, call.st);
  upload_vector(d_uv, plan.uv, call.st);
  upload_vector(d_board, plan.board_points, call.st);
  upload_vector(d_launch, plan.launch, call.st);
  upload_vector(d_entries, plan.entries, call.st);
  upload_vector(d_view_camera, plan.view_camera, call.st);
  upload_vector(d_cam_r, plan.cam_r, call.st);
  upload_vector(d_status, plan.status0, call.st);
  std::vector<double> B0((size_t)plan.C * rr, 0.0);
  for (int c = 0; c < plan.C; ++c)
    for (int i = 0; i < plan.cam_r[c]; ++i) B0[c * rr + (size_t)i * plan.rs + i] = 1.0;
  upload_vector(d_B, B0, call.st);
  d_S.alloc(N * rr, true);
  d_nvis.alloc(N, true);
  d_posterior.alloc((size_t)plan.C * rr, true);
  d_scores.alloc(2 * ne, false);
  d_winners.alloc((size_t)plan.C, false);
  guidance::SchurArgs sa{};
  sa.launch = d_launch.p; sa.vrecs = d_vrecs.p; sa.crecs = d_crecs.p; sa.board_points = d_board.p; sa.board_stride = plan.board_stride;
  sa.uv = d_uv.p; sa.rs = plan.rs; sa.S = d_S.p; sa.n_visible = d_nvis.p; sa.status = d_status.p;
  guidance::ScoreArgs sc{};
  sc.n_views = plan.V; sc.rs = plan.rs; sc.entries = d_entries.p; sc.view_camera = d_view_camera.p; sc.cam_r = d_cam_r.p; sc.S = d_S.p;
  sc.n_visible = d_nvis.p; sc.status = d_status.p; sc.B = d_B.p; sc.inv_s2 = plan.inv_s2;
  call.mark(0);
  guidance::schur_launch(sa, (int)plan.launch.size(), call.st);
  check_launch("k_view_schur");
  DeviceRounds rounds{plan, call.st, sc, d_winners, d_cam_r.p, d_B.p, d_posterior.p, d_scores, std::vector<double>(2 * ne, 0.0)};
  guidance::greedy_rounds(plan, rounds, out);
  call.mark(1);
  call.end_kernels("k_view_score");
  std::vector<int32_t> nvis(N);
  std::vector<uint8_t> status(N);
  download_async(nvis.data(), d_nvis.p, N, call.st);
  download_async(status.data(), d_status.p, N, call.st);
  if (out->S) download_async(out->S, d_S.p, (size_t)plan.V * rr, call.st);
  if (out->Q) download_async(out->Q, d_S.p + (size_t)plan.V * rr, (size_t)plan.C * rr, call.st);
  std::vector<double> post(out->posterior ? (size_t)plan.C * rr : 0);
  if (out->posterior) download_async(post.data(), d_posterior.p, post.size(), call.st);
  HIP_OK(hipStreamSynchronize(call.st));
  for (int j = 0; j < plan.V; ++j) { out->n_visible[j] = nvis[j]; out->status[j] = status[j]; }
  for (int c = 0; c < plan.C; ++c) {
    if (out->focus_status) out->focus_status[c] = status[(size_t)plan.V + c];
    if (out->focus_n_visible) out->focus_n_visible[c] = nvis[(size_t)plan.V + c];
    if (out->posterior && plan.cam_served[c])
      for (size_t i = 0; i < rr; ++i) out->posterior[c * rr + i] = post[c * rr + i];
  }
  call.finish((int64_t)plan.launch.size());
}

}  // namespace

extern "C" {

int32_t mcba_view_information(const mcba_camera_set* cams, const mcba_guidance_camera* info, int32_t n_boards, int32_t board_stride,
                              const int32_t* board_n, const double* board_points, double margin, double sigma2, int32_t n_views,
                              const mcba_guidance_view* views, const mcba_guidance_view* foci, int32_t n_picks, int32_t criterion,
                              const mcba_guidance_result* out) {
  API_BEGIN
  run_guidance(cams, info, n_boards, board_stride, board_n, board_points, margin, sigma2, n_views, views, foci, n_picks, criterion, out);
  API_END
}

}  // extern "C"
