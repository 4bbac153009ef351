// translation unit of k_rig_gram, k_focus_gram, k_rig_assemble, k_rig_score and k_rig_base_add (mcba_rigview_kernels.h) and the host
// driver of mcba_rig_view_information
#include "mcba_host.h"
#include "mcba_rigview_driver.h"
#include "mcba_rigview_kernels.h"

namespace mcba {
namespace rigview {

void gram_launch(const GramArgs& a, int n_launch, hipStream_t st) {
  if (n_launch <= 0) return;
  hipLaunchKernelGGL(k_rig_gram, dim3(n_launch), dim3(GRAM_THREADS), 0, st, a);
}

void focus_launch(const FocusArgs& a, int n_pairs, hipStream_t st) {
  if (n_pairs <= 0) return;
  hipLaunchKernelGGL(k_focus_gram, dim3(n_pairs), dim3(FOCUS_THREADS), 0, st, a);
}

void assemble_launch(const AssembleArgs& a, int n_views, hipStream_t st) {
  if (n_views <= 0) return;
  hipLaunchKernelGGL(k_rig_assemble, dim3(n_views), dim3(ASM_THREADS), 0, st, a);
}

void score_launch(const ScoreArgs& a, int n_entries, hipStream_t st) {
  if (n_entries <= 0) return;
  const size_t bytes = score_lds_doubles(a.r) * sizeof(double);
  if (bytes > 65536) {
    // (more than the default 64 KiB: the request goes through the function attribute, and a refusal is this call's error)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_rig_score), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      throw host::Error(std::string("mcba_rig_view_information: k_rig_score needs ") + std::to_string(bytes) +
                        " bytes of LDS, which this device refuses: " + hipGetErrorString(e));
    }
  }
  hipLaunchKernelGGL(k_rig_score, dim3(n_entries), dim3(SCORE_THREADS), bytes, st, a);
}

void base_add_launch(const double* S_winner, double* B, int r, int rs, double inv_s2, hipStream_t st) {
  hipLaunchKernelGGL(k_rig_base_add, dim3((r * r + 255) / 256), dim3(256), 0, st, S_winner, B, r, rs, inv_s2);
}

}  // namespace rigview
}  // namespace mcba

using namespace mcba;
using namespace mcba::host;

// uploads | the kernels and the scoring rounds (events) | downloads | whole call; slots launched
MCBA_TIMING_GETTER(mcba_debug_rig_view_information_ms, g_rigview_timing, 4)

namespace {

// the device back-end of rigview::greedy_rounds: the A stay on the device, a round moves its scores down
struct DeviceRounds {
  const rigview::Plan& plan;
  hipStream_t st;
  rigview::ScoreArgs args;
  double* d_B;
  double* d_posterior;
  DevBuf<double>& d_scores;          // half log det | focus of the list
  std::vector<double> scores;

  const double* half_log_det() const { return scores.data(); }
  const double* focus() const { return scores.data() + plan.entries.size(); }
  void score(size_t n_entries, bool with_posterior) {
    const size_t ne = plan.entries.size();
    args.half_log_det = d_scores.p;
    args.focus = d_scores.p + ne;
    args.posterior = with_posterior ? d_posterior : nullptr;
    rigview::score_launch(args, (int)n_entries, st);
    check_launch("k_rig_score");
    download_async(scores.data(), d_scores.p, n_entries, st);
    download_async(scores.data() + ne, d_scores.p + ne, n_entries, st);
    HIP_OK(hipStreamSynchronize(st));
  }
  void add(int winner) {
    const size_t rr = (size_t)plan.rs * plan.rs;
    rigview::base_add_launch(args.S + (size_t)winner * rr, d_B, plan.r, plan.rs, plan.inv_s2, st);
  }
};

void run_rig(const mcba_camera_set* cams, const double* camera_poses, int32_t r, const mcba_rig_camera* info, int32_t boards,
             int32_t n_boards, int32_t board_stride, const int32_t* board_n, const double* board_points, int32_t n_views,
             const mcba_rig_view* views, int32_t min_cameras, double margin, double sigma2, const mcba_rig_focus* focus, int32_t n_picks,
             int32_t criterion, int32_t workspace_mb, const mcba_rig_result* out) {
  DeviceCall call(g_rigview_timing);   // (before the buffers: see the type)
  call.tm.reset();
  rigview::Plan plan;
  std::string msg;
  if (!rigview::plan_rig(cams, camera_poses, r, info, boards, n_boards, board_stride, board_n, board_points, n_views, views, min_cameras,
                         margin, sigma2, focus, n_picks, criterion, workspace_mb, out, plan, msg))
    throw Error(msg);
  rigview::fill_defaults(plan, out);
  if (plan.nothing) return;             // nothing is launched, the device is not touched
  const size_t V = (size_t)plan.V, C = (size_t)plan.C, rr = (size_t)plan.rs * plan.rs, ne = plan.entries.size();
  const size_t np = (size_t)plan.n_pairs, KK = (size_t)rigview::KP * rigview::KP;
  DevBuf<double> d_crecs, d_srecs, d_board, d_W, d_frecs, d_G, d_H, d_S, d_B, d_Q, d_scores, d_posterior;
  DevBuf<int32_t> d_launch, d_entries, d_nvis, d_ncam, d_nok;
  DevBuf<uint8_t> d_loose, d_status;
  call.open(2);
  upload_vector(d_crecs, plan.crecs, call.st);
  upload_vector(d_srecs, plan.srecs, call.st);
  upload_vector(d_board, plan.board_points, call.st);
  upload_vector(d_W, plan.W, call.st);
  upload_vector(d_frecs, plan.frecs, call.st);
  upload_vector(d_launch, plan.launch, call.st);
  upload_vector(d_entries, plan.entries, call.st);
  upload_vector(d_loose, plan.loose, call.st);
  std::vector<double> B0(rr, 0.0);
  for (int i = 0; i < plan.r; ++i) B0[(size_t)i * plan.rs + i] = 1.0;
  upload_vector(d_B, B0, call.st);
  d_G.alloc(V * C * rigview::KC * rigview::KC, false);
  d_nvis.alloc(V * C, true);
  d_H.alloc(np * KK, false);
  d_nok.alloc(np, true);
  d_S.alloc(V * rr, true);
  d_ncam.alloc(V, true);
  d_status.alloc(V, true);
  d_Q.alloc(rr, true);
  d_posterior.alloc(rr, true);
  d_scores.alloc(2 * ne, false);
  rigview::GramArgs ga{};
  ga.launch = d_launch.p; ga.srecs = d_srecs.p; ga.crecs = d_crecs.p; ga.board_points = d_board.p; ga.board_stride = plan.board_stride;
  ga.G = d_G.p; ga.n_visible = d_nvis.p;
  rigview::FocusArgs fa{};
  fa.frecs = d_frecs.p; fa.gw = plan.gw; fa.n = plan.gn; fa.u0 = plan.u0; fa.v0 = plan.v0; fa.du = plan.du; fa.dv = plan.dv;
  fa.H = d_H.p; fa.n_ok = d_nok.p;
  rigview::AssembleArgs aa{};
  aa.C = plan.C; aa.r = plan.r; aa.rs = plan.rs; aa.min_cameras = plan.min_cameras; aa.srecs = d_srecs.p; aa.G = d_G.p;
  aa.n_visible = d_nvis.p; aa.W = d_W.p; aa.loose = d_loose.p; aa.S = d_S.p; aa.n_cameras = d_ncam.p; aa.status = d_status.p;
  call.mark(0);
  rigview::gram_launch(ga, (int)plan.launch.size(), call.st);
  check_launch("k_rig_gram");
  rigview::focus_launch(fa, plan.n_pairs, call.st);
  check_launch("k_focus_gram");
  rigview::assemble_launch(aa, plan.V, call.st);
  check_launch("k_rig_assemble");
  // the focus: the pairs' Gram matrices come down, Q goes up
  std::vector<double> H(np * KK), Q(rr, 0.0);
  std::vector<int32_t> nok(np, 0);
  int n_focus = 0;
  if (np > 0) {
    download_async(H.data(), d_H.p, H.size(), call.st);
    download_async(nok.data(), d_nok.p, np, call.st);
    HIP_OK(hipStreamSynchronize(call.st));
    rigview::fold_focus(plan, H.data(), Q.data());
    for (int32_t n : nok) n_focus += n;
    upload_to(d_Q.p, Q.data(), rr, call.st);
  }
  const int fstatus = focus ? rigview::focus_status(plan, n_focus) : rigview::ST_TOO_FEW;
  rigview::ScoreArgs sc{};
  sc.r = plan.r; sc.rs = plan.rs; sc.ld = rigview::score_stride(plan.r); sc.entries = d_entries.p; sc.S = d_S.p; sc.status = d_status.p;
  sc.B = d_B.p; sc.Q = fstatus == rigview::ST_OK ? d_Q.p : nullptr; sc.n_focus = (double)n_focus; sc.inv_s2 = plan.inv_s2;
  DeviceRounds rounds{plan, call.st, sc, d_B.p, d_posterior.p, d_scores, std::vector<double>(2 * ne, 0.0)};
  rigview::greedy_rounds(plan, rounds, out);
  call.mark(1);
  call.end_kernels("k_rig_score");
  std::vector<int32_t> nvis(V * C), ncam(V);
  std::vector<uint8_t> status(V);
  download_async(nvis.data(), d_nvis.p, V * C, call.st);
  download_async(ncam.data(), d_ncam.p, V, call.st);
  download_async(status.data(), d_status.p, V, call.st);
  if (out->A) download_async(out->A, d_S.p, V * rr, call.st);
  if (out->posterior) download_async(out->posterior, d_posterior.p, rr, call.st);
  HIP_OK(hipStreamSynchronize(call.st));
  for (size_t v = 0; v < V; ++v) { out->n_cameras[v] = ncam[v]; out->status[v] = status[v]; }
  for (size_t i = 0; i < V * C; ++i) out->n_visible[i] = nvis[i];
  if (out->Q) for (size_t i = 0; i < rr; ++i) out->Q[i] = Q[i];
  if (out->focus_status) *out->focus_status = (uint8_t)fstatus;
  if (out->focus_n) *out->focus_n = n_focus;
  call.finish((int64_t)plan.launch.size());
}

}  // namespace

extern "C" {

int32_t mcba_rig_view_information(const mcba_camera_set* cams, const double* camera_poses, int32_t r, const mcba_rig_camera* info,
                                  int32_t boards, int32_t n_boards, int32_t board_stride, const int32_t* board_n,
                                  const double* board_points, int32_t n_views, const mcba_rig_view* views, int32_t min_cameras,
                                  double margin, double sigma2, const mcba_rig_focus* focus, int32_t n_picks, int32_t criterion,
                                  int32_t workspace_mb, const mcba_rig_result* out) {
  API_BEGIN
  run_rig(cams, camera_poses, r, info, boards, n_boards, board_stride, board_n, board_points, n_views, views, min_cameras, margin, sigma2,
          focus, n_picks, criterion, workspace_mb, out);
  API_END
}

}  // extern "C"
