// translation unit of k_hand_eye (mcba_handeye_kernels.h) and the host driver of mcba_hand_eye
#include "mcba_host.h"
#include "mcba_handeye_driver.h"
#include "mcba_handeye_kernels.h"

namespace mcba {
namespace handeye {

void hand_eye_launch(const HandEyeArgs& a, hipStream_t st) {
  if (a.n_problems <= 0) return;
  const dim3 grid(a.n_problems), block(64);
  hipLaunchKernelGGL(k_hand_eye, grid, block, 0, st, a);
}

}  // namespace handeye
}  // namespace mcba

using namespace mcba;
using namespace mcba::host;

// plan | uploads | kernel | downloads; problems
MCBA_TIMING_GETTER(mcba_debug_hand_eye_ms, g_hand_eye_timing, 4)

extern "C" {

namespace {
void hand_eye(const mcba_hand_eye_problem& p, double* X, double* Z, int32_t* n_pairs, uint8_t* status, double* err) {
  DeviceCall call(g_hand_eye_timing);   // (before the buffers: see the type)
  handeye::Plan plan;
  std::string msg;
  if (!handeye::plan_problems(p, plan, msg)) throw Error(msg);
  handeye::fill_defaults(p, plan, X, Z, n_pairs, status, err);
  call.tm.reset();
  if (p.n_problems == 0 || plan.usable == 0) return call.record();   // nothing to solve: nothing is launched, the device is not touched
  call.open();
  const hipStream_t st = call.st;
  const size_t np_ = (size_t)p.n_problems, F = (size_t)p.F, na = (size_t)p.n_a * F, nb = (size_t)p.n_b * F;
  DevBuf<double> d_ta(na * 16), d_tb, d_out(np_ * 32);              // d_out: X [np][16] | Z [np][16]
  DevBuf<uint8_t> d_va(na), d_vb, d_status(np_);
  DevBuf<int32_t> d_idx(2 * np_), d_n(np_);                          // d_idx: index_a [np] | index_b [np]
  if (!plan.same_table) {
    d_tb.alloc(nb * 16, false);
    d_vb.alloc(nb, false);
  }
  OutBuf<double> o_err(err, np_ * F);
  call.stamp();
  upload_async(d_ta, p.table_a, na * 16, st);   // (the buffers are sized above: nothing is allocated here)
  upload_async(d_va, p.valid_a, na, st);
  if (!plan.same_table) {
    upload_async(d_tb, p.table_b, nb * 16, st);
    upload_async(d_vb, p.valid_b, nb, st);
  }
  upload_to(d_idx.p, p.index_a, np_, st);
  upload_to(d_idx.p + np_, p.index_b, np_, st);
  HIP_OK(hipStreamSynchronize(st));
  call.stamp();
  handeye::HandEyeArgs a;
  a.n_problems = p.n_problems; a.F = p.F; a.invert = p.invert_inputs != 0 ? 1 : 0;
  a.table_a = d_ta.p; a.valid_a = d_va.p;
  a.table_b = plan.same_table ? d_ta.p : d_tb.p; a.valid_b = plan.same_table ? d_va.p : d_vb.p;
  a.index_a = d_idx.p; a.index_b = d_idx.p + np_;
  a.X = d_out.p; a.Z = d_out.p + np_ * 16; a.n_pairs = d_n.p; a.status = d_status.p; a.err = o_err.dev();
  handeye::hand_eye_launch(a, st);
  check_launch("k_hand_eye");
  HIP_OK(hipStreamSynchronize(st));
  call.stamp();
  if (X) download_async(X, d_out.p, np_ * 16, st);
  if (Z) download_async(Z, d_out.p + np_ * 16, np_ * 16, st);
  if (n_pairs) download_async(n_pairs, d_n.p, np_, st);
  if (status) download_async(status, d_status.p, np_, st);
  o_err.fetch(st);
  HIP_OK(hipStreamSynchronize(st));
  call.tm.count = (int64_t)np_;
  call.record();
  const double* ms = call.tm.ms;
  if (getenv("MCBA_TIMING"))
    fprintf(stderr, "[hand_eye] %lld problems, %lld usable pairs, %d frames a row: plan %.2f ms, uploads (%.1f MB) %.2f ms, "
            "kernel %.2f ms, downloads %.2f ms\n", (long long)np_, plan.usable, p.F, ms[0],
            (double)((plan.same_table ? na : na + nb) * 129) / 1e6, ms[1], ms[2], ms[3]);
  call.finish();
}
}  // namespace

int32_t mcba_hand_eye(const mcba_hand_eye_problem* p, double* X, double* Z, int32_t* n_pairs, uint8_t* status, double* err) {
  API_BEGIN
  REQUIRE(p, "null argument");
  hand_eye(*p, X, Z, n_pairs, status, err);
  API_END
}

}  // extern "C"
