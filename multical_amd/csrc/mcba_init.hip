// translation unit of the pose alignment kernels (mcba_init_kernels.h) and the host driver of mcba_align_poses_*
#include <atomic>

#include "../../include/mcba.h"
#include "mcba_host.h"
#include "mcba_init_kernels.h"

using namespace mcba;
using namespace mcba::host;

extern "C" {

/* matrix.align_transforms_robust (transform/matrix.py:140-153) for a BATCH of problems on the device: the numeric core of
 * tables.estimate_transform (tables.py:153-176) and tables.relative_between_n (tables.py:334-345).  No handle: the
 * initialisation runs before a Calibration exists.  nA / nB = poses in A / B (ia, ib == nullptr: one per entry).
 * The stream and every buffer of a call are parked in the resource cache and taken back by the next call of the same
 * shape (an initialisation makes three calls; created and freed anew they cost 18 of its 32 ms at 16 x 1000 x 5). */
namespace {
void align_poses(int32_t n_problems, const int64_t* offsets, const double* A, int64_t nA, const int32_t* ia, const double* B,
                 int64_t nB, const int32_t* ib, const uint8_t* mask, double threshold, int32_t invert, double* out,
                 uint8_t* out_valid, uint8_t* inliers) {
  REQUIRE(n_problems >= 0 && offsets && A && B && out && out_valid, "bad argument");
  if (n_problems == 0) return;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    throw Error("no HIP device: the mcba back-end is GPU-only (there is no CPU fallback)");
  const int64_t total = offsets[n_problems];
  int64_t nmax = 1;
  for (int p = 0; p < n_problems; ++p) {
    REQUIRE(offsets[p + 1] >= offsets[p], "offsets must be non-decreasing");
    nmax = std::max<int64_t>(nmax, offsets[p + 1] - offsets[p]);
  }
  REQUIRE(offsets[0] == 0 && total >= 0, "offsets must start at 0");
  REQUIRE(nmax < (1ll << 24), "more than 2^24 pose pairs in one alignment problem");
  REQUIRE((ia == nullptr) == (ib == nullptr), "both index lists or none");
  if (ia != nullptr) {
    REQUIRE(nA > 0 && nB > 0 && nA < (1ll << 31) && nB < (1ll << 31), "bad pose table size");
    for (int64_t k = 0; k < total; ++k)
      REQUIRE(ia[k] >= 0 && ia[k] < nA && ib[k] >= 0 && ib[k] < nB, "pose index out of range");
  }
  const bool timing = getenv("MCBA_TIMING") != nullptr;
  CallTiming untimed;   // (this family has no mcba_debug_*_ms entry)
  DeviceCall call(untimed);   // (before the buffers: see the type)
  call.open();
  const hipStream_t st = call.st;
  const double t0 = call.t[0];
  DevBuf<long long> d_off, d_prof;
  DevBuf<double> dA, dB, d_out, d_f64;
  DevBuf<uint8_t> d_mask, d_valid, d_inl;
  DevBuf<int> d_i32;
  DevBuf<int32_t> d_ia, d_ib;
  d_off.alloc((size_t)n_problems + 1, false);
  {
    static_assert(sizeof(long long) == sizeof(int64_t), "offsets are copied as they are");
    upload_to(d_off.p, (const long long*)offsets, (size_t)n_problems + 1, st);
  }
  const size_t tot = (size_t)std::max<int64_t>(total, 1);
  const size_t cntA = ia ? (size_t)nA : tot, cntB = ib ? (size_t)nB : tot;
  dA.alloc(16 * cntA, false);
  const bool same_table = ia != nullptr && A == B && nA == nB;
  if (!same_table) dB.alloc(16 * cntB, false);
  if (total > 0) {
    upload_to(dA.p, A, 16 * (ia ? (size_t)nA : (size_t)total), st);
    if (!same_table) upload_to(dB.p, B, 16 * (ib ? (size_t)nB : (size_t)total), st);
    if (ia != nullptr) {
      d_ia.alloc(tot, false);
      d_ib.alloc(tot, false);
      upload_to(d_ia.p, ia, (size_t)total, st);
      upload_to(d_ib.p, ib, (size_t)total, st);
    }
  }
  if (mask) {
    d_mask.alloc(tot, false);
    if (total > 0) upload_to(d_mask.p, mask, (size_t)total, st);
  }
  d_out.alloc(16 * (size_t)n_problems, false);
  d_valid.alloc((size_t)n_problems, false);
  d_inl.alloc(tot, false);
  // per-problem scratch: 14 doubles + 7 ints per entry, sized for the largest problem
  const size_t per = (size_t)nmax, np_ = (size_t)n_problems;
  d_f64.alloc(np_ * per * 14, false);
  d_i32.alloc(np_ * per * 7, false);
  AlignScratch sc;
  sc.vec = d_f64.p;
  sc.cen = sc.vec + np_ * per * 6;
  sc.err = sc.cen + np_ * per * 6;
  sc.hgt = sc.err + np_ * per;
  sc.nd = sc.err;   // (nearest-neighbour distances of the clustering rounds: the error array is idle while a clustering runs)
  sc.size = d_i32.p;
  sc.chain = sc.size + np_ * per;
  sc.rep_a = sc.chain + np_ * per;
  sc.rep_b = sc.rep_a + np_ * per;
  sc.parent = sc.rep_b + np_ * per;
  sc.list = sc.parent + np_ * per;
  sc.live = sc.list + np_ * per;
  static const bool align_prof = dbg_switch("MCBA_ALIGN_PROF") != nullptr;
  sc.prof = nullptr;
  if (align_prof) {
    d_prof.alloc(np_ * 32);
    sc.prof = d_prof.p;
  }
  // dynamic LDS for the clustering state of problems with up to lds_cap selected entries (small batches of big problems get
  // the full 125 KB; batches of many small problems only what their largest problem needs, so that several fit a CU)
  // (a batch with a problem of more than ALIGN_LDS_CAP entries takes the full size: its error array -- 8 B per entry, up to
  //  18 150 entries -- is ranked from LDS too)
  const int lds_cap = (int)std::min<int64_t>(nmax, ALIGN_LDS_CAP);
  const size_t lds = align_lds_bytes(lds_cap);
  // (a per-DEVICE attribute: set on every call, it costs nothing next to the copies)
  HIP_OK(hipFuncSetAttribute((const void*)k_align_robust, hipFuncAttributeMaxDynamicSharedMemorySize, (int)align_lds_bytes(ALIGN_LDS_CAP)));
  const double t1 = now_seconds();
  static const bool no_staged = dbg_switch("MCBA_ALIGN_MONOLITHIC") != nullptr;
  // (the partial winners of the split scans take 24 B x ALIGN_SCAN_Z per entry and problem: batches beyond 4 M entries x problems
  //  -- 1.6 GB of them -- stay with the one-workgroup kernel)
  if (nmax > ALIGN_STAGED_MIN && n_problems <= 4096 && (size_t)n_problems * (size_t)nmax <= ((size_t)1 << 22) && !align_prof &&
      !no_staged) {
    // large problems: the rounds of the clustering as separate launches, the scans spread over the chip (k_align_stage_*)
    DevBuf<AlignStage> d_stage;
    DevBuf<int> d_done, d_pi;
    DevBuf<double> d_pf;
    d_stage.alloc(np_, true);
    d_done.alloc(2, true);
    d_pf.alloc(2 * np_ * ALIGN_SCAN_Z * per, false);     // partial winners of the split scans: key | d^2
    d_pi.alloc(2 * np_ * ALIGN_SCAN_Z * per + 2 * np_ * per, false);     // slot | size; + changed | work list
    PinnedBuf prog(64);
    unsigned long long* h_prog = (unsigned long long*)prog.p;
    static std::atomic<unsigned long long> call_counter{0};
    AlignArgs a;
    a.off = d_off.p; a.A = dA.p; a.B = same_table ? dA.p : dB.p; a.ia = ia ? d_ia.p : nullptr; a.ib = ib ? d_ib.p : nullptr;
    a.mask = mask ? d_mask.p : nullptr; a.threshold = threshold; a.invert = (int)invert; a.scratch_stride = (long long)per;
    a.base = sc; a.out = d_out.p; a.out_valid = d_valid.p; a.inliers = d_inl.p; a.st = d_stage.p; a.done_count = d_done.p;
    a.host_progress = h_prog;
    a.pkey = d_pf.p; a.pd2 = d_pf.p + np_ * ALIGN_SCAN_Z * per; a.pidx = d_pi.p; a.pn = d_pi.p + np_ * ALIGN_SCAN_Z * per;
    a.changed = d_pi.p + 2 * np_ * ALIGN_SCAN_Z * per; a.work = a.changed + np_ * per;
    const int scan_y = (int)std::max<int64_t>(1, std::min<int64_t>(64, (nmax + 255) / 256));
    for (int pass = 0; pass < 2; ++pass) {
      const unsigned long long call_id = (++call_counter) & 0xffffull;
      *h_prog = 0ull;
      HIP_OK(hipMemsetAsync(d_done.p, 0, sizeof(int), st));
      hipLaunchKernelGGL(k_align_stage_pre, dim3(n_problems), dim3(ALIGN_THREADS), 0, st, a, pass);
      check_launch("k_align_stage_pre");
      // rounds: enqueued a few ahead of the progress word [call | problems whose clustering ended | round] that block 0 of every
      // merge kernel stores (kernels of finished problems return at once; at most nmax rounds can be needed)
      constexpr int LOOKAHEAD = 8;
      int enqueued = 0, seen_round = 0, spins = 0;
      double t_wait = 0.0;
      while (true) {
        const unsigned long long w = __atomic_load_n(h_prog, __ATOMIC_ACQUIRE);
        if ((w >> 48) == call_id) {
          const int rd = (int)(w & 0xffffffull);
          if (rd != seen_round) { seen_round = rd; t_wait = 0.0; spins = 0; }
          if ((int)((w >> 24) & 0xffffffull) >= n_problems) break;
        }
        if (enqueued - seen_round < LOOKAHEAD && enqueued <= nmax + 1) {
          hipLaunchKernelGGL(k_align_stage_scan, dim3(n_problems, scan_y, ALIGN_SCAN_Z), dim3(256), 0, st, a);
          ++enqueued;
          hipLaunchKernelGGL(k_align_stage_merge, dim3(n_problems), dim3(ALIGN_THREADS), 0, st, a, call_id, enqueued);
          if ((enqueued & 15) == 0) check_launch("k_align_stage rounds");
          t_wait = 0.0;
          spins = 0;
          continue;
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
        if ((++spins & 1023) == 0) {
          const double now = now_seconds();
          if (t_wait == 0.0) t_wait = now;
          else if (now - t_wait > 0.05) {   // (a failed launch must not hang the caller)
            HIP_OK(hipStreamSynchronize(st));
            const unsigned long long w2 = __atomic_load_n(h_prog, __ATOMIC_ACQUIRE);
            REQUIRE((w2 >> 48) == call_id && ((int)(w2 & 0xffffffull) != seen_round || (int)((w2 >> 24) & 0xffffffull) >= n_problems),
                    "the staged alignment made no progress");
            t_wait = 0.0;
          }
        }
      }
      hipLaunchKernelGGL(k_align_stage_post, dim3(n_problems), dim3(ALIGN_THREADS), 0, st, a, pass);
      check_launch("k_align_stage_post");
    }
    download_async(out, d_out.p, 16 * (size_t)n_problems, st);
    download_async(out_valid, d_valid.p, (size_t)n_problems, st);
    if (inliers && total > 0) download_async(inliers, d_inl.p, (size_t)total, st);
    HIP_OK(hipStreamSynchronize(st));
    if (timing) {
      std::vector<AlignStage> hs(np_);
      HIP_OK(hipMemcpy(hs.data(), d_stage.p, np_ * sizeof(AlignStage), hipMemcpyDeviceToHost));
      long long sl = 0, sw = 0, rd = 0;
      for (const AlignStage& q : hs) { sl += q.sum_live; sw += q.sum_work; rd = std::max<long long>(rd, q.rounds); }
      fprintf(stderr, "[align_poses] %d problems, %lld entries (staged): buffers + uploads %.2f ms, kernels + downloads %.2f ms; "
              "rounds of the last pass <= %lld, clusters alive / scanning summed over rounds %lld / %lld\n",
              n_problems, (long long)total, (t1 - t0) * 1e3, (now_seconds() - t1) * 1e3, rd, sl, sw);
    }
    call.finish();
    return;
  }
  hipLaunchKernelGGL(k_align_robust, dim3(n_problems), dim3(ALIGN_THREADS), lds, st, d_off.p, dA.p,
                     (const double*)(same_table ? dA.p : dB.p), (const int32_t*)(ia ? d_ia.p : nullptr),
                     (const int32_t*)(ib ? d_ib.p : nullptr), (const uint8_t*)(mask ? d_mask.p : nullptr), threshold, (int)invert,
                     (long long)per, sc, d_out.p, d_valid.p, d_inl.p, lds_cap);
  check_launch("k_align_robust");
  download_async(out, d_out.p, 16 * (size_t)n_problems, st);
  download_async(out_valid, d_valid.p, (size_t)n_problems, st);
  if (inliers && total > 0) download_async(inliers, d_inl.p, (size_t)total, st);
  HIP_OK(hipStreamSynchronize(st));
  if (timing)
    fprintf(stderr, "[align_poses] %d problems, %lld entries: buffers + uploads %.2f ms, kernel + downloads %.2f ms\n", n_problems,
            (long long)total, (t1 - t0) * 1e3, (now_seconds() - t1) * 1e3);
  if (align_prof) {   // phase cycles of the largest problem
    std::vector<long long> hp(np_ * 32);
    HIP_OK(hipMemcpy(hp.data(), d_prof.p, hp.size() * sizeof(long long), hipMemcpyDeviceToHost));
    int big = 0;
    for (int p = 1; p < n_problems; ++p)
      if (offsets[p + 1] - offsets[p] > offsets[big + 1] - offsets[big]) big = p;
    const char* names[9] = {"compaction", "relative poses", "robust mean", "errors", "quantile + test", "  whitening", "  clustering",
                            "  cut+labels+mean", "  rounds (count)"};
    for (int pass = 0; pass < 2; ++pass)
      for (int k = 0; k < 9; ++k)
        fprintf(stderr, "[k_align_robust] problem %d (n = %lld) pass %d %-18s %10lld\n", big,
                (long long)(offsets[big + 1] - offsets[big]), pass, names[k], hp[(size_t)big * 32 + 16 * pass + k]);
  }
  call.finish();
}
}  // namespace

int32_t mcba_align_poses_robust(int32_t n_problems, const int64_t* offsets, const double* A, const double* B,
                                const uint8_t* mask, double threshold, int32_t invert, double* out, uint8_t* out_valid,
                                uint8_t* inliers) {
  API_BEGIN
  align_poses(n_problems, offsets, A, 0, nullptr, B, 0, nullptr, mask, threshold, invert, out, out_valid, inliers);
  API_END
}

int32_t mcba_align_poses_indexed(int32_t n_problems, const int64_t* offsets, const double* table_a, int64_t n_a,
                                 const int32_t* index_a, const double* table_b, int64_t n_b, const int32_t* index_b,
                                 const uint8_t* mask, double threshold, int32_t invert, double* out, uint8_t* out_valid,
                                 uint8_t* inliers) {
  API_BEGIN
  REQUIRE(index_a && index_b, "null index list");
  align_poses(n_problems, offsets, table_a, n_a, index_a, table_b, n_b, index_b, mask, threshold, invert, out, out_valid, inliers);
  API_END
}

}  // extern "C"
