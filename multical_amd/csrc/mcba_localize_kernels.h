// mcba_localize_kernels.h -- k_rig_pose<ROLLING>, the kernel of mcba_localize.h: ONE WORKGROUP OF 256 THREADS PER FRAME, the whole
// Levenberg-Marquardt loop of the frame in one launch.  The only synchronisation is __syncthreads: no workgroup waits for another,
// no floating-point atomics, every sum has a fixed order -- two calls return the same bits.
//
//   * the camera records (camera entry | camera pose, localize::REC_STRIDE doubles each) are staged in LDS once and read at the
//     address the observation's camera index selects; the frame's pose entries (R | t | L of start and end) sit in LDS too and are
//     read at wave-uniform addresses;
//   * linearisation: the four waves take the frame's records in chunks of 64, round-robin.  Lane l forms the two rows [J | r] of its
//     observation in registers (7 or 13 entries each), stages them through LDS (128 rows a wave at a stride of 17 doubles: the
//     columns K + 1 .. 15 stay zero, the operand reads of a half-wave fall on 33 consecutive doubles, one two-way conflict in 32
//     lanes) and the wave accumulates the 16 x 16 Gram matrix with v_mfma_f64_16x16x4_f64, operand lane l holding
//     V[4 s + (l >> 4)][l & 15] and result register r of lane l entry (4 r + (l >> 4), l & 15), as k_calibrate_camera does.  One
//     tile holds J^T J, J^T r and r^T r.  The four wave tiles are added in wave order through LDS;
//   * thread 0 factors and solves (localize::damped_step, well_posed, covariance: plain loops over LDS arrays) and broadcasts the
//     step through LDS; every thread then reads the same flags, so the control flow of localize::solve_frame is uniform;
//   * a trial cost is a residual-only pass over the records (L2-resident: a frame of 2 000 observations is 48 KB), lane partials
//     folded by the xor butterfly, wave sums added in wave order;
//   * the start without `init`: thread 0 picks up to four of the frame's views from what k_view_pose left on the device, threads
//     0 .. 3 turn them into rig candidates, and the workgroup scores all of them in one pass over the records.
#pragma once
#include <hip/hip_runtime.h>
#include "mcba_localize.h"
#include "mcba_pnp_kernels.h"

namespace mcba {
namespace localize {

struct RigPoseArgs {
  int C, F, max_iter;
  double sigma_px;
  const double* recs;          // [C][REC_STRIDE]
  const int32_t* first;        // [F + 1]
  const double* uv;            // [N][2]
  const int32_t* ocam;         // [N]
  const int32_t* owpt;         // [N]
  const double* W;             // [B P][3]
  const double* init;          // [F][16] or null: start from the views
  const double* init_end;      // [F][16] or null
  const int32_t* view_first;   // [F + 1]            (start from the views)
  const int32_t* view_desc;    // [views][2]
  const double* view_pose;     // [views][16]
  const int32_t* view_n;       // [views]
  const uint8_t* view_status;  // [views]
  const double* cam_inv;       // [C][12]
  const double* board_inv;     // [B][12]
  double* poses;               // [F][16]
  double* poses_end;           // [F][16] or null
  double* cov;                 // [F][K (K + 1) / 2] or null
  double* sse;                 // [F] or null
  int32_t* iters;              // [F] or null
  double* err;                 // [N] or null
  uint8_t* status;             // [F]
};

constexpr int RIG_THREADS = 256, RIG_WAVES = RIG_THREADS / 64;
constexpr int LDV = 17, STAGE = 128 * LDV;
// LDS of k_rig_pose, in doubles
constexpr int L_G = 0, L_WG = L_G + GS * GS, L_A = L_WG + RIG_WAVES * GS * GS, L_P = L_A + MAX_K * MAX_K, L_Q = L_P + MAX_K,
              L_D = L_Q + MAX_K, L_PE = L_D + MAX_K, L_QE = L_PE + 2 * POSE_STRIDE, L_CAND = L_QE + 2 * POSE_STRIDE,
              L_SC = L_CAND + MAX_CANDIDATES * POSE_STRIDE, L_COV = L_SC + 32, L_STAGE = L_COV + 80,
              L_REC = L_STAGE + RIG_WAVES * STAGE;
static_assert(L_STAGE % 2 == 0 && n_cov(MAX_K) <= 80, "layout of the LDS of k_rig_pose");
inline size_t rig_lds_bytes(int C) { return ((size_t)L_REC + (size_t)C * REC_STRIDE) * sizeof(double); }

// the device back-end of localize::solve_frame: every method is called by all threads of the workgroup
template <bool ROLLING>
struct DeviceBackend {
  static constexpr int K = ROLLING ? 12 : 6;
  double* lds;
  FrameObs o;
  int tid, wave, lane;

  __device__ const double* rec(int i) const { return lds + L_REC + (size_t)o.cam[i] * REC_STRIDE; }
  __device__ double* sc() const { return lds + L_SC; }

  // pose entries of the parameters x (threads 0 and, rolling, 1); the caller synchronises
  __device__ void entries(const double* x, double* e) const {
    if (tid < (ROLLING ? 2 : 1)) pose_entry(x + 6 * tid, e + POSE_STRIDE * tid);
  }

  __device__ double linearize() {
    double* V = lds + L_STAGE + wave * STAGE;
    const double* pe = lds + L_PE;
    const int rsub = lane >> 4, csub = lane & 15;
    pnp::wave_double4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int base = wave * 64; base < o.n; base += RIG_THREADS) {
      const int i = base + lane;
      double ru[K + 1], rv[K + 1];
      if (i < o.n) {
        obs_rows<ROLLING>(rec(i), pe, o.W + 3 * (size_t)o.wpt[i], o.uv[2 * i], o.uv[2 * i + 1], ru, rv);
      } else {
#pragma unroll
        for (int q = 0; q <= K; ++q) ru[q] = rv[q] = 0.0;
      }
#pragma unroll
      for (int q = 0; q <= K; ++q) { V[(2 * lane) * LDV + q] = ru[q]; V[(2 * lane + 1) * LDV + q] = rv[q]; }
      pnp::wave_fence();
      const int rows = 2 * min(64, o.n - base), nsteps = (rows + 3) >> 2;
      const double* vp = V + rsub * LDV + csub;
      for (int st = 0; st < nsteps; ++st) {
        const double a0 = vp[(4 * st) * LDV];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, a0, acc, 0, 0, 0);
      }
      pnp::wave_fence();
    }
    double* T = lds + L_WG + wave * GS * GS;
#pragma unroll
    for (int r = 0; r < 4; ++r) T[(rsub + 4 * r) * GS + csub] = acc[r];
    __syncthreads();
    const double* T0 = lds + L_WG;
    lds[L_G + tid] = ((T0[tid] + T0[GS * GS + tid]) + T0[2 * GS * GS + tid]) + T0[3 * GS * GS + tid];
    __syncthreads();
    return lds[L_G + K * GS + K];
  }

  __device__ bool well_posed() {
    if (tid == 0) sc()[0] = localize::well_posed(K, lds + L_G, lds + L_A) ? 1.0 : 0.0;
    __syncthreads();
    const bool ok = sc()[0] != 0.0;
    __syncthreads();
    return ok;
  }

  __device__ bool solve(double lambda, double* whitened) {
    if (tid == 0) {
      double w = 0.0;
      double* d = lds + L_D;
      const bool ok = damped_step(K, lds + L_G, lambda, lds + L_A, d, &w);
      if (ok)
        for (int i = 0; i < K; ++i) lds[L_Q + i] = lds[L_P + i] + d[i];
      sc()[0] = ok ? 1.0 : 0.0;
      sc()[1] = w;
    }
    __syncthreads();
    const bool ok = sc()[0] != 0.0;
    *whitened = sc()[1];
    if (ok) entries(lds + L_Q, lds + L_QE);
    __syncthreads();
    return ok;
  }

  // cost at the pose entries e; err (or null): per-record error; *behind: a record at or behind its camera
  __device__ double cost_at(const double* e, double* err, bool* behind) {
    double s = 0.0;
    bool any = false;
    for (int i = tid; i < o.n; i += RIG_THREADS) {
      bool b;
      const double t = obs_sq<ROLLING>(rec(i), e, o.W + 3 * (size_t)o.wpt[i], o.uv[2 * i], o.uv[2 * i + 1], &b);
      s += t;
      any = any || b;
      if (err) err[i] = sqrt(t);
    }
    s = pnp::wave_xor_sum(s);
    const bool wave_any = __ballot(any) != 0ull;
    if (lane == 0) { sc()[8 + wave] = s; sc()[12 + wave] = wave_any ? 1.0 : 0.0; }
    __syncthreads();
    const double total = ((sc()[8] + sc()[9]) + sc()[10]) + sc()[11];
    *behind = sc()[12] != 0.0 || sc()[13] != 0.0 || sc()[14] != 0.0 || sc()[15] != 0.0;
    __syncthreads();
    return total;
  }
  __device__ double trial_cost() {
    bool b;
    return cost_at(lds + L_QE, nullptr, &b);
  }

  __device__ void accept() {
    if (tid < K) lds[L_P + tid] = lds[L_Q + tid];
    if (tid < 2 * POSE_STRIDE) lds[L_PE + tid] = lds[L_QE + tid];
    __syncthreads();
  }

  // the start from the views: p <- parameters of the best candidate.  false: the frame has no start
  __device__ bool start_from_views(const RigPoseArgs& a, int f) {
    const int v0 = a.view_first[f], nv = a.view_first[f + 1] - v0;
    int* picks = (int*)(lds + L_A);                     // (scratch: nothing else uses it yet)
    if (tid == 0) sc()[0] = (double)select_views(nv, a.view_status + v0, a.view_n + v0, picks);
    __syncthreads();
    const int nc = (int)sc()[0];
    if (tid < nc) {
      const int v = v0 + picks[tid];
      double pose[16], p6[6];
      view_candidate(a.cam_inv + 12 * (size_t)a.view_desc[2 * v], a.view_pose + 16 * (size_t)v, a.board_inv + 12 * (size_t)a.view_desc[2 * v + 1],
                     pose);
      pose_to_entry(pose, p6, lds + L_CAND + tid * POSE_STRIDE);
#pragma unroll
      for (int i = 0; i < 6; ++i) lds[L_WG + tid * 6 + i] = p6[i];                        // (parameters of candidate tid)
    }
    __syncthreads();
    if (nc == 0) return false;
    double s[MAX_CANDIDATES] = {0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < o.n; i += RIG_THREADS) {
#pragma unroll
      for (int k = 0; k < MAX_CANDIDATES; ++k)
        if (k < nc) s[k] += candidate_term(rec(i), lds + L_CAND + k * POSE_STRIDE, o.W + 3 * (size_t)o.wpt[i], o.uv[2 * i], o.uv[2 * i + 1]);
    }
#pragma unroll
    for (int k = 0; k < MAX_CANDIDATES; ++k) {
      const double t = pnp::wave_xor_sum(s[k]);
      if (lane == 0) sc()[16 + 4 * wave + k] = t;
    }
    __syncthreads();
    double scores[MAX_CANDIDATES];
#pragma unroll
    for (int k = 0; k < MAX_CANDIDATES; ++k) scores[k] = ((sc()[16 + k] + sc()[20 + k]) + sc()[24 + k]) + sc()[28 + k];
    const int best = pick_candidate(scores, nc);
    if (best >= 0 && tid < K) lds[L_P + tid] = lds[L_WG + best * 6 + (tid % 6)];       // (rolling: end = start)
    __syncthreads();
    return best >= 0;
  }
};

template <bool ROLLING>
__global__ __launch_bounds__(RIG_THREADS) void k_rig_pose(RigPoseArgs a) {
  extern __shared__ __attribute__((aligned(16))) double rig_lds[];
  constexpr int K = ROLLING ? 12 : 6, KC = n_cov(K);
  double* lds = rig_lds;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int i0 = a.first[f], n = a.first[f + 1] - i0;
  DeviceBackend<ROLLING> be{lds, FrameObs{a.uv + 2 * (size_t)i0, a.ocam + i0, a.owpt + i0, a.W, n}, tid, tid >> 6, tid & 63};
  double* err = a.err ? a.err + i0 : nullptr;
  // what a frame without a result returns; everything below is uniform over the workgroup
  int status = ST_OK, iters = 0;
  bool have = false, converged = false;
  if (n < min_observations(ROLLING)) {
    status = ST_TOO_FEW;
  } else {
    for (int i = tid; i < a.C * REC_STRIDE; i += RIG_THREADS) lds[L_REC + i] = a.recs[i];
    for (int i = tid; i < RIG_WAVES * STAGE; i += RIG_THREADS) lds[L_STAGE + i] = 0.0;
    __syncthreads();
    bool started = true;
    if (a.init) {
      if (tid == 0) intr::pose_to_params(a.init + 16 * (size_t)f, lds + L_P);
      if (ROLLING && tid == 1) intr::pose_to_params((a.init_end ? a.init_end : a.init) + 16 * (size_t)f, lds + L_P + 6);
      __syncthreads();
    } else {
      started = be.start_from_views(a, f);
    }
    if (!started) {
      status = ST_DEGENERATE;
    } else {
      be.entries(lds + L_P, lds + L_PE);
      __syncthreads();
      double cost = 0.0;
      converged = solve_frame(be, n, a.max_iter, &have, &iters, &cost);
      if (!have) status = ST_DEGENERATE;
    }
  }
  if (!have) {
    for (int i = tid; i < n; i += RIG_THREADS)
      if (err) err[i] = 0.0;
    if (tid < 16) {
      const double v = (tid % 5 == 0) ? 1.0 : 0.0;
      a.poses[16 * (size_t)f + tid] = v;
      if (a.poses_end) a.poses_end[16 * (size_t)f + tid] = v;
    }
    if (a.cov)
      for (int i = tid; i < KC; i += RIG_THREADS) a.cov[(size_t)f * KC + i] = undistort::quiet_nan();
    if (tid == 0) {
      if (a.sse) a.sse[f] = 0.0;
      if (a.iters) a.iters[f] = iters;
      a.status[f] = (uint8_t)status;
    }
    return;
  }
  bool behind = false;
  const double sse = be.cost_at(lds + L_PE, err, &behind);
  if (tid == 0) {
    double* cov = lds + L_COV;
    for (int i = 0; i < KC; ++i) cov[i] = undistort::quiet_nan();
    covariance(K, lds + L_G, pixel_variance(a.sigma_px, sse, n, K), lds + L_A, cov);
  }
  __syncthreads();
  if (tid < 16) {
    // rotation and translation straight from the pose entry: R [9] | t [3]
    const int r = tid >> 2, c = tid & 3;
    const double* pe = lds + L_PE;
    a.poses[16 * (size_t)f + tid] = r == 3 ? (c == 3 ? 1.0 : 0.0) : (c == 3 ? pe[POSE_T + r] : pe[POSE_R + 3 * r + c]);
    if (a.poses_end) {
      const double* qe = pe + POSE_STRIDE;
      const double ident = (tid % 5 == 0) ? 1.0 : 0.0;
      a.poses_end[16 * (size_t)f + tid] =
          !ROLLING ? ident : r == 3 ? (c == 3 ? 1.0 : 0.0) : (c == 3 ? qe[POSE_T + r] : qe[POSE_R + 3 * r + c]);
    }
  }
  if (a.cov)
    for (int i = tid; i < KC; i += RIG_THREADS) a.cov[(size_t)f * KC + i] = lds[L_COV + i];
  if (tid == 0) {
    if (a.sse) a.sse[f] = sse;
    if (a.iters) a.iters[f] = iters;
    a.status[f] = (uint8_t)(behind ? ST_BEHIND : converged ? ST_OK : ST_NOT_CONVERGED);
  }
}

hipError_t rig_pose_launch(const RigPoseArgs& a, bool rolling, hipStream_t st);   // mcba_localize.hip

}  // namespace localize
}  // namespace mcba
