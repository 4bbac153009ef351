// mcba_recon_kernels.h -- k_reconstruction_uncertainty, the kernel of mcba_recon.h.
//
//   * ONE WAVEFRONT serves a tile of 16 consecutive points of one job (single-wave workgroups, as k_residual_gram); the tiles of all
//     jobs form one list (tile_first), grid-strided above 2^20 workgroups, the job of a tile found by bisection (uniform), as in
//     k_projection_uncertainty;
//   * front, FP64 VALU: lane 16 s + p takes point p of the tile and camera slot 4 round + s: Y, project_padded, J_c, P_c, and writes
//     B_c = J_c^T P_c into the stage S[coordinate i][point p][k = 24 slot + column] (48 rows of 24 G columns, row stride 24 G + 4: the
//     MFMA's operand reads hit every bank twice, the floor of a 64-lane 8-byte read) and its J_c^T J_c beside it.  A slot that is
//     no view of the point, and a point past the end of the job, leave zero rows.  Lanes p < 16 add the round's J_c^T J_c to their H
//     in slot order (G = 8: two rounds); then they factor it, write status, n_views, the view mask and cov_noise, and leave H^-1, the
//     status and Y_a in LDS;
//   * product, v_mfma_f64_16x16x4_f64: per tile of 16 columns of the factor three accumulators (one per coordinate), 6 G k-steps:
//     A = S[i][csub][4 ks + rsub], B = W[(4 ks + rsub) ldw + 16 ct + csub] from global memory (the job's [24 G][ldw] factor, zero-
//     padded to ldw = 16 ceil(r / 16): no load has a bounds test; at most 192 KiB, L2-resident), the six loads of the next camera in
//     flight under the 18 MFMAs of the current one.  D row = (lane >> 4) + 4 q, column = lane & 15: a lane holds u_x, u_y, u_z of
//     the same four (point, column) entries, so
//   * tail, in-lane: z = -H^-1 u (+ the reference term from the six pose rows of a), z z^T into the lane's four 6-vectors.  After the
//     last column tile the 16 lanes of a point are summed through LDS in the order csub = 0 .. 15 by one lane, which stores cov_cal:
//     the 16 interleaved partial sums mcba_recon.h states, the same bytes on every call.  Padded columns contribute exactly 0.
// Every register array is indexed by unrolled constants: no scratch.  No atomics, no cross-block waits; nothing is read or written
// past a job's last point.
#pragma once
#include <hip/hip_runtime.h>
#include "mcba_recon.h"

namespace mcba {
namespace recon {

struct KernelArgs {
  int n_jobs;
  const double* recs;                 // [n_jobs][JR_STRIDE]
  const double* wdev;                 // the jobs' factors [24 G][ldw], one after the other
  const long long* w_first;           // [n_jobs] where a job's factor starts
  const long long* first;             // [n_jobs + 1] first point of every job
  const long long* tile_first;        // [n_jobs + 1]
  const double* points;               // [N][3]
  const unsigned long long* masks;    // [N] or null
  double sigma2;
  double* cov_cal;                    // [N][6]
  double* cov_noise;                  // [N][6]
  int32_t* n_views;                   // [N]
  unsigned long long* views;          // [N]
  uint8_t* status;                    // [N]
};

constexpr int RC_TILE = 16, RC_THREADS = 64;
constexpr long long RC_MAX_GRID = 1 << 20;

typedef double rc_double4 __attribute__((ext_vector_type(4)));   // accumulator of v_mfma_f64_16x16x4_f64

__host__ __device__ constexpr int stage_stride(int G) { return KC * G + 4; }

// GM: the widest group of the call (4 or 8) -- it sizes the stage
template <int GM>
__global__ __launch_bounds__(RC_THREADS) void k_reconstruction_uncertainty(KernelArgs a) {
  __shared__ double S[48 * stage_stride(GM)];     // the stage; after the product: the partial sums [16][16][6]
  __shared__ double Hs[64 * 6];                   // J^T J of the round's (slot, point) lanes
  __shared__ double Pt[16 * 9];                   // H^-1 | Y_a of a point
  __shared__ int Vf[64];                          // the lane's (slot, point) is a view
  __shared__ int St[16];                          // status of a point; -1: past the end of the job
  static_assert(16 * 16 * 6 <= 48 * stage_stride(2), "the partial sums fit the smallest stage");
  const int lane = threadIdx.x, rsub = lane >> 4, csub = lane & 15;
  const long long tiles = a.tile_first[a.n_jobs];
  const double nan = undistort::quiet_nan();
  bool first_round = true;
  for (long long b = blockIdx.x; b < tiles; b += gridDim.x) {       // (uniform per workgroup: the barriers are safe)
    if (!first_round) __syncthreads();
    first_round = false;
    int lo = 0, hi = a.n_jobs;                                      // the last job whose first tile is <= b
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (a.tile_first[mid] <= b) lo = mid; else hi = mid;
    }
    const int j = lo;
    const double* rec = a.recs + (size_t)j * JR_STRIDE;
    const double* Wj = a.wdev + a.w_first[j];
    const int G = (int)rec[JR_G], ldw = (int)rec[JR_LDW], ref = (int)rec[JR_REF];
    const int ld = stage_stride(G);
    const double margin = rec[JR_MARGIN];
    // ---- front: lane (s = rsub, p = csub)
    const long long i0 = (b - a.tile_first[j]) * RC_TILE + csub;
    const bool valid = i0 < a.first[j + 1] - a.first[j];
    const size_t at = (size_t)(a.first[j] + (valid ? i0 : 0));
    double X[3] = {0.0, 0.0, 0.0};
    unsigned long long mask = 0;
    if (valid) {
      X[0] = a.points[3 * at]; X[1] = a.points[3 * at + 1]; X[2] = a.points[3 * at + 2];
      mask = a.masks != nullptr ? a.masks[at] : ~0ull;
    }
    double H[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                   // lanes p < 16: the running sums of their point
    int n = 0;
    unsigned long long views = 0;
    bool loose = false;
    for (int round = 0; 4 * round < G; ++round) {
      if (round > 0) __syncthreads();                               // (the sums of the round before are taken)
      const int slot = 4 * round + rsub;
      if (slot < G) {
        View v;
        const bool is_view = ((mask >> slot) & 1) != 0 && view_of_point(slot_of(rec, slot), margin, X, v);
        double* row = S + csub * ld + KC * slot;
        double* h = Hs + lane * 6;
        if (is_view) {
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < KC; ++k) row[i * 16 * ld + k] = b_entry(v, i, k);
          double hv[6];
          view_H(v, hv);
#pragma unroll
          for (int i = 0; i < 6; ++i) h[i] = hv[i];
        } else {
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < KC; ++k) row[i * 16 * ld + k] = 0.0;
        }
        Vf[lane] = is_view ? 1 : 0;
      }
      __syncthreads();
      if (lane < 16) {
        for (int s = 0; s < 4 && 4 * round + s < G; ++s) {          // slot order
          if (Vf[s * 16 + lane] == 0) continue;
          const double* h = Hs + (s * 16 + lane) * 6;
#pragma unroll
          for (int i = 0; i < 6; ++i) H[i] += h[i];
          ++n;
          views |= 1ull << (4 * round + s);
          loose = loose || slot_of(rec, 4 * round + s)[SL_LOOSE] != 0.0;
        }
      }
    }
    if (lane < 16) {
      int status = -1;
      if (valid) {
        Point pt;
        point_H(rec, X, H, n, views, loose, pt);
        status = pt.status;
        double cn[6];
        if (status == ST_OK) {
          noise_covariance(rec, pt, a.sigma2, cn);
#pragma unroll
          for (int i = 0; i < 6; ++i) Pt[lane * 9 + i] = pt.Hi[i];
#pragma unroll
          for (int i = 0; i < 3; ++i) Pt[lane * 9 + 6 + i] = pt.Ya[i];
        } else {
#pragma unroll
          for (int i = 0; i < 6; ++i) cn[i] = nan;
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) a.cov_noise[6 * at + i] = cn[i];
        a.n_views[at] = n;
        a.views[at] = views;
        a.status[at] = (uint8_t)status;
      }
      St[lane] = status;
    }
    __syncthreads();
    // ---- product and tail: lane (rsub, csub) holds rows rsub + 4 q, column 16 ct + csub
    Point pq[4];
    bool ok[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p = rsub + 4 * q;
      ok[q] = St[p] == ST_OK;
#pragma unroll
      for (int i = 0; i < 6; ++i) pq[q].Hi[i] = ok[q] ? Pt[p * 9 + i] : 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) pq[q].Ya[i] = ok[q] ? Pt[p * 9 + 6 + i] : 0.0;
    }
    double c[4][6];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < 6; ++i) c[q][i] = 0.0;
    const double* sp = S + csub * ld + rsub;
    for (int ct = 0; 16 * ct < ldw; ++ct) {
      const double* wp = Wj + (size_t)rsub * ldw + 16 * ct + csub;
      rc_double4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = acc0, acc2 = acc0;
      double w[6], wn[6];
#pragma unroll
      for (int u = 0; u < 6; ++u) w[u] = wp[(size_t)(4 * u) * ldw];
      double pose[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (ref >= 0) {
#pragma unroll
        for (int m = 0; m < 6; ++m) pose[m] = Wj[(size_t)(KC * ref + KI + m) * ldw + 16 * ct + csub];
      }
      for (int g = 0; g < G; ++g) {
        const int gn = g + 1 < G ? g + 1 : g;                       // (the last camera loads its own rows again: in bounds)
#pragma unroll
        for (int u = 0; u < 6; ++u) wn[u] = wp[(size_t)(KC * gn + 4 * u) * ldw];
#pragma unroll
        for (int u = 0; u < 6; ++u) {
          const int k = KC * g + 4 * u;
          acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(sp[k], w[u], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(sp[16 * ld + k], w[u], acc1, 0, 0, 0);
          acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(sp[32 * ld + k], w[u], acc2, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 6; ++u) w[u] = wn[u];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (!ok[q]) continue;
        const double u[3] = {acc0[q], acc1[q], acc2[q]};
        double z[3];
        response(rec, pq[q], u, pose, z);
        add_outer(z, c[q]);
      }
    }
    __syncthreads();                                                // (every lane is done with the stage)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < 6; ++i) S[((rsub + 4 * q) * 16 + csub) * 6 + i] = c[q][i];
    __syncthreads();
    if (lane < 16 && valid) {
      double out[6];
      if (St[lane] == ST_OK) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          double s = S[(lane * 16) * 6 + i];
          for (int l = 1; l < LANES; ++l) s += S[(lane * 16 + l) * 6 + i];
          out[i] = s;
        }
      } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) out[i] = nan;
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) a.cov_cal[6 * at + i] = out[i];
    }
  }
}

void recon_launch(const KernelArgs& a, long long tiles, int max_group, hipStream_t st);   // mcba_recon.hip

}  // namespace recon
}  // namespace mcba
