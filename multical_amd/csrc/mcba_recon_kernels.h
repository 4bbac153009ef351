// mcba_recon_kernels.h -- k_reconstruction_uncertainty, the kernel of mcba_recon.h, and k_reconstruction_pairs,
// the same tile re-cut for pairs of points.
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
//
// k_reconstruction_pairs: a tile is 8 consecutive PAIRS of one job, row t of the stage the a end of pair t and row 8 + t its b end (a
// point that occurs in several pairs is computed once per occurrence).  Front (rc_front) and product (rc_product) are the ones
// above, said once more as functions: k_reconstruction_uncertainty keeps its own text, so that its instruction stream stays the one
// that was measured.  The front's lanes p < 16 keep cov_noise, the view mask, X and the point's index in LDS instead of storing them.  A lane's
// rows rsub + 4 q are then the a ends (q = 0, 1) and the b ends (q = 2, 3) of ITS two pairs in the same column: the tail forms z_a,
// z_b and d = z_a - z_b in-lane and adds d d^T (6 sums) and z_a z_b^T (9 sums) per pair.  The 16 column lanes of a pair are summed
// through LDS in the order csub = 0 .. 15 by lane t < 8, which finishes the pair (recon::pair_finish) and stores whatever output is
// asked for.  Nothing is read or written past a job's last pair; the pair indices were checked against the job's n on the host.
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

struct PairKernelArgs {
  int n_jobs;
  const double* recs;                 // as above
  const double* wdev;
  const long long* w_first;
  const long long* first;             // [n_jobs + 1] first point of every job
  const long long* pair_first;        // [n_jobs + 1] first pair of every job
  const long long* tile_first;        // [n_jobs + 1] first pair tile of every job
  const double* points;               // [N][3]
  const unsigned long long* masks;    // [N] or null
  const long long* pairs;             // [K][2] indices into the job's own points
  double sigma2;
  // [K] rows; any of them null: not stored
  double* cov_diff_cal;               // [K][6]
  double* cross_cal;                  // [K][9]
  double* cov_diff_noise;             // [K][6]
  double* length;
  double* length_var_cal;
  double* length_var_noise;
  unsigned long long* views_a;
  unsigned long long* views_b;
  uint8_t* status;
};

constexpr int RC_TILE = 16, RC_THREADS = 64, RP_TILE = 8;
constexpr long long RC_MAX_GRID = 1 << 20;

typedef double rc_double4 __attribute__((ext_vector_type(4)));   // accumulator of v_mfma_f64_16x16x4_f64

__host__ __device__ constexpr int stage_stride(int G) { return KC * G + 4; }

// the last job whose first tile is <= b (uniform)
__device__ __forceinline__ int rc_job_of_tile(const long long* tile_first, int n_jobs, long long b) {
  int lo = 0, hi = n_jobs;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tile_first[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

// front of a tile: lane (s = rsub, p = csub) stages B_c of its point X for the slots 4 round + s (zero rows where the slot is no view)
// and lanes p < 16 sum H, the views and the unconstrained flag of their point in slot order.  Ends on a barrier-free statement: the
// caller synchronises before the stage is read.
__device__ __forceinline__ void rc_front(const double* rec, int G, int ld, double margin, const double* X, unsigned long long mask,
                                         double* S, double* Hs, int* Vf, double* H, int& n, unsigned long long& views, bool& loose) {
  const int lane = threadIdx.x, rsub = lane >> 4, csub = lane & 15;
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
}

// product of one tile of 16 columns: acc_i += S[i] W over the 6 G k-steps; sp = S + csub ld + rsub, wp = the lane's first element of W
__device__ __forceinline__ void rc_product(const double* sp, int ld, const double* wp, int ldw, int G, rc_double4& acc0, rc_double4& acc1,
                                           rc_double4& acc2) {
  double w[6], wn[6];
#pragma unroll
  for (int u = 0; u < 6; ++u) w[u] = wp[(size_t)(4 * u) * ldw];
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
}

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

template <int GM>
__global__ __launch_bounds__(RC_THREADS) void k_reconstruction_pairs(PairKernelArgs a) {
  __shared__ double S[48 * stage_stride(GM)];     // the stage; after the product: the partial sums [8][16][15]
  __shared__ double Hs[64 * 6];
  __shared__ double Pt[16 * 9];                   // H^-1 | Y_a of a row's point
  __shared__ double Nz[16 * 6];                   // its cov_noise
  __shared__ double Xs[16 * 3];                   // the point itself
  __shared__ unsigned long long Vw[16];           // its view mask
  __shared__ long long Ix[16];                    // its index in the job
  __shared__ int Vf[64];
  __shared__ int St[16];                          // status of a row's point; -1: the pair is past the end of the job
  static_assert(RP_TILE * 16 * 15 <= 48 * stage_stride(2), "the partial sums fit the smallest stage");
  static_assert(2 * RP_TILE == RC_TILE, "a ends in rows 0 .. 7, b ends in rows 8 .. 15");
  const int lane = threadIdx.x, rsub = lane >> 4, csub = lane & 15;
  const long long tiles = a.tile_first[a.n_jobs];
  bool first_round = true;
  for (long long b = blockIdx.x; b < tiles; b += gridDim.x) {       // (uniform per workgroup: the barriers are safe)
    if (!first_round) __syncthreads();
    first_round = false;
    const int j = rc_job_of_tile(a.tile_first, a.n_jobs, b);
    const double* rec = a.recs + (size_t)j * JR_STRIDE;
    const double* Wj = a.wdev + a.w_first[j];
    const int G = (int)rec[JR_G], ldw = (int)rec[JR_LDW], ref = (int)rec[JR_REF];
    const int ld = stage_stride(G);
    const double margin = rec[JR_MARGIN];
    // ---- front: lane (s = rsub, p = csub), row p = end (p >> 3) of pair (p & 7) of the tile
    const long long k0 = (b - a.tile_first[j]) * RP_TILE + (csub & 7);
    const bool valid = k0 < a.pair_first[j + 1] - a.pair_first[j];
    const size_t pair_at = (size_t)(a.pair_first[j] + (valid ? k0 : 0));
    const long long ix = valid ? a.pairs[2 * pair_at + (csub >> 3)] : 0;
    const size_t at = (size_t)(a.first[j] + ix);
    double X[3] = {0.0, 0.0, 0.0};
    unsigned long long mask = 0;
    if (valid) {
      X[0] = a.points[3 * at]; X[1] = a.points[3 * at + 1]; X[2] = a.points[3 * at + 2];
      mask = a.masks != nullptr ? a.masks[at] : ~0ull;
    }
    double H[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int n = 0;
    unsigned long long views = 0;
    bool loose = false;
    rc_front(rec, G, ld, margin, X, mask, S, Hs, Vf, H, n, views, loose);
    if (lane < 16) {
      int status = -1;
      if (valid) {
        Point pt;
        point_H(rec, X, H, n, views, loose, pt);
        status = pt.status;
        if (status == ST_OK) {
          double cn[6];
          noise_covariance(rec, pt, a.sigma2, cn);
#pragma unroll
          for (int i = 0; i < 6; ++i) Pt[lane * 9 + i] = pt.Hi[i];
#pragma unroll
          for (int i = 0; i < 3; ++i) Pt[lane * 9 + 6 + i] = pt.Ya[i];
#pragma unroll
          for (int i = 0; i < 6; ++i) Nz[lane * 6 + i] = cn[i];
        }
      }
      St[lane] = status;
      Vw[lane] = views;
      Ix[lane] = ix;
#pragma unroll
      for (int i = 0; i < 3; ++i) Xs[lane * 3 + i] = X[i];
    }
    __syncthreads();
    // ---- product and tail: rows rsub + 4 q of column 16 ct + csub: q = 0, 1 the a ends of the pairs rsub, rsub + 4; q = 2, 3 their b ends
    Point pq[4];
    bool ok[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) ok[q] = St[rsub + 4 * q] == ST_OK && St[rsub + 4 * q + RP_TILE] == ST_OK;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p = rsub + 4 * q;
#pragma unroll
      for (int i = 0; i < 6; ++i) pq[q].Hi[i] = ok[q & 1] ? Pt[p * 9 + i] : 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) pq[q].Ya[i] = ok[q & 1] ? Pt[p * 9 + 6 + i] : 0.0;
    }
    double cd[2][6], cx[2][9];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
#pragma unroll
      for (int i = 0; i < 6; ++i) cd[q][i] = 0.0;
#pragma unroll
      for (int i = 0; i < 9; ++i) cx[q][i] = 0.0;
    }
    const double* sp = S + csub * ld + rsub;
    for (int ct = 0; 16 * ct < ldw; ++ct) {
      const double* wp = Wj + (size_t)rsub * ldw + 16 * ct + csub;
      rc_double4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = acc0, acc2 = acc0;
      double pose[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (ref >= 0) {
#pragma unroll
        for (int m = 0; m < 6; ++m) pose[m] = Wj[(size_t)(KC * ref + KI + m) * ldw + 16 * ct + csub];
      }
      rc_product(sp, ld, wp, ldw, G, acc0, acc1, acc2);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (!ok[q]) continue;
        const double ua[3] = {acc0[q], acc1[q], acc2[q]}, ub[3] = {acc0[q + 2], acc1[q + 2], acc2[q + 2]};
        double za[3], zb[3];
        response(rec, pq[q], ua, pose, za);
        response(rec, pq[q + 2], ub, pose, zb);
        add_pair(za, zb, cd[q], cx[q]);
      }
    }
    __syncthreads();                                                // (every lane is done with the stage)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      double* part = S + ((rsub + 4 * q) * 16 + csub) * 15;
#pragma unroll
      for (int i = 0; i < 6; ++i) part[i] = cd[q][i];
#pragma unroll
      for (int i = 0; i < 9; ++i) part[6 + i] = cx[q][i];
    }
    __syncthreads();
    if (lane < RP_TILE && valid) {                                  // lane t: pair t of the tile (its own `valid` is the pair's)
      double sum[15];
#pragma unroll
      for (int i = 0; i < 15; ++i) sum[i] = S[(lane * 16) * 15 + i];
#pragma unroll 1
      for (int l = 1; l < LANES; ++l) {                             // (one column lane at a time: 15 loads in flight, not 240)
#pragma unroll
        for (int i = 0; i < 15; ++i) sum[i] += S[(lane * 16 + l) * 15 + i];
      }
      const int ea = lane, eb = lane + RP_TILE;
      PairResult out;
      pair_finish(rec, Xs + 3 * ea, Xs + 3 * eb, Ix[ea] == Ix[eb], St[ea], St[eb], Nz + 6 * ea, Nz + 6 * eb, sum, sum + 6, out);
      if (a.cov_diff_cal != nullptr) {
#pragma unroll
        for (int i = 0; i < 6; ++i) a.cov_diff_cal[6 * pair_at + i] = out.cov_diff_cal[i];
      }
      if (a.cross_cal != nullptr) {
#pragma unroll
        for (int i = 0; i < 9; ++i) a.cross_cal[9 * pair_at + i] = out.cross_cal[i];
      }
      if (a.cov_diff_noise != nullptr) {
#pragma unroll
        for (int i = 0; i < 6; ++i) a.cov_diff_noise[6 * pair_at + i] = out.cov_diff_noise[i];
      }
      if (a.length != nullptr) a.length[pair_at] = out.length;
      if (a.length_var_cal != nullptr) a.length_var_cal[pair_at] = out.length_var_cal;
      if (a.length_var_noise != nullptr) a.length_var_noise[pair_at] = out.length_var_noise;
      if (a.views_a != nullptr) a.views_a[pair_at] = Vw[ea];
      if (a.views_b != nullptr) a.views_b[pair_at] = Vw[eb];
      if (a.status != nullptr) a.status[pair_at] = (uint8_t)out.status;
    }
  }
}

void recon_launch(const KernelArgs& a, long long tiles, int max_group, hipStream_t st);            // mcba_recon.hip
void recon_pairs_launch(const PairKernelArgs& a, long long tiles, int max_group, hipStream_t st);  // mcba_recon.hip

}  // namespace recon
}  // namespace mcba
