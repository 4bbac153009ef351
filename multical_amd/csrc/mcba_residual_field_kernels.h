// Kernels of the residual field (mcba_residual_gram): the Gram matrices of the rows [b(u, v) | r_x | r_y] of
// mcba_residual_field.h, one symmetric NC x NC block per (camera, fold = frame mod n_folds).  Not templated on the camera family or
// the motion model: the projected points and the valid mask come from k_residual (the buffers of mcba_project /
// mcba_reprojection_error, reference [C,F,B,P] order), the observed points and the inlier bytes from the handle's frame-major tables.
//
//   k_residual_gram       ONE WAVEFRONT PER (camera, fold, frame chunk).  The wave walks the B P slots of its frames in rounds of
//                         RG_GROUPS groups of 64 (the loads of a round are in flight together: a single-wave workgroup has nobody
//                         to hide a round trip behind) and ballot-compacts the participating ones (valid, inlier if inliers_only,
//                         observed pixel inside the image) in slot order into a pending list, as k_obscov compacts a view's
//                         slots; every 64 pending slots become one dense chunk:
//                         lane i writes the 18 non-zero entries of row i into the staging buffer V [64][RG_LD] (which is zero
//                         everywhere else), the upper 16 x 16 tiles of V^T V below ceil(NC / 16) are accumulated by
//                         v_mfma_f64_16x16x4_f64 -- the staged-rows-to-MFMA idiom of wave_gram_tiles (mcba_gram_front.h) at 64
//                         columns, 10 tiles instead of 3 -- and lane i takes its 18 entries back out.  The last chunk of a wave is
//                         short: its rows beyond the count are the zeros that are already there, and the k-loop stops at
//                         ceil(n / 4).  The tiles leave as the wave's partial, [10][16][16] doubles.
//                         Coverage counts: integer atomics, LDS first, then one global add per non-empty cell and workgroup
//                         (integers are associative: the maps do not depend on the order).
//   k_residual_gram_fold  one workgroup per (camera, fold, upper tile): entry e of the tile summed over the chunk partials in chunk
//                         order (k_obscov_fold's pattern: one order, the same bytes on every call, eight independent loads in
//                         flight), written to [NC][NC] with its mirror image; entries of the padded tiles beyond NC are dropped.
//                         Row counts and the outside counts (integers) are summed by the first tile's workgroup.
//
// CHUNKING RULE: nch = min(frames of the largest fold, ceil(RG_TARGET_GROUPS / (C n_folds))) frame chunks per (camera, fold), the
// frames of a fold dealt to them in contiguous runs of ceil(frames of the fold / nch).  A workgroup holds 40 KB of LDS, so four
// single-wave workgroups are resident per CU, one per SIMD: 1024 on the 256 CUs.  RG_TARGET_GROUPS = 2048 launches twice that: the
// rows of a chunk vary by a factor of about three between cameras and frames, and the dispatcher hands the queued workgroups to the
// SIMDs that finish first (measured at 8 x 500 x 2: 176 us with 1024, 155 us with 2048).  8 cameras x 5 folds get 52 chunks of 2 frames
// at 500 frames.  The partials cost nch x 20 KB per (camera, fold) of HBM traffic, written once and read once.
// No float atomics, no cross-block waits, no scratch (the accumulators are indexed by unrolled constants).
#pragma once
#include <hip/hip_runtime.h>
#include "mcba_residual_field.h"

namespace mcba {
namespace resfield {

constexpr int RG_LD = 68;                      // row stride of the staging buffer in doubles (64 columns + padding)
constexpr int RG_TILES = 10;                   // upper tiles of a 4 x 4 tile grid
constexpr int RG_PART = RG_TILES * 256;        // doubles of a workgroup's partial
constexpr int RG_TARGET_GROUPS = 2048;
constexpr int RG_GROUPS = 4;                  // groups of 64 slots whose loads are in flight together
constexpr int RG_PEND = 64 * (RG_GROUPS + 1);  // pending list: fewer than 64 left over + the groups of one round

typedef double rg_double4 __attribute__((ext_vector_type(4)));   // accumulator of v_mfma_f64_16x16x4_f64

struct GramArgs {
  const double* proj;          // [C,F,B,P,2] projected points (k_residual)
  const uint8_t* valid;        // [C,F,B,P]   the mask of mcba_reprojection_error
  const double2* obs;          // [F][C][B][P] observed points (the handle's table)
  const uint8_t* inlier;       // [F][C][B][P]
  const int32_t* image_size;   // [C][2] W, H
  int C, F, BP;                // B * P slots per (camera, frame)
  int nx, ny, n_folds, nch, inliers_only;
  int cov_w, cov_h;            // 0, 0: no coverage maps
  double* part;                // [C][n_folds][nch][RG_PART]
  long long* cpart;            // [C][n_folds][nch][2] rows that entered, slots outside the image
  int32_t* coverage;           // [C][2][cov_h][cov_w], zero on entry
};

// frame chunks per (camera, fold): the rule at the head of this file
inline int gram_chunks(int C, int F, int n_folds) {
  const int per_fold = (F + n_folds - 1) / n_folds;
  const int want = (RG_TARGET_GROUPS + C * n_folds - 1) / (C * n_folds);
  const int nch = want < per_fold ? want : per_fold;
  return nch < 1 ? 1 : nch;
}

// index of upper tile (ti, tj), ti <= tj < 4
__host__ __device__ constexpr int gram_tile(int ti, int tj) { return ti * 4 - ti * (ti - 1) / 2 + (tj - ti); }

__device__ __forceinline__ void rg_fence() {
  // LDS accesses of one wavefront complete in issue order; the fence stops the compiler from moving them across
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// one dense chunk: the first n <= 64 entries of the pending list pe (entry = f BP + q: frame and slot inside the camera's frame)
template <int NT>
__device__ __forceinline__ void gram_chunk(const GramArgs& a, double* V, const int* pe, int n, int lane, int c, double W, double H,
                                           int K, rg_double4 (&acc)[RG_TILES]) {
  const int rsub = lane >> 4, csub = lane & 15;
  double* row = V + lane * RG_LD;
  int col[16];
  if (lane < n) {
    const int e = pe[lane], f = e / a.BP, q = e - f * a.BP;
    const double2 ob = a.obs[(f * a.C + c) * a.BP + q];
    const size_t ri = (size_t)((c * a.F + f) * a.BP + q);
    const double px = a.proj[2 * ri], py = a.proj[2 * ri + 1];
    double w[16];
    field_row(ob.x, ob.y, W, H, a.nx, a.ny, col, w);
#pragma unroll
    for (int i = 0; i < 16; ++i) row[col[i]] = w[i];
    row[K] = px - ob.x;
    row[K + 1] = py - ob.y;
  }
  rg_fence();
  const int nsteps = (n + 3) >> 2;
  const double* vp = V + rsub * RG_LD + csub;
  for (int st = 0; st < nsteps; ++st) {
    double av[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) av[t] = vp[(4 * st) * RG_LD + 16 * t];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
      for (int tj = ti; tj < NT; ++tj)
        acc[gram_tile(ti, tj)] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[ti], av[tj], acc[gram_tile(ti, tj)], 0, 0, 0);
  }
  rg_fence();
  if (lane < n) {   // the buffer is all zeros again
#pragma unroll
    for (int i = 0; i < 16; ++i) row[col[i]] = 0.0;
    row[K] = 0.0;
    row[K + 1] = 0.0;
  }
  rg_fence();
}

template <int NT>
__global__ __launch_bounds__(64) void k_residual_gram(GramArgs a) {
  __shared__ double V[64 * RG_LD];
  __shared__ int pe[RG_PEND];
  __shared__ int cov[2 * MAX_COV_BINS];
  const int lane = threadIdx.x;
  const int j = blockIdx.x % a.nch, ck = blockIdx.x / a.nch, k = ck % a.n_folds, c = ck / a.n_folds;
  const int nf = k < a.F ? (a.F - k + a.n_folds - 1) / a.n_folds : 0;   // frames k, k + n_folds, ... of the fold
  const int per = (nf + a.nch - 1) / a.nch;
  const int i0 = min(nf, j * per), i1 = min(nf, i0 + per);
  const double W = (double)a.image_size[2 * c], H = (double)a.image_size[2 * c + 1];
  const int K = n_control(a.nx, a.ny), nbins = a.coverage != nullptr ? a.cov_w * a.cov_h : 0;
  for (int e = lane; e < 64 * RG_LD; e += 64) V[e] = 0.0;
  for (int e = lane; e < 2 * nbins; e += 64) cov[e] = 0;
  rg_fence();
  rg_double4 acc[RG_TILES];
#pragma unroll
  for (int t = 0; t < RG_TILES; ++t) acc[t] = rg_double4{0.0, 0.0, 0.0, 0.0};
  int npend = 0;
  long long rows = 0, outc = 0;
  for (int i = i0; i < i1; ++i) {
    const int f = k + i * a.n_folds;
    const int bs = (f * a.C + c) * a.BP, br = (c * a.F + f) * a.BP;
    for (int q0 = 0; q0 < a.BP; q0 += 64 * RG_GROUPS) {
      // the loads of RG_GROUPS groups of 64 slots are in flight together; then their ballots, one after the other (slot order)
      bool v[RG_GROUPS], in[RG_GROUPS];
      double2 ob[RG_GROUPS];
#pragma unroll
      for (int u = 0; u < RG_GROUPS; ++u) {
        const int q = q0 + 64 * u + lane;
        const int qc = q < a.BP ? q : 0;
        v[u] = a.valid[br + qc] != 0;
        in[u] = a.inlier[bs + qc] != 0;
        ob[u] = a.obs[bs + qc];
      }
#pragma unroll
      for (int u = 0; u < RG_GROUPS; ++u) {
        const int q = q0 + 64 * u + lane;
        const bool val = q < a.BP && v[u];
        const bool cand = val && (in[u] || a.inliers_only == 0);
        const bool ins = inside_image(ob[u].x, ob[u].y, W, H);
        if (nbins > 0 && val && ins)
          atomicAdd(&cov[(in[u] ? 0 : nbins) + coverage_bin(ob[u].y, H, a.cov_h) * a.cov_w + coverage_bin(ob[u].x, W, a.cov_w)], 1);
        outc += __popcll(__ballot(cand && !ins));
        const bool act = cand && ins;
        const unsigned long long m = __ballot(act);
        if (act) pe[npend + __popcll(m & ((1ull << lane) - 1ull))] = f * a.BP + q;
        npend += __popcll(m);
      }
      rg_fence();
      int head = 0;
      for (; npend >= 64; npend -= 64, head += 64) {
        gram_chunk<NT>(a, V, pe + head, 64, lane, c, W, H, K, acc);
        rows += 64;
      }
      if (head > 0) {   // the rest (fewer than 64) moves to the front of the list
        const int rest = lane < npend ? pe[head + lane] : 0;
        rg_fence();
        if (lane < npend) pe[lane] = rest;
        rg_fence();
      }
    }
  }
  if (npend > 0) {
    gram_chunk<NT>(a, V, pe, npend, lane, c, W, H, K, acc);
    rows += npend;
  }
  const int rsub = lane >> 4, csub = lane & 15;
  double* out = a.part + (size_t)blockIdx.x * RG_PART;
#pragma unroll
  for (int ti = 0; ti < NT; ++ti)
#pragma unroll
    for (int tj = ti; tj < NT; ++tj)
#pragma unroll
      for (int q = 0; q < 4; ++q) out[gram_tile(ti, tj) * 256 + (rsub + 4 * q) * 16 + csub] = acc[gram_tile(ti, tj)][q];
  if (lane == 0) {
    a.cpart[2 * (size_t)blockIdx.x] = rows;
    a.cpart[2 * (size_t)blockIdx.x + 1] = outc;
  }
  for (int e = lane; e < 2 * nbins; e += 64) {
    const int n = cov[e];
    if (n != 0) atomicAdd(&a.coverage[(size_t)c * 2 * nbins + e], n);
  }
}

// grid (C n_folds, upper tiles of the ceil(NC / 16)^2 tile grid); gram [C][n_folds][NC][NC], count [C][n_folds], outside [C] (zero on entry)
__global__ __launch_bounds__(256) void k_residual_gram_fold(GramArgs a, double* __restrict__ gram, long long* __restrict__ count,
                                                           unsigned long long* __restrict__ outside) {
  constexpr int UB = 8;
  const int tid = threadIdx.x, r = tid >> 4, cc = tid & 15;
  const int NC = n_control(a.nx, a.ny) + 2, NT = (NC + 15) / 16;
  int ti = 0, y = blockIdx.y;   // upper tile blockIdx.y of the NT x NT tile grid, row by row
  while (y >= NT - ti) {
    y -= NT - ti;
    ++ti;
  }
  const int tj = ti + y;
  const size_t first = (size_t)blockIdx.x * a.nch;
  const double* p = a.part + first * RG_PART + gram_tile(ti, tj) * 256 + tid;
  double sum = 0.0;
  for (int j0 = 0; j0 < a.nch; j0 += UB) {   // chunk order; UB independent loads in flight
    double x[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) x[u] = p[(size_t)min(j0 + u, a.nch - 1) * RG_PART];
#pragma unroll
    for (int u = 0; u < UB; ++u)
      if (j0 + u < a.nch) sum += x[u];
  }
  const int row = 16 * ti + r, col = 16 * tj + cc;
  if (row <= col && col < NC) {
    double* G = gram + (size_t)blockIdx.x * NC * NC;
    G[(size_t)row * NC + col] = sum;
    G[(size_t)col * NC + row] = sum;
  }
  if (blockIdx.y == 0 && tid == 0) {
    long long rows = 0, out = 0;
    for (int j = 0; j < a.nch; ++j) {
      rows += a.cpart[2 * (first + j)];
      out += a.cpart[2 * (first + j) + 1];
    }
    count[blockIdx.x] = rows;
    if (out != 0) atomicAdd(&outside[blockIdx.x / a.n_folds], (unsigned long long)out);
  }
}

}  // namespace resfield
}  // namespace mcba
