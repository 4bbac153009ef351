// mcba_uncertainty_kernels.h -- k_projection_uncertainty, the kernel of mcba_uncertainty.h.
//
//   * one query per lane: an exact Newton inverse, one or two analytic projections, then r responses s = J w_j from the structured
//     pieces (Kc_b, A_b, the 3-vector dY, A_xy^-1 Kc_a) accumulated into (uu, uv, vv).  FP64 VALU work; the row pair J is never
//     materialised and nothing is reduced across lanes;
//   * a workgroup of 256 threads serves one tile of 256 consecutive queries of one job; the tiles of all jobs form one list
//     (tile_first), grid-strided above 2^20 workgroups.  A workgroup finds the job of a tile by bisection (uniform);
//   * the job's record (two camera entries, R_ba | t_ba, scalars, the unit columns of unconstrained parameters and W^T: at most
//     19 KiB) is staged in LDS when the job changes and read at wave-uniform addresses: the camera-family switches and the
//     reference branch are wave-uniform, only the status of a query diverges;
//   * the pixel of a query comes from registers (grid: u0 + ix du, v0 + iy dv; 32 bytes written a query, nothing read) or from a
//     list (16 bytes read a lane, contiguous across the wave);
//   * lanes past the end of a job read nothing and write nothing.
// Every array index is a compile-time constant after unrolling (the padded 2 x 18 camera blocks): no scratch.  One barrier pair per
// staged job, no atomics, no cross-block waits.
#pragma once
#include <hip/hip_runtime.h>
#include "mcba_uncertainty.h"

namespace mcba {
namespace uncertainty {

struct KernelArgs {
  int n_jobs;
  const double* recs;            // [n_jobs][REC_STRIDE]
  const long long* first;        // [n_jobs + 1]
  const long long* tile_first;   // [n_jobs + 1]
  const long long* uv_first;     // [n_jobs]; -1: a grid
  const double* grid;            // [n_jobs][4]
  const int32_t* grid_w;         // [n_jobs]
  const double* uv;              // the lists
  double* cov;                   // [n,3]
  double* std;                   // [n] or null
  uint8_t* status;               // [n]
};

constexpr int UNC_THREADS = 256;
constexpr long long UNC_MAX_GRID = 1 << 20;

__global__ __launch_bounds__(UNC_THREADS) void k_projection_uncertainty(KernelArgs a) {
  __shared__ double rec[REC_STRIDE];
  const long long tiles = a.tile_first[a.n_jobs];
  int staged = -1;
  for (long long b = blockIdx.x; b < tiles; b += gridDim.x) {       // (uniform per workgroup: the barriers are safe)
    int lo = 0, hi = a.n_jobs;                                      // the last job whose first tile is <= b
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (a.tile_first[mid] <= b) lo = mid; else hi = mid;
    }
    const int j = lo;
    if (j != staged) {
      if (staged >= 0) __syncthreads();                             // (every lane is done with the previous record)
      const double* src = a.recs + (size_t)j * REC_STRIDE;
      const int count = REC_W + ((int)src[REC_LOOSE] + (int)src[REC_RANK]) * KP;
      for (int i = threadIdx.x; i < count; i += UNC_THREADS) rec[i] = src[i];
      __syncthreads();
      staged = j;
    }
    const long long i = (b - a.tile_first[j]) * UNC_THREADS + threadIdx.x;
    if (i < a.first[j + 1] - a.first[j]) {
      double u, v;
      const long long list = a.uv_first[j];
      if (list < 0) {
        grid_pixel(i, a.grid_w[j], a.grid[4 * j], a.grid[4 * j + 1], a.grid[4 * j + 2], a.grid[4 * j + 3], u, v);
      } else {
        u = a.uv[2 * (list + i)];
        v = a.uv[2 * (list + i) + 1];
      }
      Result r;
      query(rec, u, v, r);
      const size_t slot = (size_t)(a.first[j] + i);
      a.cov[3 * slot] = r.uu;
      a.cov[3 * slot + 1] = r.uv;
      a.cov[3 * slot + 2] = r.vv;
      if (a.std) a.std[slot] = r.std;
      a.status[slot] = (uint8_t)r.status;
    }
  }
}

void uncertainty_launch(const KernelArgs& a, long long tiles, hipStream_t st);       // mcba_uncertainty.hip

}  // namespace uncertainty
}  // namespace mcba
