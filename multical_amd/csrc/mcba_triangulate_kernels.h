// mcba_triangulate_kernels.h -- k_triangulate, the kernel of mcba_triangulate.h.
//
//   * one point per lane: 3 unknowns and at most C observations, nothing to reduce across lanes.  FP64 VALU work; no MFMA (the
//     largest product of the kernel is 2 x 3 by 3 x 3);
//   * a workgroup of 256 threads owns one frame and 256 consecutive points of it; the grid is F x ceil(M / 256) workgroups,
//     grid-strided above 2^20;
//   * the frame's C records (camera entry | view matrix | end matrix, triangulate::REC_STRIDE doubles each) are staged in LDS once
//     per workgroup and read at wave-uniform addresses inside the loops over cameras: the camera-family switch is wave-uniform,
//     only the `valid` byte (and what follows from it: the usable-view mask) diverges;
//   * observations are read in place from [C,F,M,2], 16 bytes a lane, contiguous across the wave, and read AGAIN by every pass
//     (L2 serves them): no per-view state in registers, the register count does not depend on C;
//   * lanes past M read nothing and write nothing.
// One barrier pair per workgroup round, no atomics, no cross-block waits.
#pragma once
#include <hip/hip_runtime.h>
#include "mcba_triangulate.h"

namespace mcba {
namespace triangulate {

struct KernelArgs {
  Tables t;
  long long M;                // points per frame
  const double* points;       // [C,F,M,2]
  const uint8_t* valid;       // [C,F,M]
  int rolling;
  double sigma_px;
  int max_iter;               // clamped
  double* X;                  // [F,M,3]
  double* cov;                // [F,M,6] or null
  double* sse;                // [F,M]   or null
  double* err;                // [C,F,M] or null
  int32_t* n_views;           // [F,M]   or null
  uint8_t* status;            // [F,M]
};

constexpr int TRI_THREADS = 256;
constexpr long long TRI_MAX_GRID = 1 << 20;

inline size_t lds_bytes(int C) { return (size_t)C * REC_STRIDE * sizeof(double); }

__global__ __launch_bounds__(TRI_THREADS) void k_triangulate(KernelArgs a) {
  extern __shared__ double recs[];            // [C][REC_STRIDE]
  const int C = a.t.C, F = a.t.F;
  const long long tiles = (a.M + TRI_THREADS - 1) / TRI_THREADS, rounds = tiles * F;
  const size_t FM = (size_t)F * (size_t)a.M;
  for (long long b = blockIdx.x; b < rounds; b += gridDim.x) {      // (uniform per workgroup: the barriers are safe)
    const int f = (int)(b / tiles);
    const long long m = (b - (long long)f * tiles) * TRI_THREADS + threadIdx.x;
    for (int i = threadIdx.x; i < C * REC_STRIDE; i += TRI_THREADS) recs[i] = staged_value(a.t, f, i);
    __syncthreads();
    if (m < a.M) {
      const size_t slot = (size_t)f * (size_t)a.M + (size_t)m;      // point of [F,M]; camera c adds c * FM
      Observations o;
      o.uv = a.points + 2 * slot;
      o.valid = a.valid + slot;
      o.err = a.err ? a.err + slot : nullptr;
      o.uv_stride = 2 * FM;
      o.valid_stride = FM;
      o.err_stride = FM;
      PointResult r;
      triangulate_point(recs, C, a.rolling != 0, o, a.sigma_px, a.max_iter, r);
      a.X[3 * slot] = r.X[0];
      a.X[3 * slot + 1] = r.X[1];
      a.X[3 * slot + 2] = r.X[2];
      if (a.cov) {
#pragma unroll
        for (int i = 0; i < 6; ++i) a.cov[6 * slot + i] = r.cov[i];
      }
      if (a.sse) a.sse[slot] = r.sse;
      if (a.n_views) a.n_views[slot] = r.n_views;
      a.status[slot] = (uint8_t)r.status;
    }
    __syncthreads();                                                // (the next round stages over the records)
  }
}

void triangulate_launch(const KernelArgs& a, hipStream_t st);       // mcba_triangulate.hip

}  // namespace triangulate
}  // namespace mcba
