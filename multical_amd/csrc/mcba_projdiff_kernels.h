// mcba_projdiff_kernels.h -- the two kernels of mcba_projdiff.h.
//
// k_projdiff_fit: ONE WORKGROUP OF 256 THREADS PER JOB THAT FITS, the whole Levenberg-Marquardt loop (localize::solve_frame) in one
// launch, modelled on k_rig_pose.  The only synchronisation is __syncthreads under workgroup-uniform control flow: no atomics, no
// workgroup waits for another, every sum has a fixed order -- two calls return the same bits.
//   * first pass: thread t takes fit pixels t, t + 256, ..: the exact inverse under calibration 0, the validity under calibration 1
//     at the identity and the focus disc, RAY_STRIDE doubles a pixel into the job's run of the scratch buffer (at most 65 536
//     pixels = 3 MiB: L2 resident); the pixels that take part are counted by the xor butterfly;
//   * linearisation: the four waves take the fit pixels in chunks of 64, round-robin.  A lane forms its two rows [J | r] (4 or 7
//     entries each; zero for a pixel that does not take part) in registers, stages them through LDS at the 17-double stride of
//     k_rig_pose (columns K + 1 .. 15 stay zero) and the wave accumulates one v_mfma_f64_16x16x4_f64 tile holding J^T J, J^T r and
//     r^T r, operand lane l holding V[4 s + (l >> 4)][l & 15], result register r of lane l entry (4 r + (l >> 4), l & 15).  The four
//     wave tiles are added in wave order;
//   * thread 0 factors and solves (localize::damped_step, well_posed) and broadcasts through LDS;
//   * a trial cost is a residual-only pass over the rays, lane partials folded by the xor butterfly, wave sums added in wave order;
//   * the fit record (transform, counts, RMS before and after, status) stays in `fit` for the map kernel: no host round trip.
//
// k_projdiff_map: one query per lane, tiles of 256 consecutive queries of one job, the tile list shared over all jobs with the job
// found by bisection and the grid stride of k_projection_uncertainty.  The job's record (the camera entries of both calibrations:
// two for an intrinsics job, four for a transfer job; R_ba | t_ba of both; rho) and its transform (R(omega) | rho tau, formed by
// thread 0 from the fit record) are staged in LDS when the job changes; family switches and the mode branch are wave-uniform, lanes
// past the end of a job read and write nothing, every array index is a compile-time constant: no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include "mcba_projdiff.h"
#include "mcba_pnp_kernels.h"

namespace mcba {
namespace projdiff {

struct FitArgs {
  const double* recs;            // [n_jobs][REC_STRIDE]
  const int32_t* fit_jobs;       // [grid]
  const long long* ray_first;    // [grid + 1]
  const PixelSet* fit_pixels;    // [grid]
  const Focus* focus;            // [grid]
  const double* uv;              // the lists
  double* rays;                  // [ray_first[grid]][RAY_STRIDE]
  double* fit;                   // [n_jobs][FIT_STRIDE]
};

struct MapArgs {
  int n_jobs;
  const double* recs;            // [n_jobs][REC_STRIDE]
  const double* fit;             // [n_jobs][FIT_STRIDE]
  const long long* first;        // [n_jobs + 1]
  const long long* tile_first;   // [n_jobs + 1]
  const PixelSet* queries;       // [n_jobs]
  const double* uv;              // the lists
  double* diff;                  // [n,2]
  double* magnitude;             // [n] or null
  double* landing;               // [n,2] or null
  uint8_t* status;               // [n]
};

constexpr int PD_THREADS = 256, PD_WAVES = PD_THREADS / 64;
constexpr long long PD_MAX_GRID = 1 << 20;
constexpr int LDV = 17, STAGE = 128 * LDV;
// LDS of k_projdiff_fit, in doubles
constexpr int L_G = 0, L_WG = L_G + GS * GS, L_A = L_WG + PD_WAVES * GS * GS, L_P = L_A + MAX_K * MAX_K, L_Q = L_P + 8, L_D = L_Q + 8,
              L_PE = L_D + MAX_K, L_QE = L_PE + POSE_STRIDE, L_SC = L_QE + POSE_STRIDE, L_REC = L_SC + 16, L_STAGE = L_REC + REC_STRIDE,
              L_END = L_STAGE + PD_WAVES * STAGE;
static_assert(L_STAGE % 2 == 0, "layout of the LDS of k_projdiff_fit");
inline size_t fit_lds_bytes() { return (size_t)L_END * sizeof(double); }

// the device back-end of localize::solve_frame: every method is called by all threads of the workgroup
template <int K>
struct DeviceBackend {
  double* lds;
  const double* rays;
  int n, tid, wave, lane;
  double cost0;

  __device__ double* sc() const { return lds + L_SC; }
  __device__ const double* rec() const { return lds + L_REC; }

  // pose entry of the parameters x (thread 0); the caller synchronises
  __device__ void entries(const double* x, double* e) const {
    if (tid == 0) {
      double x6[6] = {x[0], x[1], x[2], 0.0, 0.0, 0.0};
      if constexpr (K == 6) { x6[3] = x[3]; x6[4] = x[4]; x6[5] = x[5]; }
      pose_entry(x6, e);
    }
  }

  __device__ double linearize() {
    double* V = lds + L_STAGE + wave * STAGE;
    const double* pe = lds + L_PE;
    const int rsub = lane >> 4, csub = lane & 15;
    pnp::wave_double4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int base = wave * 64; base < n; base += PD_THREADS) {
      const int i = base + lane;
      double ru[K + 1], rv[K + 1];
#pragma unroll
      for (int q = 0; q <= K; ++q) ru[q] = rv[q] = 0.0;
      if (i < n) {
        const double* ray = rays + (size_t)i * RAY_STRIDE;
        if (ray[RAY_OK] != 0.0) fit_rows<K>(rec(), pe, ray, ru, rv);
      }
#pragma unroll
      for (int q = 0; q <= K; ++q) { V[(2 * lane) * LDV + q] = ru[q]; V[(2 * lane + 1) * LDV + q] = rv[q]; }
      pnp::wave_fence();
      const int rows = 2 * min(64, n - base), nsteps = (rows + 3) >> 2;
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
    const double c = lds[L_G + K * GS + K];
    if (cost0 < 0.0) cost0 = c;
    return c;
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
      const bool ok = localize::damped_step(K, lds + L_G, lambda, lds + L_A, d, &w);
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

  __device__ double cost_at(const double* e) {
    double s = 0.0;
    for (int i = tid; i < n; i += PD_THREADS) {
      const double* ray = rays + (size_t)i * RAY_STRIDE;
      if (ray[RAY_OK] != 0.0) s += fit_sq(rec(), e, ray);
    }
    s = pnp::wave_xor_sum(s);
    if (lane == 0) sc()[8 + wave] = s;
    __syncthreads();
    const double total = ((sc()[8] + sc()[9]) + sc()[10]) + sc()[11];
    __syncthreads();
    return total;
  }
  __device__ double trial_cost() { return cost_at(lds + L_QE); }

  __device__ void accept() {
    if (tid < K) lds[L_P + tid] = lds[L_Q + tid];
    if (tid < POSE_STRIDE) lds[L_PE + tid] = lds[L_QE + tid];
    __syncthreads();
  }
};

// the fit of one job after the first pass; everything is uniform over the workgroup
template <int K>
__device__ void fit_on_device(double* lds, const double* rays, int n, int n_fit, double* fit) {
  const int tid = threadIdx.x;
  DeviceBackend<K> be{lds, rays, n, tid, tid >> 6, tid & 63, -1.0};
  int status = FIT_TOO_FEW, iters = 0;
  double cost1 = 0.0;
  if (n_fit >= min_pixels(K == 6 ? MODE_RIGID : MODE_ROTATION)) {
    if (tid < 8) lds[L_P + tid] = 0.0;
    for (int i = tid; i < PD_WAVES * STAGE; i += PD_THREADS) lds[L_STAGE + i] = 0.0;
    __syncthreads();
    be.entries(lds + L_P, lds + L_PE);
    __syncthreads();
    bool have = false;
    double cost = 0.0;
    const bool converged = localize::solve_frame(be, n_fit, MAX_ITERATIONS, &have, &iters, &cost);
    status = fit_status(have, converged);
    if (have) cost1 = be.cost_at(lds + L_PE);
  }
  if (tid == 0) fit_record(lds + L_P, K, n_fit, iters, be.cost0, cost1, status, fit);
}

__global__ __launch_bounds__(PD_THREADS) void k_projdiff_fit(FitArgs a) {
  extern __shared__ __attribute__((aligned(16))) double projdiff_lds[];
  double* lds = projdiff_lds;
  const int g = blockIdx.x, tid = threadIdx.x, j = a.fit_jobs[g];
  const long long r0 = a.ray_first[g];
  const int n = (int)(a.ray_first[g + 1] - r0);
  double* rays = a.rays + (size_t)r0 * RAY_STRIDE;
  for (int i = tid; i < REC_STRIDE; i += PD_THREADS) lds[L_REC + i] = a.recs[(size_t)j * REC_STRIDE + i];
  __syncthreads();
  // first pass
  const PixelSet set = a.fit_pixels[g];
  const Focus focus = a.focus[g];
  double count = 0.0;
  for (int i = tid; i < n; i += PD_THREADS) {
    double u, v, ray[RAY_STRIDE];
    pixel_of(set, a.uv, i, u, v);
    fit_ray(lds + L_REC, focus, u, v, ray);
#pragma unroll
    for (int k = 0; k < RAY_STRIDE; ++k) rays[(size_t)i * RAY_STRIDE + k] = ray[k];
    count += ray[RAY_OK];
  }
  count = pnp::wave_xor_sum(count);                     // (whole numbers below 2^53: exact in any order)
  if ((tid & 63) == 0) lds[L_SC + 8 + (tid >> 6)] = count;
  __syncthreads();                                      // (and the rays of this workgroup are visible to all of it)
  const int n_fit = (int)(((lds[L_SC + 8] + lds[L_SC + 9]) + lds[L_SC + 10]) + lds[L_SC + 11]);
  __syncthreads();
  double* fit = a.fit + (size_t)j * FIT_STRIDE;
  if ((int)lds[L_REC + REC_MODE] == MODE_RIGID) fit_on_device<6>(lds, rays, n, n_fit, fit);
  else fit_on_device<3>(lds, rays, n, n_fit, fit);
}

__global__ __launch_bounds__(PD_THREADS) void k_projdiff_map(MapArgs a) {
  __shared__ double rec[REC_STRIDE];
  __shared__ double xf[XF_STRIDE];
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
      const bool has_a = src[REC_HAS_A] != 0.0;
      for (int i = threadIdx.x; i < REC_STRIDE; i += PD_THREADS)
        if (has_a || i < REC_A0 || i >= REC_RHO) rec[i] = src[i];
      if (threadIdx.x == 0) stage_transform(src, a.fit + (size_t)j * FIT_STRIDE, xf);
      __syncthreads();
      staged = j;
    }
    const long long i = (b - a.tile_first[j]) * PD_THREADS + threadIdx.x;
    if (i < a.first[j + 1] - a.first[j]) {
      double u, v;
      pixel_of(a.queries[j], a.uv, i, u, v);
      Result r;
      query(rec, xf, u, v, r);
      const size_t slot = (size_t)(a.first[j] + i);
      a.diff[2 * slot] = r.du;
      a.diff[2 * slot + 1] = r.dv;
      if (a.magnitude) a.magnitude[slot] = r.mag;
      if (a.landing) { a.landing[2 * slot] = r.lu; a.landing[2 * slot + 1] = r.lv; }
      a.status[slot] = (uint8_t)r.status;
    }
  }
}

hipError_t fit_launch(const FitArgs& a, int n_fit_jobs, hipStream_t st);           // mcba_projdiff.hip
void map_launch(const MapArgs& a, long long tiles, hipStream_t st);

}  // namespace projdiff
}  // namespace mcba
