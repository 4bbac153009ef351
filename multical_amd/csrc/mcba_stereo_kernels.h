// mcba_stereo_kernels.h -- k_stereo_pair, the kernel of mcba_stereo.h: ONE WORKGROUP OF 256 THREADS PER PAIR that has a view, the
// whole Levenberg-Marquardt loop of the pair in one launch.  The only synchronisation is __syncthreads: no workgroup waits for
// another, no floating-point atomics, every sum has a fixed order -- two calls return the same bits.
//
//   * the records of the pair's two cameras sit in LDS; the relative pose's entry (R | t | L) and its trial sit there too and are
//     read at wave-uniform addresses.  The camera family is switched at run time (triangulate::project_jac): a pair may mix them;
//   * linearisation: the four waves take the pair's views round-robin.  A wave walks the board's P slots in chunks of 64, lane l
//     holding corner l of the chunk: both cameras' pixels come from the one [C,F,B,P,2] table.  The lane forms the two LEFT rows
//     [rel | view | r] of its corner in registers (13 entries each), stages them through LDS (128 rows a wave at k_rig_pose's stride
//     of 17 doubles: the columns 13 .. 15 stay zero, the operand reads of a half-wave fall on 33 consecutive doubles) and the wave
//     accumulates the 16 x 16 Gram matrix with v_mfma_f64_16x16x4_f64, operand lane l holding V[4 s + (l >> 4)][l & 15] and result
//     register r of lane l entry (4 r + (l >> 4), l & 15), as k_rig_pose and k_calibrate_camera do; then the two RIGHT rows go
//     through the same 128-row buffer.  One tile holds H_rr, H_rv, H_vv, both gradients and the cost of the view;
//   * the tile goes to LDS; its pair part is added to the wave's partial sums, its view part (H_vv, H_vr, g_v) to the view's
//     block in the global workspace (L2-resident) for the solve and the back-substitution, which are repeated for every damping
//     value without a new linearisation: nine views of a wave are eliminated side by side (seven lanes a view, one column of W
//     each, the Schur entries then added view by view), and a lane back-substitutes one view, the step norms folded by the xor
//     butterfly.  Wave partials are added in wave order; thread 0 factors the reduced system and broadcasts the step through LDS;
//   * a trial cost is a residual-only pass, lane partials folded by the xor butterfly, view costs added per wave in view order,
//     wave sums in wave order; the start scores its (up to four) candidates with the same pass.
#pragma once
#include <hip/hip_runtime.h>
#include "mcba_stereo.h"
#include "mcba_pnp_kernels.h"

namespace mcba {
namespace stereo {

struct StereoArgs {
  Tables t;
  int max_iter;
  double sigma_px;
  const int32_t* desc;         // [n_launched][2] left, right
  const int32_t* first;        // [n_launched + 1]
  const int32_t* slot;         // [views]
  const int32_t* n_common;     // [views]
  const int32_t* n_points;     // [n_launched]
  double* ws;                  // [views][VB_STRIDE]
  double* T;                   // [n_launched][16]
  double* cov;                 // [n_launched][36] or null
  double* sse;                 // [n_launched] or null
  int32_t* iters;              // [n_launched] or null
  uint8_t* status;             // [n_launched]
};

constexpr int PAIR_THREADS = 256;
static_assert(PAIR_THREADS / 64 == WAVES, "the host build's device order deals the views to as many partials");
constexpr int LDV = 17, STAGE = 128 * LDV;
// LDS of k_stereo_pair, in doubles
constexpr int L_STAGE = 0, L_WG = L_STAGE + WAVES * STAGE, L_PART = L_WG + WAVES * GS * GS, L_HS = L_PART + WAVES * PART,
              L_SS = L_HS + PART, L_P = L_SS + PART, L_Q = L_P + 8, L_DI = L_Q + 8, L_PE = L_DI + 8, L_QE = L_PE + POSE_STRIDE,
              L_CAND = L_QE + POSE_STRIDE, L_SC = L_CAND + MAX_CANDIDATES * 8, L_INV = L_SC + 32, L_REC = L_INV + 36,
              L_TOTAL = L_REC + 2 * CAM_STRIDE;
static_assert(L_WG % 2 == 0 && L_REC % 2 == 0, "layout of the LDS of k_stereo_pair");
constexpr size_t PAIR_LDS_BYTES = (size_t)L_TOTAL * sizeof(double);   // 82 KiB: above the default limit of a launch

// the device back-end of stereo::solve_pair: every method is called by all threads of the workgroup
struct DeviceBackend {
  const StereoArgs& a;
  double* lds;
  int l, r, v0, nv, tid, wave, lane;

  __device__ double* part(int w) const { return lds + L_PART + w * PART; }
  __device__ double* sc() const { return lds + L_SC; }
  __device__ double* block(int i) const { return a.ws + (size_t)(v0 + i) * VB_STRIDE; }
  __device__ const double* rec(int side) const { return lds + L_REC + side * CAM_STRIDE; }
  __device__ void fold(int n, double* out) const {
    for (int e = tid; e < n; e += PAIR_THREADS) out[e] = ((part(0)[e] + part(1)[e]) + part(2)[e]) + part(3)[e];
  }

  __device__ double linearize() {
    const Tables& t = a.t;
    double* hp = part(wave);
    double* V = lds + L_STAGE + wave * STAGE;
    double* G = lds + L_WG + wave * GS * GS;
    for (int e = lane; e < PART; e += 64) hp[e] = 0.0;
    const double* pe = lds + L_PE;
    const int rsub = lane >> 4, csub = lane & 15;
    for (int i = wave; i < nv; i += WAVES) {
      const int s = a.slot[v0 + i], b = s % t.B;
      const size_t rowl = slot_row(t, l, s), rowr = slot_row(t, r, s);
      double* vb = block(i);
      double p[6], ve[POSE_STRIDE];
#pragma unroll
      for (int q = 0; q < 6; ++q) p[q] = vb[VB_P + q];
      pose_entry(p, ve);
      pnp::wave_double4 acc = {0.0, 0.0, 0.0, 0.0};
      for (int base = 0; base < t.P; base += 64) {
        const int j = base + lane;
        const bool good = j < t.P && common_corner(t, rowl, rowr, b, j < t.P ? j : 0);
        double X[3] = {0.0, 0.0, 0.0};
        if (good) {
          const double* bd = t.board + ((size_t)b * t.P + j) * 3;
          X[0] = bd[0]; X[1] = bd[1]; X[2] = bd[2];
        }
        const int rows = 2 * min(64, t.P - base), nsteps = (rows + 3) >> 2;
        const double* vp = V + rsub * LDV + csub;
#pragma unroll 1
        for (int side = 0; side < 2; ++side) {
          double ru[NV], rv[NV];
          if (good) {
            const size_t row = (side ? rowr : rowl) + j;
            corner_rows(side, rec(side), ve, pe, X, t.points[2 * row], t.points[2 * row + 1], ru, rv);
          } else {
#pragma unroll
            for (int q = 0; q < NV; ++q) ru[q] = rv[q] = 0.0;
          }
#pragma unroll
          for (int q = 0; q < NV; ++q) { V[(2 * lane) * LDV + q] = ru[q]; V[(2 * lane + 1) * LDV + q] = rv[q]; }
          pnp::wave_fence();
          for (int st = 0; st < nsteps; ++st) {
            const double a0 = vp[(4 * st) * LDV];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, a0, acc, 0, 0, 0);
          }
          pnp::wave_fence();
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) G[(rsub + 4 * q) * GS + csub] = acc[q];
      pnp::wave_fence();
      if (lane < N_PAIR_SUMS) hp[lane] += pair_sum_entry(G, lane);
      for (int e = lane; e < N_VIEW_ENTRIES; e += 64) view_entry(G, e, vb);
      pnp::wave_fence();
    }
    __syncthreads();
    fold(N_PAIR_SUMS, lds + L_HS);
    __syncthreads();
    return lds[L_HS + 42];
  }

  // W and the Schur sums of every view at this damping; false: a block did not factor
  __device__ bool eliminate(double lambda, double floor) {
    double* sp = part(wave);
    for (int e = lane; e < PART; e += 64) sp[e] = 0.0;
    bool ok = true;
    // nine of the wave's views at a time: lane 7 g + j factors the block of view g of the group and solves for column j of its W
    // (the seven lanes of a view run the same factorisation in lockstep); the Schur entries are then added view by view, in view order
    constexpr int GROUP = 9;
    const int g = lane / 7, j = lane - 7 * g;
    for (int n0 = 0; wave + WAVES * n0 < nv; n0 += GROUP) {
      const int i = wave + WAVES * (n0 + g);
      if (g < GROUP && i < nv) ok = view_w_column(block(i), lambda, j, floor) && ok;
      pnp::wave_fence();
      if (lane < N_SCHUR) {
        for (int k = 0; k < GROUP; ++k) {
          const int i2 = wave + WAVES * (n0 + k);
          if (i2 < nv) sp[lane] += view_schur_entry(block(i2), lane);
        }
      }
    }
    const bool wave_ok = __ballot(!ok) == 0ull;
    if (lane == 0) sc()[4 + wave] = wave_ok ? 1.0 : 0.0;
    __syncthreads();
    const bool all_ok = sc()[4] != 0.0 && sc()[5] != 0.0 && sc()[6] != 0.0 && sc()[7] != 0.0;
    fold(N_SCHUR, lds + L_SS);
    __syncthreads();
    return all_ok;
  }

  __device__ bool solve(double lambda, bool* small) {
    bool all_ok = eliminate(lambda, 0.0);
    if (tid == 0) {
      double dn = 0.0, pn = 0.0;
      const bool good = all_ok && reduced_solve(lds + L_HS, lds + L_SS, lambda, lds + L_DI, lds + L_P, lds + L_Q, &dn, &pn);
      if (good) pose_entry(lds + L_Q, lds + L_QE);
      sc()[0] = good ? 1.0 : 0.0;
      sc()[1] = dn;
      sc()[2] = pn;
    }
    __syncthreads();
    all_ok = sc()[0] != 0.0;
    if (all_ok) {   // (uniform) lane l back-substitutes the wave's views l, l + 64, ...; lane partials folded by the xor butterfly
      double wd = 0.0, wp = 0.0;
      for (int i = wave + WAVES * lane; i < nv; i += WAVES * 64) view_backsub(block(i), lds + L_DI, &wd, &wp);
      wd = pnp::wave_xor_sum(wd);
      wp = pnp::wave_xor_sum(wp);
      if (lane == 0) { sc()[8 + 2 * wave] = wd; sc()[9 + 2 * wave] = wp; }
    }
    __threadfence_block();
    __syncthreads();
    if (all_ok) {
      double dn = sc()[1], pn = sc()[2];
#pragma unroll
      for (int w = 0; w < WAVES; ++w) { dn += sc()[8 + 2 * w]; pn += sc()[9 + 2 * w]; }
      *small = sqrt(dn) <= pnp::LM_STEP_TOL * (sqrt(pn) + pnp::LM_STEP_TOL);
    }
    __syncthreads();
    return all_ok;
  }

  // cost of the views at their trial poses with the relative pose entry e; SCORE: as a start candidate pays it
  template <bool SCORE>
  __device__ double costs(const double* e) {
    const Tables& t = a.t;
    double wc = 0.0;
    for (int i = wave; i < nv; i += WAVES) {
      const int s = a.slot[v0 + i], b = s % t.B;
      const size_t rowl = slot_row(t, l, s), rowr = slot_row(t, r, s);
      double* vb = block(i);
      double p[6], ve[POSE_STRIDE];
#pragma unroll
      for (int q = 0; q < 6; ++q) p[q] = vb[VB_Q + q];
      pose_entry(p, ve);
      double sl = 0.0, sr = 0.0;
      for (int j = lane; j < t.P; j += 64)
        if (common_corner(t, rowl, rowr, b, j)) {
          const double* bd = t.board + ((size_t)b * t.P + j) * 3;
          const double X[3] = {bd[0], bd[1], bd[2]};
          sl += corner_sq<SCORE>(0, rec(0), ve, e, X, t.points[2 * (rowl + j)], t.points[2 * (rowl + j) + 1]);
          sr += corner_sq<SCORE>(1, rec(1), ve, e, X, t.points[2 * (rowr + j)], t.points[2 * (rowr + j) + 1]);
        }
      sl = pnp::wave_xor_sum(sl);
      sr = pnp::wave_xor_sum(sr);
      if (!SCORE && lane == 0) { vb[VB_SSE] = sl; vb[VB_SSE + 1] = sr; }
      wc += sl + sr;
    }
    if (lane == 0) sc()[8 + wave] = wc;
    __syncthreads();
    const double total = ((sc()[8] + sc()[9]) + sc()[10]) + sc()[11];
    __syncthreads();
    return total;
  }
  __device__ double trial() { return costs<false>(lds + L_QE); }

  __device__ void copy_views(int from, int to) {
    const int mine = nv > wave ? (nv - wave + WAVES - 1) / WAVES : 0;   // views of this wave
    for (int e = lane; e < 6 * mine; e += 64) {
      double* vb = block(wave + WAVES * (e / 6));
      vb[to + e % 6] = vb[from + e % 6];
    }
    __threadfence_block();
    __syncthreads();
  }
  __device__ void accept() {
    if (tid < 6) lds[L_P + tid] = lds[L_Q + tid];
    if (tid < POSE_STRIDE) lds[L_PE + tid] = lds[L_QE + tid];
    copy_views(VB_Q, VB_P);
  }

  __device__ bool start() {
    const Tables& t = a.t;
    const size_t fb = (size_t)t.F * t.B;
    for (int i = wave; i < nv; i += WAVES)
      if (lane == 0) {
        double* vb = block(i);
        intr::pose_to_params(t.view_poses + 16 * ((size_t)l * fb + (size_t)a.slot[v0 + i]), vb + VB_P);
        for (int q = 0; q < 6; ++q) vb[VB_Q + q] = vb[VB_P + q];
      }
    int* picks = (int*)(lds + L_DI);                     // (scratch: nothing else uses it yet)
    if (tid == 0) sc()[0] = (double)select_views(nv, a.n_common + v0, picks);
    __threadfence_block();
    __syncthreads();
    const int nc = (int)sc()[0];
    if (tid < nc) {
      const size_t s = (size_t)a.slot[v0 + picks[tid]];
      candidate_params(t.view_poses + 16 * ((size_t)l * fb + s), t.view_poses + 16 * ((size_t)r * fb + s), lds + L_CAND + 8 * tid);
    }
    __syncthreads();
    double scores[MAX_CANDIDATES] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int c = 0; c < nc; ++c) {
      if (tid == 0) pose_entry(lds + L_CAND + 8 * c, lds + L_QE);
      __syncthreads();
      const double sco = costs<true>(lds + L_QE);
#pragma unroll
      for (int k = 0; k < MAX_CANDIDATES; ++k) scores[k] = (k == c) ? sco : scores[k];
    }
    const int best = localize::pick_candidate(scores, nc);
    if (best >= 0) {
      if (tid < 6) lds[L_P + tid] = lds[L_CAND + 8 * best + tid];
      __syncthreads();
      if (tid == 0) pose_entry(lds + L_P, lds + L_PE);
    }
    __syncthreads();
    return best >= 0;
  }

  __device__ bool information() {
    const bool all_ok = eliminate(0.0, PIVOT_FLOOR);
    if (tid == 0) sc()[0] = (all_ok && reduced_inverse(lds + L_HS, lds + L_SS, lds + L_INV)) ? 1.0 : 0.0;
    __syncthreads();
    const bool ok = sc()[0] != 0.0;
    __syncthreads();
    return ok;
  }

  __device__ double final_costs() {
    copy_views(VB_P, VB_Q);
    return costs<false>(lds + L_PE);
  }
};

__global__ __launch_bounds__(PAIR_THREADS) void k_stereo_pair(StereoArgs a) {
  extern __shared__ __attribute__((aligned(16))) double stereo_lds[];
  double* lds = stereo_lds;
  const int k = blockIdx.x, tid = threadIdx.x;
  const int l = a.desc[2 * k], r = a.desc[2 * k + 1], v0 = a.first[k], nv = a.first[k + 1] - v0;
  for (int i = tid; i < WAVES * STAGE; i += PAIR_THREADS) lds[L_STAGE + i] = 0.0;
  if (tid < 2 * CAM_STRIDE) lds[L_REC + tid] = a.t.recs[(size_t)(tid < CAM_STRIDE ? l : r) * CAM_STRIDE + tid % CAM_STRIDE];
  __syncthreads();
  DeviceBackend be{a, lds, l, r, v0, nv, tid, tid >> 6, tid & 63};
  int iters = 0;
  bool have = false;
  double sse = 0.0;
  const int status = solve_pair(be, a.max_iter, &iters, &have, &sse);   // (uniform over the workgroup)
  if (tid < 16) {
    const int row = tid >> 2, c = tid & 3;
    const double* pe = lds + L_PE;
    const double ident = (tid % 5 == 0) ? 1.0 : 0.0;
    a.T[16 * (size_t)k + tid] = !have ? ident : row == 3 ? ident : (c == 3 ? pe[POSE_T + row] : pe[POSE_R + 3 * row + c]);
  }
  if (a.cov && tid < 36) {
    const double s2 = pixel_variance(a.sigma_px, sse, a.n_points[k], nv);
    a.cov[36 * (size_t)k + tid] = have ? s2 * lds[L_INV + tid] : undistort::quiet_nan();
  }
  if (tid == 0) {
    if (a.sse) a.sse[k] = have ? sse : 0.0;
    if (a.iters) a.iters[k] = iters;
    a.status[k] = (uint8_t)status;
  }
}

hipError_t stereo_pair_launch(const StereoArgs& a, int n_launched, hipStream_t st);   // mcba_stereo.hip

}  // namespace stereo
}  // namespace mcba
