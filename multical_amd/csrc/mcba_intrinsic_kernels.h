// mcba_intrinsic_kernels.h -- the kernels of mcba_calibrate_intrinsics (mathematics: mcba_intrinsic.h).
//
//   k_intrinsic_homography<NPL>   one wavefront per active view: homography board plane -> raw pixels (LanePoints + WaveReducer
//                                 of k_view_pose)
//   k_intrinsic_focal             one wavefront per camera: start block [fx fy cx cy 0 0...] from the camera's homographies, in
//                                 view order, and the camera-table entry k_view_pose reads
//   (k_view_pose)                 the start pose of every view with that camera
//   k_calibrate_camera<ND, FISH>  ONE WORKGROUP PER CAMERA, four waves, the whole Levenberg-Marquardt loop in one launch.  The
//                                 only synchronisation is __syncthreads: no workgroup waits for another, no floating-point
//                                 atomics, every sum has a fixed order -- two calls return the same bits.
// Work division of k_calibrate_camera: the waves take the camera's usable views round-robin.  A wave walks its view in chunks of
// 64 corners, lane l holding corner l of the chunk: residual and the two rows [Kc | A (-[R X]x | I) diag(L, I) | r] in registers,
// staged through LDS (128 rows x 26 columns per wave) and accumulated into the view's Gram matrix by v_mfma_f64_16x16x4_f64 --
// the three upper 16 x 16 tiles of the 32-column matrix (one tile for the 4-coefficient models: 15 columns), operand lane l
// holding V[4 s + (l >> 4)][16 t + (l & 15)] as in k_linearize.  The Gram matrix goes back to LDS; its camera part is added to
// the wave's partial sums, its view part (H_vv, H_vi, g_v) goes to the global workspace (L2-resident at these sizes) for the
// solve and the back-substitution, which are repeated for every damping value without a new linearisation.  Wave partials are
// added in wave order; thread 0 factors the reduced system and broadcasts the step through LDS.  Corners are re-read from
// HBM / L2 in every pass (a camera's 50 views x 324 corners are 0.65 MB).
#pragma once
#include <hip/hip_runtime.h>
#include "mcba_intrinsic.h"
#include "mcba_pnp_kernels.h"

namespace mcba {
namespace intr {

typedef pnp::wave_double4 intr_double4;
using pnp::wave_fence;

struct IntrinsicArgs {
  int P, max_iter, warm;
  const double* pixel;        // [views][P][2]   the views of the cameras that are solved, camera-major
  const uint8_t* valid;       // [views][P]
  const int32_t* desc;        // [views][2] camera, board
  const double* board;        // [B][P][3]
  const double* planes;       // [B][PLANE_STRIDE]
  const int32_t* cam_first;   // [C + 1] view range of every camera
  const uint8_t* cam_fa;      // [C]
  const uint8_t* cam_fish;    // [C]
  const int32_t* cam_nd;      // [C]
  const double* mask;         // [C][MAX_KI]
  const double* image_size;   // [C][2]
  double* Hv;                 // [views][10] homography + usable flag
  double* blk;                // [C][BLK] camera blocks: start (uploaded when warm) -> result
  double* cam_entry;          // [C][CAM_STRIDE] start camera, read by k_view_pose
  double* pose;               // [views][16] start pose -> result
  uint8_t* vstatus;           // [views] status of the start pose -> of the view
  double* sse;                // [views]
  int32_t* n_used;            // [views]
  double* ws;                 // [views][VB_STRIDE]
  int32_t* ulist;             // [views] the usable views of every camera, compacted inside its range
  int32_t* cam_iters;         // [C]
  uint8_t* cam_status;        // [C]
  const int32_t* group;       // cameras of this launch
};

constexpr int CAL_THREADS = 256, CAL_WAVES = CAL_THREADS / 64;
constexpr int STAGE_ROWS = 128, LDV = 26;                    // two rows per corner of a 64-corner chunk
constexpr int STAGE = STAGE_ROWS * LDV + 8;                  // (+ the tail the second tile's operand reads past the last row)
constexpr int PART = ((n_cam_sums(MAX_KI) + 1) / 2) * 2;     // wave partial of the camera sums / of the Schur sums
// LDS of k_calibrate_camera, in doubles
constexpr int L_STAGE = 0, L_PART = L_STAGE + CAL_WAVES * STAGE, L_HS = L_PART + CAL_WAVES * PART, L_SS = L_HS + PART,
              L_A = L_SS + PART, L_DI = L_A + MAX_KI * MAX_KI, L_BLK = L_DI + MAX_KI, L_QBLK = L_BLK + BLK + 1,
              L_E = L_QBLK + BLK + 1, L_EQ = L_E + CAM_STRIDE, L_MASK = L_EQ + CAM_STRIDE, L_SC = L_MASK + MAX_KI,
              L_TOTAL = L_SC + 16;
constexpr size_t CAL_LDS_BYTES = (size_t)L_TOTAL * sizeof(double);
static_assert(GS * GS <= STAGE, "the Gram matrix reuses the staging buffer");

template <int NPL>
__global__ __launch_bounds__(pnp::VIEW_POSE_THREADS) void k_intrinsic_homography(IntrinsicArgs a, int n_views) {
  const int k = blockIdx.x * (pnp::VIEW_POSE_THREADS / 64) + (threadIdx.x >> 6);
  if (k >= n_views) return;
  const int lane = threadIdx.x & 63, b = a.desc[2 * k + 1];
  pnp::LanePoints<NPL> pts;
  load_view_raw(pts, lane, 64, a.P, a.pixel + (size_t)k * a.P * 2, a.valid + (size_t)k * a.P, a.board + (size_t)b * a.P * 3);
  double Hv[10];
  view_homography(pts, pnp::WaveReducer(), a.planes + (size_t)b * pnp::PLANE_STRIDE, Hv);
  if (lane < 10) {
    double v = Hv[0];
#pragma unroll
    for (int i = 1; i < 10; ++i) v = (lane == i) ? Hv[i] : v;
    a.Hv[(size_t)k * 10 + lane] = v;
  }
}

__global__ __launch_bounds__(64) void k_intrinsic_focal(IntrinsicArgs a) {
  const int c = blockIdx.x, k0 = a.cam_first[c], nv = a.cam_first[c + 1] - k0;
  if (nv <= 0 || threadIdx.x != 0) return;
  double* blk = a.blk + (size_t)c * BLK;
  const bool fa = a.cam_fa[c] != 0, fish = a.cam_fish[c] != 0;
  if (!camera_start(a.Hv + (size_t)k0 * 10, nv, a.image_size[2 * c], a.image_size[2 * c + 1], fa, fish, blk)) {
    a.cam_status[c] = (uint8_t)CAM_DEGENERATE;
    for (int i = 0; i < BLK; ++i) blk[i] = i < 2 ? 1.0 : 0.0;   // (k_view_pose still runs over the camera's views)
  }
  camera_entry(blk, a.cam_nd[c], 0.0, fa, a.cam_entry + (size_t)c * CAM_STRIDE, fish);
}

// the device back-end of intr::lm_loop: every method is called by all threads of the workgroup
template <int ND, bool FISH>
struct DeviceBackend {
  static constexpr int KI = 4 + ND, NV = KI + 7, NCS = n_cam_sums(KI), NSS = KI * (KI + 1);
  const IntrinsicArgs& a;
  double* lds;
  int c, k0, nu, tid, wave, lane;
  bool fa;

  __device__ double* stage() const { return lds + L_STAGE + wave * STAGE; }
  __device__ double* part(int w) const { return lds + L_PART + w * PART; }
  __device__ int view(int i) const { return a.ulist[k0 + i]; }
  __device__ double* block(int k) const { return a.ws + (size_t)k * VB_STRIDE; }

  __device__ double linearize() {
    double* hp = part(wave);
    double* V = stage();
    for (int e = lane; e < NCS; e += 64) hp[e] = 0.0;
    const double* cam = lds + L_E;
    const double* mask = lds + L_MASK;
    const int rsub = lane >> 4, csub = lane & 15;
    for (int i = wave; i < nu; i += CAL_WAVES) {
      const int k = view(i), b = a.desc[2 * k + 1];
      double* vb = block(k);
      double p[6], R[9], L[9];
#pragma unroll
      for (int q = 0; q < 6; ++q) p[q] = vb[VB_P + q];
      rodrigues(p, R, L);
      const double* px = a.pixel + (size_t)k * a.P * 2;
      const uint8_t* ok = a.valid + (size_t)k * a.P;
      const double* bd = a.board + (size_t)b * a.P * 3;
      intr_double4 acc00 = {0.0, 0.0, 0.0, 0.0}, acc01 = acc00, acc11 = acc00;
      for (int base = 0; base < a.P; base += 64) {
        const int j = base + lane;
        double ru[NV], rv[NV];
        const bool good = j < a.P && ok[j < a.P ? j : 0] != 0;
        if (good) {
          const double X[3] = {bd[3 * j], bd[3 * j + 1], bd[3 * j + 2]};
          corner_rows<ND, FISH>(cam, R, L, p + 3, mask, X, px[2 * j], px[2 * j + 1], ru, rv);
        } else {
#pragma unroll
          for (int q = 0; q < NV; ++q) ru[q] = rv[q] = 0.0;
        }
#pragma unroll
        for (int q = 0; q < NV; ++q) { V[(2 * lane) * LDV + q] = ru[q]; V[(2 * lane + 1) * LDV + q] = rv[q]; }
        wave_fence();
        const int rows = 2 * min(64, a.P - base), nsteps = (rows + 3) >> 2;
        const double* vp = V + rsub * LDV + csub;
        for (int st = 0; st < nsteps; ++st) {
          const double a0 = vp[(4 * st) * LDV];
          acc00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, a0, acc00, 0, 0, 0);
          if constexpr (NV > 16) {
            // the second tile's operand is columns 16 .. 31 of a row staged at stride LDV = 26: its entries 10 .. 15 are columns
            // 0 .. 5 of the NEXT row (of the 8-double tail after the last one).  They only reach Gram rows / columns 26 .. 31,
            // which nothing reads (NV <= 25): gsym is only ever asked for indices below NV.
            const double a1 = vp[(4 * st) * LDV + 16];
            acc01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, a1, acc01, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, a1, acc11, 0, 0, 0);
          }
        }
        wave_fence();
      }
      // the Gram matrix takes the place of the staged rows: entry (i, j), i <= j, at V[i GS + j]
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        V[(rsub + 4 * r) * GS + csub] = acc00[r];
        if constexpr (NV > 16) {
          V[(rsub + 4 * r) * GS + 16 + csub] = acc01[r];
          V[(16 + rsub + 4 * r) * GS + 16 + csub] = acc11[r];
        }
      }
      wave_fence();
      for (int e = lane; e < NCS; e += 64) hp[e] += cam_sum_entry(V, KI, e);
      for (int e = lane; e < n_view_entries(KI); e += 64) view_entry(V, KI, e, vb);
      wave_fence();
      // (the matrix leaves the buffer: the next view's rows rewrite columns 0 .. NV - 1 of every row, the columns NV .. 25 are 0 again)
      for (int e = lane; e < STAGE; e += 64) V[e] = 0.0;
      wave_fence();
    }
    __syncthreads();
    double* hs = lds + L_HS;
    for (int e = tid; e < NCS; e += CAL_THREADS) hs[e] = ((part(0)[e] + part(1)[e]) + part(2)[e]) + part(3)[e];
    __syncthreads();
    return hs[KI * KI + KI];
  }

  __device__ bool solve(double lambda, bool* small) {
    double* sp = part(wave);
    double* sc = lds + L_SC;
    for (int e = lane; e < NSS; e += 64) sp[e] = 0.0;
    bool ok = true;
    for (int i = wave; i < nu; i += CAL_WAVES) {
      double* vb = block(view(i));
      if (lane <= KI) ok = view_w_column(vb, KI, lambda, lane) && ok;
      wave_fence();
      for (int e = lane; e < NSS; e += 64) sp[e] += view_schur_entry(vb, KI, e);
    }
    const bool wave_ok = __ballot(!ok) == 0ull;
    if (lane == 0) sc[4 + wave] = wave_ok ? 1.0 : 0.0;
    __syncthreads();
    bool all_ok = sc[4] != 0.0 && sc[5] != 0.0 && sc[6] != 0.0 && sc[7] != 0.0;
    double* ss = lds + L_SS;
    for (int e = tid; e < NSS; e += CAL_THREADS) ss[e] = ((part(0)[e] + part(1)[e]) + part(2)[e]) + part(3)[e];
    __syncthreads();
    if (tid == 0) {
      double dn = 0.0, pn = 0.0;
      const bool good = all_ok && reduced_solve(KI, lds + L_HS, ss, lambda, lds + L_A, lds + L_DI, lds + L_BLK, lds + L_QBLK, &dn, &pn);
      if (good) camera_entry(lds + L_QBLK, ND, 0.0, fa, lds + L_EQ, FISH);
      sc[0] = good ? 1.0 : 0.0;
      sc[1] = dn;
      sc[2] = pn;
    }
    __syncthreads();
    all_ok = sc[0] != 0.0;
    if (all_ok && lane == 0) {
      double wd = 0.0, wp = 0.0;
      for (int i = wave; i < nu; i += CAL_WAVES) view_backsub(block(view(i)), KI, lds + L_DI, &wd, &wp);
      sc[8 + 2 * wave] = wd;
      sc[9 + 2 * wave] = wp;
    }
    __syncthreads();
    if (all_ok) {
      double dn = sc[1], pn = sc[2];
#pragma unroll
      for (int w = 0; w < CAL_WAVES; ++w) { dn += sc[8 + 2 * w]; pn += sc[9 + 2 * w]; }
      *small = sqrt(dn) <= pnp::LM_STEP_TOL * (sqrt(pn) + pnp::LM_STEP_TOL);
    }
    __syncthreads();
    return all_ok;
  }

  // cost of the views at their trial poses with the trial camera
  __device__ double trial() {
    const double* cam = lds + L_EQ;
    double* sc = lds + L_SC;
    double wc = 0.0;
    for (int i = wave; i < nu; i += CAL_WAVES) {
      const int k = view(i), b = a.desc[2 * k + 1];
      double* vb = block(k);
      double p[6], R[9], L[9];
#pragma unroll
      for (int q = 0; q < 6; ++q) p[q] = vb[VB_Q + q];
      rodrigues(p, R, L);
      const double* px = a.pixel + (size_t)k * a.P * 2;
      const uint8_t* ok = a.valid + (size_t)k * a.P;
      const double* bd = a.board + (size_t)b * a.P * 3;
      double s = 0.0;
      for (int j = lane; j < a.P; j += 64)
        if (ok[j] != 0) {
          const double X[3] = {bd[3 * j], bd[3 * j + 1], bd[3 * j + 2]};
          s += corner_sse<ND, FISH>(cam, R, p + 3, X, px[2 * j], px[2 * j + 1]);
        }
      s = pnp::wave_xor_sum(s);
      if (lane == 0) vb[VB_SSE] = s;
      wc += s;
    }
    if (lane == 0) sc[8 + wave] = wc;
    __syncthreads();
    const double total = ((sc[8] + sc[9]) + sc[10]) + sc[11];
    __syncthreads();
    return total;
  }

  __device__ void copy_point(bool to_trial) {
    double* cur = lds + L_BLK;
    double* tri = lds + L_QBLK;
    if (tid < BLK) { if (to_trial) tri[tid] = cur[tid]; else cur[tid] = tri[tid]; }
    if (tid < CAM_STRIDE) { if (to_trial) lds[L_EQ + tid] = lds[L_E + tid]; else lds[L_E + tid] = lds[L_EQ + tid]; }
    for (int i = wave; i < nu; i += CAL_WAVES)
      if (lane < 6) {
        double* vb = block(view(i));
        if (to_trial) vb[VB_Q + lane] = vb[VB_P + lane]; else vb[VB_P + lane] = vb[VB_Q + lane];
      }
    __syncthreads();
  }
  __device__ void accept() { copy_point(false); }
  __device__ void final_pass() {
    copy_point(true);
    trial();
  }
};

template <int ND, bool FISH>
__global__ __launch_bounds__(CAL_THREADS) void k_calibrate_camera(IntrinsicArgs a) {
  extern __shared__ __attribute__((aligned(16))) double intr_lds[];
  double* lds = intr_lds;
  const int c = a.group[blockIdx.x], tid = threadIdx.x;
  const int k0 = a.cam_first[c], nv = a.cam_first[c + 1] - k0;
  if (a.cam_status[c] != (uint8_t)CAM_OK) return;              // (no focal start; uniform)
  double* sc = lds + L_SC;
  if (tid == 0) {
    int nu = 0;
    for (int k = k0; k < k0 + nv; ++k) {
      a.sse[k] = 0.0;
      a.n_used[k] = 0;
      const int st = a.vstatus[k];
      if (st == pnp::ST_OK || st == pnp::ST_NOT_CONVERGED) { a.ulist[k0 + nu++] = k; a.vstatus[k] = (uint8_t)pnp::ST_OK; }
    }
    sc[3] = (double)nu;
  }
  for (int e = tid; e < CAL_WAVES * STAGE; e += CAL_THREADS) lds[L_STAGE + e] = 0.0;
  if (tid < BLK) lds[L_BLK + tid] = a.blk[(size_t)c * BLK + tid];
  if (tid < MAX_KI) lds[L_MASK + tid] = a.mask[(size_t)c * MAX_KI + tid];
  __threadfence_block();
  __syncthreads();
  const int nu = (int)sc[3];
  if (nu < MIN_VIEWS) {
    if (tid == 0) a.cam_status[c] = (uint8_t)CAM_TOO_FEW_VIEWS;
    return;
  }
  const bool fa = a.cam_fa[c] != 0;
  if (tid == 0) camera_entry(lds + L_BLK, ND, 0.0, fa, lds + L_E, FISH);
  for (int i = tid; i < nu; i += CAL_THREADS) {
    const int k = a.ulist[k0 + i];
    pose_to_params(a.pose + (size_t)k * 16, a.ws + (size_t)k * VB_STRIDE + VB_P);
  }
  __threadfence_block();
  __syncthreads();
  DeviceBackend<ND, FISH> be{a, lds, c, k0, nu, tid, tid >> 6, tid & 63, fa};
  int iters = 0;
  bool finite = false;
  const bool ok = lm_loop(be, a.max_iter, &iters, &finite);
  if (tid == 0) a.cam_iters[c] = iters;
  if (!finite) {
    if (tid == 0) a.cam_status[c] = (uint8_t)CAM_DEGENERATE;
    return;
  }
  be.final_pass();
  if (tid < BLK) a.blk[(size_t)c * BLK + tid] = (tid == 1 && fa) ? lds[L_BLK] : lds[L_BLK + tid];
  for (int i = be.wave; i < nu; i += CAL_WAVES) {
    const int k = a.ulist[k0 + i];
    const uint8_t* vok = a.valid + (size_t)k * a.P;
    int n = 0;
    for (int base = 0; base < a.P; base += 64) {
      const int j = base + be.lane;
      n += __popcll(__ballot(j < a.P && vok[j < a.P ? j : 0] != 0));
    }
    if (be.lane == 0) {
      const double* vb = a.ws + (size_t)k * VB_STRIDE;
      params_to_pose(vb + VB_P, a.pose + (size_t)k * 16);
      a.sse[k] = vb[VB_SSE];
      a.n_used[k] = n;
    }
  }
  if (tid == 0) a.cam_status[c] = (uint8_t)(ok ? CAM_OK : CAM_NOT_CONVERGED);
}

// mcba_intrinsic.hip
hipError_t intrinsic_start_launch(const IntrinsicArgs& a, int n_views, int C, hipStream_t st);
hipError_t calibrate_camera_launch(const IntrinsicArgs& a, int nd, bool fisheye, int n_cameras, hipStream_t st);

}  // namespace intr
}  // namespace mcba
