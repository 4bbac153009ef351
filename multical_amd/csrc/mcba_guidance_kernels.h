// mcba_guidance_kernels.h -- the kernels of mcba_guidance.h.
//
// k_view_schur: ONE WORKGROUP OF 128 THREADS PER VIEW (candidate or focus), two waves; the staging of the rows and the MFMA accumulation
// are wave_gram_tiles of mcba_gram_front.h, which k_rig_gram (mcba_rigview_kernels.h) shares.  The records of the view and of its camera
// (entry, image size, W_c) are staged in LDS and read at uniform addresses; the camera-family switch is uniform over the workgroup.
//   * a wave takes the view's points in chunks of 64, round-robin; lane l owns point l of the chunk: visibility, one projection
//     (project_padded), the two rows [Kc W_c | E] of r + n_nuisance <= 24 entries, written straight to LDS at a 25-double stride
//     (128 rows a wave), a point that is not visible as zero rows; the visible points are counted by ballot;
//   * the wave accumulates the upper three 16 x 16 tiles (00, 01, 11) of the 32-column Gram matrix by v_mfma_f64_16x16x4_f64,
//     operand lane l holding V[4 s + (l >> 4)][16 t + (l & 15)], result register q of lane l entry (4 q + (l >> 4), l & 15), as in
//     k_calibrate_camera -- the 01 / 11 tiles only when r + n_nuisance > 16.  The second tile's operand is columns 16 .. 31 of a row
//     staged at stride 25: its entries 9 .. 15 are columns 0 .. 6 of the NEXT row (of the 8-double tail after the last one).  They
//     only reach Gram rows / columns 25 .. 31, which nothing reads; column 24 is never written and stays 0;
//   * the last K-step of a chunk may be half filled: the lanes past the view's last point write zero rows;
//   * epilogue: the two wave tiles are added in wave order, thread 0 factors the nuisance block, threads c < r solve their column of
//     Y = L^-1 G_ek, thread (i, j) writes S_ij = G_ij - sum_k Y_ki Y_kj; a view that is not OK gets S = 0.
// No atomics, no cross-block waits, every sum has a fixed order: two calls return the same bits.  Every register array is indexed
// by compile-time constants after unrolling (the padded 2 x 18 camera block); the rows go to LDS as they are formed: no scratch.
//
// k_view_score: one wavefront per entry of the score list (a candidate, or the null view of a camera: the base alone), four to a
// workgroup.  Lane 0 factors M = B_c + S_v / sigma^2, lane 1 the base B_c; then lane j solves column j of X = L^-1 Q_c, lane i
// entry (i, i) of L^-1 X^T, lane 0 adds the trace in index order.  With `posterior` the null view also writes (L L^T)^-1.
// k_base_add: B_c += S_winner / sigma^2 for the winners of a round.
#pragma once
#include <hip/hip_runtime.h>
#include "mcba_guidance.h"
#include "mcba_gram_front.h"

namespace mcba {
namespace guidance {

struct SchurArgs {
  const int32_t* launch;         // [grid] the views that are served
  const double* vrecs;           // [n_views + C][V_STRIDE]
  const double* crecs;           // [C][CREC_STRIDE]
  const double* board_points;    // [B][board_stride][3]
  int board_stride;
  const double* uv;              // the lists
  int rs;                        // row stride of an S
  double* S;                     // [n_views + C][rs][rs]
  int32_t* n_visible;            // [n_views + C]
  uint8_t* status;               // [n_views + C]
};

struct ScoreArgs {
  int n_entries, n_views, rs;
  const int32_t* entries;        // [n_entries] view, or -(c + 1): the null view of camera c
  const int32_t* view_camera;    // [n_views + C]
  const int32_t* cam_r;          // [C]
  const double* S;               // [n_views + C][rs][rs]; the focus of camera c is view n_views + c
  const int32_t* n_visible;
  const uint8_t* status;
  const double* B;               // [C][rs][rs]
  double inv_s2;
  double* gain;                  // [n_entries]
  double* focus;                 // [n_entries]
  double* posterior;             // [C][rs][rs] or null
};

// LDS of k_view_schur, in doubles
constexpr int L_CREC = 0, L_VREC = L_CREC + CREC_STRIDE, L_STAGE = L_VREC + V_STRIDE, L_G = L_STAGE + SCHUR_WAVES * STAGE,
              L_L = L_G + GS * GS, L_Y = L_L + MAX_NN * MAX_NN, L_SC = L_Y + MAX_NN * MAX_R, L_END = L_SC + 8;
static_assert(MAX_COLS < LDV && LDV + 7 <= GS, "the columns a row holds, and what the second operand reads past it");
static_assert((size_t)L_END * sizeof(double) <= 65536, "static LDS of k_view_schur");

__global__ __launch_bounds__(SCHUR_THREADS) void k_view_schur(SchurArgs a) {
  __shared__ double lds[L_END];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int v = a.launch[blockIdx.x];
  const double* vsrc = a.vrecs + (size_t)v * V_STRIDE;
  const double* csrc = a.crecs + (size_t)(int)vsrc[V_CAMERA] * CREC_STRIDE;
  if (tid < V_STRIDE) lds[L_VREC + tid] = vsrc[tid];
  for (int i = tid; i < CREC_STRIDE; i += SCHUR_THREADS) lds[L_CREC + i] = csrc[i];
  for (int i = tid; i < SCHUR_WAVES * STAGE; i += SCHUR_THREADS) lds[L_STAGE + i] = 0.0;
  __syncthreads();
  const double* crec = lds + L_CREC;
  const double* vrec = lds + L_VREC;
  const int r = (int)crec[CREC_RANK], nn = (int)vrec[V_NN], n = (int)vrec[V_N], cols = r + nn;
  double* V = lds + L_STAGE + wave * STAGE;
  const int count = wave_gram_tiles(V, n, cols, wave, lane, [&](int i, double* row_u, double* row_v) {
    return point_rows(crec, vrec, a.board_points, a.board_stride, a.uv, i, r, nn, row_u, row_v);
  });
  if (lane == 0) lds[L_SC + wave] = (double)count;
  __syncthreads();
  double* G = lds + L_G;
  const double* T0 = lds + L_STAGE;
  for (int e = tid; e < GS * GS; e += SCHUR_THREADS) {
    const int i = e / GS, j = e % GS;
    G[e] = (i <= j && (i < 16 || j >= 16)) ? T0[e] + T0[STAGE + e] : 0.0;
  }
  __syncthreads();
  double* L = lds + L_L;
  double* Y = lds + L_Y;
  if (tid == 0) lds[L_SC + 4] = (nn == 0 || nuisance_factor(G, r, nn, L)) ? 1.0 : 0.0;
  __syncthreads();
  const int n_visible = (int)(lds[L_SC] + lds[L_SC + 1]);
  const int status = view_status(n_visible, (int)vrec[V_MIN], lds[L_SC + 4] != 0.0);       // (uniform over the workgroup)
  double* S = a.S + (size_t)v * a.rs * a.rs;
  if (status == ST_OK) {
    if (tid < r && nn > 0) nuisance_column(G, r, nn, L, tid, Y);
    __syncthreads();
    for (int e = tid; e < r * r; e += SCHUR_THREADS) S[(e / r) * a.rs + e % r] = schur_entry(G, nn, Y, e / r, e % r);
  } else {
    for (int e = tid; e < r * r; e += SCHUR_THREADS) S[(e / r) * a.rs + e % r] = 0.0;
  }
  if (tid == 0) {
    a.n_visible[v] = n_visible;
    a.status[v] = (uint8_t)status;
  }
}

constexpr int SCORE_THREADS = 256, SCORE_WAVES = SCORE_THREADS / 64;
constexpr int SCORE_LDS = 4 * MAX_R * MAX_R;      // Lm | Lb | X | Yw of a wave

__global__ __launch_bounds__(SCORE_THREADS) void k_view_score(ScoreArgs a) {
  __shared__ double lds[SCORE_WAVES * SCORE_LDS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int e = blockIdx.x * SCORE_WAVES + wave;
  if (e >= a.n_entries) return;                               // (no workgroup barrier below: the waves are on their own)
  const int ent = a.entries[e];
  const bool null_view = ent < 0;
  const int c = null_view ? -ent - 1 : a.view_camera[ent];
  const int r = a.cam_r[c], rs = a.rs;
  const double nan = undistort::quiet_nan();
  if (!null_view && a.status[ent] != ST_OK) {
    if (lane == 0) { a.gain[e] = nan; a.focus[e] = nan; }
    return;
  }
  double* Lm = lds + wave * SCORE_LDS;
  double* Lb = Lm + MAX_R * MAX_R;
  double* X = Lb + MAX_R * MAX_R;
  double* Yw = X + MAX_R * MAX_R;
  const double* B = a.B + (size_t)c * rs * rs;
  const double* S = null_view ? nullptr : a.S + (size_t)ent * rs * rs;
  bool ok = true;
  if (lane == 0) { form_lower(r, B, S, rs, a.inv_s2, Lm); ok = chol_lower(r, Lm); }
  if (lane == 1) { form_lower(r, B, nullptr, rs, a.inv_s2, Lb); ok = chol_lower(r, Lb); }
  pnp::wave_fence();
  if (__ballot(!ok) != 0ull) {
    if (lane == 0) { a.gain[e] = nan; a.focus[e] = nan; }
    return;
  }
  const int f = a.n_views + c;
  const bool has_focus = a.status[f] == ST_OK && a.n_visible[f] > 0;
  if (has_focus && lane < r) forward_column(r, Lm, a.S + (size_t)f * rs * rs, rs, lane, X);
  pnp::wave_fence();
  if (has_focus && lane < r) diagonal_entry(Lm, X, lane, Yw);
  pnp::wave_fence();
  if (lane == 0) {
    a.gain[e] = half_log_det(r, Lm) - half_log_det(r, Lb);
    double trace = 0.0;
    for (int i = 0; has_focus && i < r; ++i) trace += Yw[i * MAX_R + i];
    a.focus[e] = has_focus ? focus_rms_of(trace, (double)a.n_visible[f]) : nan;
  }
  if (a.posterior && null_view) {
    pnp::wave_fence();
    if (lane < r) inverse_column(r, Lm, lane, Yw, a.posterior + (size_t)c * rs * rs, rs);
  }
}

// B_c += inv_s2 S_winner; one workgroup per camera
__global__ __launch_bounds__(64) void k_base_add(const int32_t* winners, const int32_t* cam_r, const double* S, double* B, int rs,
                                                 double inv_s2) {
  const int c = blockIdx.x, w = winners[c], r = cam_r[c];
  if (w < 0) return;
  for (int e = threadIdx.x; e < r * r; e += 64) {
    const int at = (e / r) * rs + e % r;
    B[(size_t)c * rs * rs + at] = B[(size_t)c * rs * rs + at] + inv_s2 * S[(size_t)w * rs * rs + at];
  }
}

void schur_launch(const SchurArgs& a, int n_launch, hipStream_t st);                 // mcba_guidance.hip
void score_launch(const ScoreArgs& a, hipStream_t st);
void base_add_launch(const int32_t* winners, const int32_t* cam_r, const double* S, double* B, int rs, double inv_s2, int C,
                     hipStream_t st);

}  // namespace guidance
}  // namespace mcba
