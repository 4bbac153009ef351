// mcba_rigview_kernels.h -- the kernels of mcba_rigview.h.
//
// k_rig_gram: ONE WORKGROUP OF 128 THREADS PER SLOT (view, camera): the front end of k_view_schur (guidance::wave_gram_tiles: lanes,
// chunks of 64 points, rows in LDS at a 25-double stride, the half-filled last K-step, three f64 MFMA tiles) with the raw rows
// [K | P'] of 24 columns; the two wave tiles are added in wave order and G_vc is written full and symmetric with the visible count.
// Every register array is indexed by compile-time constants: no scratch.
// k_focus_gram: one workgroup of 256 threads per focus pair (a, b): the pixels of the grid in chunks of 64, thread l < 64 writes the
// row pair J of pixel l (uncertainty::query_rows; zero unless OK) to LDS, every thread adds the chunk to its entries of sum J^T J
// [KP][KP] in pixel order.
// k_rig_assemble: one workgroup of 256 threads per view, the contributing cameras one after the other in camera order: W'_c and
// T = G_vc W'_c staged in LDS, thread (ti, tj) = (tid / 16, tid % 16) holds the entries (ti + 16 p, tj + 16 q), p >= q, of
// sum_c W_c^T T_c in registers (36 blocks of the lower triangle), U and G_xx accumulate in LDS; then the 6 x 6 Cholesky (thread 0),
// Y = L^-1 U (a thread per column), S = sum - Y^T Y, written with its mirror image.  A view that is not OK gets S = 0.
// k_rig_score: ONE WORKGROUP OF 256 THREADS PER ENTRY of the score list (a candidate, or -1: the base alone).  M = B + S / sigma^2
// sits once in dynamic LDS at the odd stride score_stride(r) (r = 128: 129 x 128 doubles and 3 r + 8 more = 132 KiB of the CU's 160): right-looking
// Cholesky in place, triangular inverse in place row by row (the row of L that is being replaced is read from a copy, double
// buffered: one barrier a row), thread i forms X[i, :] Q X[i, :]^T, thread 0 adds them in index order.  With `posterior` the base
// alone also writes X^T X.
// k_rig_base_add: B += S_winner / sigma^2.
// No atomics, no cross-block waits, every sum has a fixed order: two calls return the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include "mcba_gram_front.h"
#include "mcba_rigview.h"

namespace mcba {
namespace rigview {

struct GramArgs {
  const int32_t* launch;         // [grid] the slots that are served
  const double* srecs;           // [V C][S_STRIDE]
  const double* crecs;           // [C][RC_STRIDE]
  const double* board_points;    // [B][board_stride][3]
  int board_stride;
  double* G;                     // [V C][KC][KC]
  int32_t* n_visible;            // [V C]
};

struct FocusArgs {
  const double* frecs;           // [n_pairs][F_STRIDE]
  int gw, n;                     // the grid of the reference camera
  double u0, v0, du, dv;
  double* H;                     // [n_pairs][KP][KP]
  int32_t* n_ok;                 // [n_pairs]
};

struct AssembleArgs {
  int C, r, rs, min_cameras;
  const double* srecs;
  const double* G;
  const int32_t* n_visible;      // [V C]
  const double* W;               // [C][KC][rs]
  const uint8_t* loose;          // [C]
  double* S;                     // [V][rs][rs]
  int32_t* n_cameras;            // [V]
  uint8_t* status;               // [V]
};

struct ScoreArgs {
  int r, rs, ld;
  const int32_t* entries;        // [grid] view, or -1: the base alone
  const double* S;               // [V][rs][rs]
  const uint8_t* status;         // [V]
  const double* B;               // [rs][rs]
  const double* Q;               // [rs][rs] or null: no focus
  double n_focus;
  double inv_s2;
  double* half_log_det;          // [grid]
  double* focus;                 // [grid]
  double* posterior;             // [rs][rs] or null
};

constexpr int GRAM_THREADS = guidance::SCHUR_THREADS, GRAM_WAVES = guidance::SCHUR_WAVES;
static_assert(KC < guidance::LDV && KC <= GS, "a staged row holds the 24 columns");
constexpr int LG_CREC = 0, LG_SREC = LG_CREC + RC_STRIDE, LG_STAGE = LG_SREC + S_STRIDE, LG_SC = LG_STAGE + GRAM_WAVES * guidance::STAGE,
              LG_END = LG_SC + 8;
static_assert((size_t)LG_END * sizeof(double) <= 65536, "static LDS of k_rig_gram");

__global__ __launch_bounds__(GRAM_THREADS) void k_rig_gram(GramArgs a) {
  __shared__ double lds[LG_END];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int slot = a.launch[blockIdx.x];
  const double* ssrc = a.srecs + (size_t)slot * S_STRIDE;
  const double* csrc = a.crecs + (size_t)(int)ssrc[guidance::V_CAMERA] * RC_STRIDE;
  if (tid < S_STRIDE) lds[LG_SREC + tid] = ssrc[tid];
  for (int i = tid; i < RC_STRIDE; i += GRAM_THREADS) lds[LG_CREC + i] = csrc[i];
  for (int i = tid; i < GRAM_WAVES * guidance::STAGE; i += GRAM_THREADS) lds[LG_STAGE + i] = 0.0;
  __syncthreads();
  const double* crec = lds + LG_CREC;
  const double* srec = lds + LG_SREC;
  const int n = (int)srec[guidance::V_N];
  double* V = lds + LG_STAGE + wave * guidance::STAGE;
  const int count = guidance::wave_gram_tiles(V, n, KC, wave, lane, [&](int i, double* row_u, double* row_v) {
    return point_rows(crec, srec, a.board_points, a.board_stride, i, row_u, row_v);
  });
  if (lane == 0) lds[LG_SC + wave] = (double)count;
  __syncthreads();
  const double* T0 = lds + LG_STAGE;
  double* G = a.G + (size_t)slot * KC * KC;
  for (int e = tid; e < KC * KC; e += GRAM_THREADS) {
    const int i = e / KC, j = e % KC, at = i <= j ? i * GS + j : j * GS + i;
    G[e] = T0[at] + T0[guidance::STAGE + at];
  }
  if (tid == 0) a.n_visible[slot] = (int)(lds[LG_SC] + lds[LG_SC + 1]);
}
static_assert(GRAM_WAVES == 2, "k_rig_gram adds two wave tiles");

constexpr int FOCUS_THREADS = 256, FOCUS_CHUNK = 64, FOCUS_ENTRIES = KP * KP / FOCUS_THREADS;
static_assert(KP * KP % FOCUS_THREADS == 0, "the entries of sum J^T J divide among the threads");
constexpr int LF_REC = 0, LF_J = LF_REC + F_STRIDE, LF_OK = LF_J + FOCUS_CHUNK * 2 * KP, LF_END = LF_OK + FOCUS_CHUNK;
static_assert((size_t)LF_END * sizeof(double) <= 65536, "static LDS of k_focus_gram");

__global__ __launch_bounds__(FOCUS_THREADS) void k_focus_gram(FocusArgs a) {
  __shared__ double lds[LF_END];
  const int tid = threadIdx.x, pair = blockIdx.x;
  for (int i = tid; i < F_STRIDE; i += FOCUS_THREADS) lds[LF_REC + i] = a.frecs[(size_t)pair * F_STRIDE + i];
  __syncthreads();
  const double* rec = lds + LF_REC;
  double acc[FOCUS_ENTRIES];
#pragma unroll
  for (int q = 0; q < FOCUS_ENTRIES; ++q) acc[q] = 0.0;
  int n_ok = 0;                                                   // (thread 0's is the pair's)
  for (int base = 0; base < a.n; base += FOCUS_CHUNK) {           // (uniform over the workgroup)
    if (tid < FOCUS_CHUNK) {
      double* J = lds + LF_J + tid * 2 * KP;
      const int i = base + tid;
      bool ok = false;
      if (i < a.n) {
        double u, v;
        uncertainty::grid_pixel(i, a.gw, a.u0, a.v0, a.du, a.dv, u, v);
        ok = uncertainty::query_rows(rec, u, v, J) == uncertainty::ST_OK;
      }
      if (!ok)
        for (int k = 0; k < 2 * KP; ++k) J[k] = 0.0;
      lds[LF_OK + tid] = ok ? 1.0 : 0.0;
    }
    __syncthreads();
    if (tid == 0)
      for (int l = 0; l < FOCUS_CHUNK; ++l) n_ok += lds[LF_OK + l] != 0.0 ? 1 : 0;
#pragma unroll
    for (int q = 0; q < FOCUS_ENTRIES; ++q) {
      const int e = tid + FOCUS_THREADS * q, i = e / KP, j = e % KP;
      double s = acc[q];
      for (int l = 0; l < FOCUS_CHUNK; ++l) {
        const double* J = lds + LF_J + l * 2 * KP;
        s += J[i] * J[j];
        s += J[KP + i] * J[KP + j];
      }
      acc[q] = s;
    }
    __syncthreads();
  }
  double* H = a.H + (size_t)pair * KP * KP;
#pragma unroll
  for (int q = 0; q < FOCUS_ENTRIES; ++q) H[tid + FOCUS_THREADS * q] = acc[q];
  if (tid == 0) a.n_ok[pair] = n_ok;
}

constexpr int ASM_THREADS = 256, ASM_B = MAX_R / 16;
constexpr int LA_W = 0, LA_T = LA_W + KC * MAX_R, LA_G = LA_T + KC * MAX_R, LA_D = LA_G + KC * KC, LA_U = LA_D + NN * NN,
              LA_GX = LA_U + NN * MAX_R, LA_L = LA_GX + NN * GS, LA_SC = LA_L + guidance::MAX_NN * guidance::MAX_NN, LA_END = LA_SC + 4;
static_assert((size_t)LA_END * sizeof(double) <= 65536, "static LDS of k_rig_assemble");
static_assert(MAX_R % 16 == 0 && ASM_THREADS == 256, "a thread holds the entries (ti + 16 p, tj + 16 q)");

__global__ __launch_bounds__(ASM_THREADS) void k_rig_assemble(AssembleArgs a) {
  __shared__ double lds[LA_END];
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15, v = blockIdx.x, r = a.r;
  double* W = lds + LA_W;
  double* T = lds + LA_T;
  double* G = lds + LA_G;
  double* D = lds + LA_D;
  double* U = lds + LA_U;
  double* Gx = lds + LA_GX;
  double* L = lds + LA_L;
  for (int e = tid; e < NN * MAX_R; e += ASM_THREADS) U[e] = 0.0;
  for (int e = tid; e < NN * GS; e += ASM_THREADS) Gx[e] = 0.0;
  double acc[ASM_B][ASM_B];
#pragma unroll
  for (int p = 0; p < ASM_B; ++p)
#pragma unroll
    for (int q = 0; q < ASM_B; ++q) acc[p][q] = 0.0;
  int n_cameras = 0;
  bool loose = false;
  for (int c = 0; c < a.C; ++c) {                                 // (uniform over the workgroup)
    const size_t slot = (size_t)v * a.C + c;
    const double* srec = a.srecs + slot * S_STRIDE;
    if (!contributes(a.n_visible[slot], (int)srec[guidance::V_MIN])) continue;
    ++n_cameras;
    loose = loose || a.loose[c] != 0;
    __syncthreads();                                              // (the last camera's W and T have been read)
    for (int e = tid; e < KC * MAX_R; e += ASM_THREADS) {
      const int k = e / MAX_R, j = e % MAX_R;
      W[e] = j < r ? centred_w(a.W + (size_t)c * KC * a.rs, a.rs, srec + guidance::V_CENTRE, k, j) : 0.0;
    }
    for (int e = tid; e < KC * KC; e += ASM_THREADS) G[e] = a.G[slot * KC * KC + e];
    if (tid < NN * NN) D[tid] = srec[S_D + tid];
    __syncthreads();
    for (int e = tid; e < KC * MAX_R; e += ASM_THREADS) T[e] = gw_entry(G, W, MAX_R, e / MAX_R, e % MAX_R);
    __syncthreads();
    for (int e = tid; e < NN * MAX_R; e += ASM_THREADS) U[e] = U[e] + du_entry(D, T, MAX_R, e / MAX_R, e % MAX_R);
    if (tid < NN * NN) Gx[(tid / NN) * GS + tid % NN] = Gx[(tid / NN) * GS + tid % NN] + gxx_entry(D, G, tid / NN, tid % NN);
    for (int k = 0; k < KC; ++k) {
      double w[ASM_B], t[ASM_B];
#pragma unroll
      for (int p = 0; p < ASM_B; ++p) {
        w[p] = W[k * MAX_R + ti + 16 * p];
        t[p] = T[k * MAX_R + tj + 16 * p];
      }
#pragma unroll
      for (int p = 0; p < ASM_B; ++p)
#pragma unroll
        for (int q = 0; q <= p; ++q) acc[p][q] += w[p] * t[q];
    }
  }
  __syncthreads();
  if (tid == 0) lds[LA_SC] = (n_cameras > 0 && guidance::nuisance_factor(Gx, 0, NN, L)) ? 1.0 : 0.0;
  __syncthreads();
  const int status = view_status(n_cameras, a.min_cameras, loose, lds[LA_SC] != 0.0);      // (uniform over the workgroup)
  if (status == ST_OK) {
    if (tid < r) nuisance_solve(L, U, MAX_R, tid);
    __syncthreads();
  }
  double* S = a.S + (size_t)v * a.rs * a.rs;
#pragma unroll
  for (int p = 0; p < ASM_B; ++p)
#pragma unroll
    for (int q = 0; q <= p; ++q) {
      const int i = ti + 16 * p, j = tj + 16 * q;
      if (i < r && j <= i) {
        const double s = status == ST_OK ? yty_sub(U, MAX_R, i, j, acc[p][q]) : 0.0;
        S[(size_t)i * a.rs + j] = s;
        S[(size_t)j * a.rs + i] = s;
      }
    }
  if (tid == 0) {
    a.n_cameras[v] = n_cameras;
    a.status[v] = (uint8_t)status;
  }
}

constexpr int SCORE_THREADS = 256;
// dynamic LDS of k_rig_score in doubles: M | two row copies | the thread values | the pivot flag
MCBA_HD size_t score_lds_doubles(int r) { return (size_t)r * score_stride(r) + 3 * (size_t)r + 8; }

__global__ __launch_bounds__(SCORE_THREADS) void k_rig_score(ScoreArgs a) {
  extern __shared__ double dyn[];
  const int tid = threadIdx.x, e = blockIdx.x, r = a.r, ld = a.ld, rs = a.rs;
  const int ent = a.entries[e];
  const double nan = undistort::quiet_nan();
  if (ent >= 0 && a.status[ent] != ST_OK) {                       // (uniform over the workgroup)
    if (tid == 0) { a.half_log_det[e] = nan; a.focus[e] = nan; }
    return;
  }
  double* M = dyn;
  double* rows = M + (size_t)r * ld;
  double* vals = rows + 2 * r;
  const double* S = ent >= 0 ? a.S + (size_t)ent * rs * rs : nullptr;
  for (int x = tid; x < r * ld; x += SCORE_THREADS) {
    const int i = x / ld, j = x % ld;
    double m = 0.0;
    if (j <= i) {
      m = a.B[(size_t)i * rs + j];
      if (S) m = m + a.inv_s2 * S[(size_t)i * rs + j];
    }
    M[x] = m;
  }
  __syncthreads();
  for (int j = 0; j < r; ++j) {
    const double d = M[j * ld + j];
    if (!(d > 0.0)) {                                             // (every thread reads the same pivot)
      if (tid == 0) { a.half_log_det[e] = nan; a.focus[e] = nan; }
      return;
    }
    const double l = sqrt(d);
    __syncthreads();
    if (tid == 0) M[j * ld + j] = l;
    for (int i = j + 1 + tid; i < r; i += SCORE_THREADS) M[i * ld + j] = M[i * ld + j] / l;
    __syncthreads();
    const int n = r - j - 1;
    for (int x = tid; x < n * n; x += SCORE_THREADS) {
      const int ii = x / n, kk = x % n;
      if (kk <= ii) chol_term(M, ld, j + 1 + ii, j + 1 + kk, j);
    }
    __syncthreads();
  }
  if (tid == 0) a.half_log_det[e] = half_log_det(r, M, ld);
  // X = L^-1 in place, row by row; rows[i & 1] holds row i of L
  if (tid == 0) rows[0] = M[0];
  __syncthreads();
  for (int i = 0; i < r; ++i) {
    const double* row_l = rows + (i & 1) * r;
    if (i + 1 < r)
      for (int k = tid; k <= i + 1; k += SCORE_THREADS) rows[((i + 1) & 1) * r + k] = M[(i + 1) * ld + k];
    for (int j = tid; j <= i; j += SCORE_THREADS) M[i * ld + j] = inverse_entry(M, ld, row_l, i, j);
    __syncthreads();
  }
  const bool has_focus = a.Q != nullptr && a.n_focus > 0.0;
  if (has_focus) {
    for (int i = tid; i < r; i += SCORE_THREADS) vals[i] = trace_row(M, ld, a.Q, rs, i);
    __syncthreads();
  }
  if (tid == 0) {
    double trace = 0.0;
    for (int i = 0; has_focus && i < r; ++i) trace += vals[i];
    a.focus[e] = has_focus ? guidance::focus_rms_of(trace, a.n_focus) : nan;
  }
  if (a.posterior && ent < 0)
    for (int x = tid; x < r * r; x += SCORE_THREADS) a.posterior[(size_t)(x / r) * rs + x % r] = posterior_entry(r, M, ld, x / r, x % r);
}

// B += inv_s2 S_winner
__global__ __launch_bounds__(256) void k_rig_base_add(const double* S, double* B, int r, int rs, double inv_s2) {
  for (int e = blockIdx.x * 256 + threadIdx.x; e < r * r; e += gridDim.x * 256) {
    const size_t at = (size_t)(e / r) * rs + e % r;
    B[at] = B[at] + inv_s2 * S[at];
  }
}

void gram_launch(const GramArgs& a, int n_launch, hipStream_t st);                   // mcba_rigview.hip
void focus_launch(const FocusArgs& a, int n_pairs, hipStream_t st);
void assemble_launch(const AssembleArgs& a, int n_views, hipStream_t st);
void score_launch(const ScoreArgs& a, int n_entries, hipStream_t st);              // throws where the LDS request is refused
void base_add_launch(const double* S_winner, double* B, int r, int rs, double inv_s2, hipStream_t st);

}  // namespace rigview
}  // namespace mcba
