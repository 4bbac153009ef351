// mcba_handeye_kernels.h -- k_hand_eye: the robot-world hand-eye closed form of mcba_handeye.h, one wavefront per problem.
//
// Launched over the list of problems (index pairs into the two pose tables); a 64-thread workgroup each, no barrier.
//   * sweep 1: lanes stride over the frames, 64 a chunk.  A lane reads both validity bytes and, where both are set, the two poses
//     (inverted rigidly if asked); the usable pairs of the chunk are compacted by a ballot + prefix count, so row r of the staging
//     buffer is the chunk's r-th usable pair in frame order: vec(R_A) | vec(R_B), 18 doubles.  G = sum vec(R_A) vec(R_B)^T is the
//     product [9 x n] [n x 9] of those rows: v_mfma_f64_16x16x4_f64, four pairs an instruction, operand lane l holding row
//     4 s + (l >> 4), column l & 15 (columns 9 .. 15 are zeros the lanes supply themselves, the rows of the last group of four that
//     hold no pair are zeroed in LDS), accumulated over the chunks in the instruction's accumulator.  (A VALU form of the same sum
//     -- lane l owning entries l and l + 64 of the 81 and walking the staged rows -- measured 0.166 / 0.143 ms against 0.160 /
//     0.139 ms for this one at the cfg5 / cfg5_40 problem lists, profiles/hand_eye_timing.txt: not faster, not kept.)  sum R_A and
//     the count are lane partials folded by the xor butterfly.
//   * G goes to LDS and is read back by every lane (broadcast reads at constant offsets): the 9x9 Jacobi sweeps, the two
//     projections and the 6x6 solve run redundantly in all 64 lanes on identical bits, as k_view_pose does for its 9x9 -- control
//     flow stays uniform without a broadcast.
//   * sweep 2 (the 6 right-hand-side sums, R_Z known) and sweep 3 (err, X and Z known) walk the frames again, each lane its own,
//     re-reading the poses (the rows of a problem are 2 x F x 128 bytes, L2-resident after sweep 1) -- no staging of all pairs, so
//     F is not bounded by LDS.  err is written by the lane that owns the frame, 0 for frames that did not enter.
// Every sum has a fixed order: two calls return the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include "mcba_handeye.h"
#include "mcba_pnp_kernels.h"

namespace mcba {
namespace handeye {

struct HandEyeArgs {
  int n_problems, F, invert;
  const double* table_a;      // [n_a][F][16]
  const uint8_t* valid_a;     // [n_a][F]
  const double* table_b;      // [n_b][F][16]
  const uint8_t* valid_b;     // [n_b][F]
  const int32_t* index_a;     // [n_problems]
  const int32_t* index_b;     // [n_problems]
  double* X;                  // [n_problems][16]
  double* Z;                  // [n_problems][16]
  int32_t* n_pairs;           // [n_problems]
  uint8_t* status;            // [n_problems]
  double* err;                // [n_problems][F] or null
};

constexpr int HE_ROW = 18;     // vec(R_A) | vec(R_B)
constexpr int HE_CHUNK = 64;

__global__ __launch_bounds__(64) void k_hand_eye(HandEyeArgs a) {
  __shared__ double V[HE_CHUNK * HE_ROW];
  __shared__ double Gs[81];
  const int k = blockIdx.x, lane = threadIdx.x;
  if (k >= a.n_problems) return;
  const size_t ia = (size_t)a.index_a[k], ib = (size_t)a.index_b[k];
  const double* ta = a.table_a + ia * a.F * 16;
  const double* tb = a.table_b + ib * a.F * 16;
  const uint8_t* va = a.valid_a + ia * a.F;
  const uint8_t* vb = a.valid_b + ib * a.F;
  const bool inv = a.invert != 0;
  const int rsub = lane >> 4, csub = lane & 15;

  // ---- sweep 1: G, sum R_A, count ----
  pnp::wave_double4 acc = {0.0, 0.0, 0.0, 0.0};
  double sums[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) sums[i] = 0.0;
  for (int base = 0; base < a.F; base += HE_CHUNK) {
    const int f = base + lane;
    const bool good = f < a.F && va[f < a.F ? f : 0] != 0 && vb[f < a.F ? f : 0] != 0;
    const unsigned long long mask = __ballot(good);
    const int m = __popcll(mask);
    if (m == 0) continue;                                // (wave-uniform)
    const int row = __popcll(mask & ((1ull << lane) - 1ull));
    if (good) {
      double RA[9], tA[3], RB[9], tB[3];
      load_pose(ta + (size_t)f * 16, inv, RA, tA);
      load_pose(tb + (size_t)f * 16, inv, RB, tB);
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        V[row * HE_ROW + i] = RA[i];
        V[row * HE_ROW + 9 + i] = RB[i];
        sums[i] += RA[i];
      }
      sums[9] += 1.0;
    }
    const int m4 = (m + 3) & ~3;                         // (<= 64: the rows of the buffer)
    if (lane >= m && lane < m4) {
#pragma unroll
      for (int i = 0; i < HE_ROW; ++i) V[lane * HE_ROW + i] = 0.0;
    }
    pnp::wave_fence();
    const double* vp = V + rsub * HE_ROW + (csub < 9 ? csub : 0);
    for (int st = 0; st < (m4 >> 2); ++st) {
      const double x = vp[(4 * st) * HE_ROW], y = vp[(4 * st) * HE_ROW + 9];
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(csub < 9 ? x : 0.0, csub < 9 ? y : 0.0, acc, 0, 0, 0);
    }
    pnp::wave_fence();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (rsub + 4 * r < 9 && csub < 9) Gs[(rsub + 4 * r) * 9 + csub] = acc[r];
  pnp::wave_fence();
#pragma unroll
  for (int i = 0; i < 10; ++i) sums[i] = pnp::wave_xor_sum(sums[i]);
  const int n = (int)(sums[9] + 0.5);

  // ---- the closed form, redundantly in every lane ----
  double RX[9], RZ[9], tX[3] = {0.0, 0.0, 0.0}, tZ[3] = {0.0, 0.0, 0.0};
  bool ok = n >= MIN_PAIRS;
  if (ok) {
    double v[9];
    ok = leading_vector(Gs, v);
    pnp::wave_fence();                                     // (G is read again from LDS instead of living through the sweeps)
    ok = ok && rotations_of_vector(Gs, v, RX, RZ);
  }
  if (ok) {
    // ---- sweep 2: right-hand side of the translation system ----
    double rhs[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int f = lane; f < a.F; f += 64)
      if (va[f] != 0 && vb[f] != 0) {
        double RA[9], tA[3], RB[9], tB[3], q[6];
        load_pose(ta + (size_t)f * 16, inv, RA, tA);
        load_pose(tb + (size_t)f * 16, inv, RB, tB);
        rhs_terms(RA, tA, tB, RZ, q);
#pragma unroll
        for (int i = 0; i < 6; ++i) rhs[i] += q[i];
      }
#pragma unroll
    for (int i = 0; i < 6; ++i) rhs[i] = pnp::wave_xor_sum(rhs[i]);
    ok = solve_translations(sums, rhs, (double)n, tX, tZ);
    ok = ok && all_finite(RX, 9) && all_finite(RZ, 9) && all_finite(tX, 3) && all_finite(tZ, 3);
  }

  // ---- sweep 3: residuals; outputs ----
  if (a.err != nullptr) {
    double* e = a.err + (size_t)k * a.F;
    for (int f = lane; f < a.F; f += 64) {
      double r = 0.0;
      if (ok && va[f] != 0 && vb[f] != 0) {
        double RA[9], tA[3], RB[9], tB[3];
        load_pose(ta + (size_t)f * 16, inv, RA, tA);
        load_pose(tb + (size_t)f * 16, inv, RB, tB);
        r = pair_error(RA, tA, RB, tB, RX, tX, RZ, tZ);
      }
      e[f] = r;
    }
  }
  double Xm[16], Zm[16];
  if (ok) {
    store_pose(RX, tX, Xm);
    store_pose(RZ, tZ, Zm);
  } else {
    identity_pose(Xm);
    identity_pose(Zm);
  }
  if (lane < 32) {
    const int i = lane & 15;
    double x = Xm[0], z = Zm[0];
#pragma unroll
    for (int j = 1; j < 16; ++j) { x = (i == j) ? Xm[j] : x; z = (i == j) ? Zm[j] : z; }
    if (lane < 16) a.X[(size_t)k * 16 + i] = x;
    else a.Z[(size_t)k * 16 + i] = z;
  }
  if (lane == 0) {
    a.n_pairs[k] = n;
    a.status[k] = (uint8_t)(ok ? ST_OK : n < MIN_PAIRS ? ST_TOO_FEW : ST_DEGENERATE);
  }
}

void hand_eye_launch(const HandEyeArgs& a, hipStream_t st);   // mcba_handeye.hip

}  // namespace handeye
}  // namespace mcba
