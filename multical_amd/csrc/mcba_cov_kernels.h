// Kernels of the parameter covariance (mcba_covariance).
//
// In the Jacobi-scaled space A = D H D (D = diag(H)^-1/2, 0 for held and unobserved parameters, which get a unit diagonal) the
// per-frame blocks are eliminated exactly as in the solver (k_schur_frame<DF, true>: A_ff = L_f L_f^T, W_f = L_f^-1 A_fs) and the
// reduced system S = A_ss - sum_f W_f^T W_f is formed by the solver's SYRK / k_schur_reduce<true> and factored by the panel
// Cholesky (which writes L back).  Then
//     Sigma_ss = S^-1 = L^-T L^-1           k_cov_trinv (L^-1) + k_schur_syrk (L^-T L^-1) + k_cov_fold
//     V_f      = L_f^-T W_f
//     Sigma_fs = -V_f Sigma_ss              k_cov_frame (one workgroup per frame, the hot path)
//     Sigma_ff = L_f^-T L_f^-1 + V_f Sigma_ss V_f^T = L_f^-T L_f^-1 - Sigma_fs V_f^T
// and every output is unscaled as sigma^2 D Sigma D on the way out.
#pragma once

namespace mcba {

constexpr int COV_PIVOT_NONE = 0x7fffffff;
constexpr double COV_PIVOT_MIN = 1e-10;   // smallest admissible L_kk^2 in the scaled space (every diagonal entry of A is 1)

// bad[0] = smallest x index (internal order) of a frame parameter whose pivot L_ii^2 < COV_PIVOT_MIN, bad[1] the same for the
// reduced system; COV_PIVOT_NONE = none.  Lf keeps 1 / L_ii on its diagonal; the panel factor keeps L_kk on the diagonal of buf.
// (NaN -- what a non-positive pivot leaves behind in both factors -- fails the test as well.)
__global__ __launch_bounds__(256) void k_cov_pivots(Dims d, const double* __restrict__ Lf, const double* __restrict__ L,
                                                    int* __restrict__ bad) {
  const int nf = d.DF * d.Fl, ns = d.ns;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nf + ns; e += gridDim.x * blockDim.x) {
    if (e < nf) {
      const int fl = e / d.DF, i = e % d.DF;
      const double dinv = Lf[(size_t)fl * d.DF * d.DF + i * d.DF + i];
      if (!(dinv * dinv * COV_PIVOT_MIN <= 1.0)) atomicMin(bad, d.frame_to_x(d.f0 + fl, i));
    } else {
      const int k = e - nf;
      const double l = L[(size_t)k * ns + k];
      if (!(l * l >= COV_PIVOT_MIN)) atomicMin(bad + 1, d.shared_to_x(k));
    }
  }
}

// X = L^-1 (lower triangular, ns x ns, row stride ns; the caller zeroes the upper triangle) from the panel factor L (lower
// triangle of buf, row stride ns) and its inverted diagonal tiles Ld (chol_linv: [nbc][16][16], L_kk^-1).  One workgroup per
// 16-column block j, one thread per entry of a 16 x 16 tile; the block column of X lives in LDS while it is formed by the
// blocked forward substitution  X_jj = L_jj^-1,  X_ij = -L_ii^-1 sum_{k=j}^{i-1} L_ik X_kj.  (ns^3 / 3 flops: not the hot path.)
constexpr int COV_TRINV_THREADS = 256;
__host__ __device__ inline size_t cov_trinv_lds_bytes(int ns) {
  const int nbc = (ns + CT - 1) / CT;
  return ((size_t)nbc * CT * CT + CT * CTL) * sizeof(double);
}
__global__ __launch_bounds__(COV_TRINV_THREADS) void k_cov_trinv(int ns, const double* __restrict__ L,
                                                                 const double* __restrict__ Ld, double* __restrict__ X) {
  extern __shared__ __attribute__((aligned(16))) double cov_xs[];
  const int nbc = (ns + CT - 1) / CT, j = blockIdx.x;
  const int tid = threadIdx.x, r = tid >> 4, c = tid & 15;
  double* Xs = cov_xs;                       // rows 16 j .. 16 nbc of the block column, [row - 16 j][16]
  double* T = Xs + (size_t)(nbc - j) * CT * CT;
  Xs[r * CT + c] = Ld[(size_t)j * CT * CT + r * CT + c];
  __syncthreads();
  for (int i = j + 1; i < nbc; ++i) {
    const int gi = CT * i + r;
    double s0 = 0.0, s1 = 0.0;
    if (gi < ns) {
      const double* li = L + (size_t)gi * ns;
      for (int k = CT * j; k < CT * i; k += 2) {   // (16 i <= ns - 1: both columns exist)
        s0 += li[k] * Xs[(k - CT * j) * CT + c];
        s1 += li[k + 1] * Xs[(k + 1 - CT * j) * CT + c];
      }
    }
    T[r * CTL + c] = s0 + s1;
    __syncthreads();
    const double* ldi = Ld + (size_t)i * CT * CT + r * CT;
    double x = 0.0;
#pragma unroll
    for (int q = 0; q < CT; ++q) x -= ldi[q] * T[q * CTL + c];
    Xs[(CT * (i - j) + r) * CT + c] = x;
    __syncthreads();
  }
  for (int e = tid; e < (nbc - j) * CT * CT; e += COV_TRINV_THREADS) {
    const int row = CT * j + e / CT, col = CT * j + (e % CT);
    if (row < ns && col < ns && col <= row) X[(size_t)row * ns + col] = Xs[e];
  }
}

// Sigma_ss (scaled) from the partial SYRK tiles of X^T X (k_schur_syrk layout: P[split][upper tile (ti <= tj)][16 x 16] holds
// the LOWER block S[16 tj + row][16 ti + col]).  Sg: both triangles, row stride nsp (a multiple of 16), zero behind ns -- the
// operand of k_cov_frame.  Sout: sigma^2 D Sigma_ss D in the internal shared order, ns x ns.
__global__ __launch_bounds__(256) void k_cov_fold(Dims d, const double* __restrict__ P, int ntile, int ksplit,
                                                  const double* __restrict__ dcov, double sigma2, int nsp,
                                                  double* __restrict__ Sg, double* __restrict__ Sout) {
  const int ns = d.ns, nt2 = ntile * (ntile + 1) / 2;
  const size_t total = (size_t)nsp * nsp;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(e / nsp), j = (int)(e % nsp);
    double v = 0.0;
    if (i < ns && j < ns) {
      const int a = min(i, j), b = max(i, j), ti = a / 16, tj = b / 16;
      const int tile = ti * ntile - (ti * (ti - 1)) / 2 + (tj - ti);
      const double* pp = P + (size_t)tile * 256 + (b % 16) * 16 + (a % 16);
      double s0 = 0.0, s1 = 0.0;
      int sp = 0;
      for (; sp + 1 < ksplit; sp += 2) {
        s0 += pp[(size_t)sp * nt2 * 256];
        s1 += pp[(size_t)(sp + 1) * nt2 * 256];
      }
      if (sp < ksplit) s0 += pp[(size_t)sp * nt2 * 256];
      v = s0 + s1;
      Sout[(size_t)i * ns + j] = sigma2 * dcov[d.shared_to_x(i)] * v * dcov[d.shared_to_x(j)];
    }
    Sg[e] = v;
  }
}

// Per-frame marginal blocks.  One workgroup of COV_FRAME_WAVES wavefronts per frame:
//   (1) V_f = L_f^-T W_f (DF x ns, rows padded to 16 with zeros) into LDS, thread s solving column s; L_f^-1 by wave 0;
//   (2) every wavefront takes 16-column tiles of Sigma_ss in turn: Sigma_fs[:, tile] = -V_f Sigma_ss[:, tile] with
//       v_mfma_f64_16x16x4_f64 (A = V_f from LDS, B = four rows of the tile straight from L2: 16 lanes read 128 contiguous
//       bytes), written out unscaled if asked for, and folded at once into its share of  Sigma_fs V_f^T  (four more MFMAs
//       with the tile transposed through a wave-private LDS scratch tile);
//   (3) the wavefront shares are summed in a fixed order and Sigma_ff = L_f^-T L_f^-1 - Sigma_fs V_f^T is unscaled.
// Sigma_ss is read once per frame (F nsp^2 8 B in all, from L2 / MALL: 663 KB at ns = 286 stays resident).
constexpr int COV_FRAME_WAVES = 4, COV_FRAME_THREADS = 64 * COV_FRAME_WAVES;
__host__ __device__ inline int cov_frame_ldv(int nsp) { return nsp + 1; }   // (odd stride: the 16 rows of an A operand hit 16 banks)
__host__ __device__ inline size_t cov_frame_lds_bytes(int nsp) {
  return ((size_t)CT * cov_frame_ldv(nsp) + (size_t)COV_FRAME_WAVES * CT * CTL + (size_t)COV_FRAME_WAVES * 256 + 2 * CT * CTL + 2 * CT) *
         sizeof(double);
}
template <int DF>
__global__ __launch_bounds__(COV_FRAME_THREADS) void k_cov_frame(Dims d, const double* __restrict__ Lf, const double* __restrict__ W,
                                                                 const double* __restrict__ Sg, int nsp, const double* __restrict__ dcov,
                                                                 double sigma2, double* __restrict__ cov_ff, double* __restrict__ cov_fs) {
  extern __shared__ __attribute__((aligned(16))) double cov_fr[];
  const int ldv = cov_frame_ldv(nsp);
  double* Vs = cov_fr;                                       // [16][ldv]
  double* Ts = Vs + (size_t)CT * ldv;                        // [waves][16][CTL]  Sigma_fs tile of a wavefront
  double* red = Ts + (size_t)COV_FRAME_WAVES * CT * CTL;     // [waves][256]      shares of Sigma_fs V^T
  double* Ls = red + (size_t)COV_FRAME_WAVES * 256;          // [16][CTL]         L_f (strict lower) with 1 / L_ii on the diagonal
  double* Li = Ls + CT * CTL;                                // [16][CTL]         L_f^-1
  double* ds = Li + CT * CTL;                                // [16]              D of the frame's parameters
  const int fl = blockIdx.x, f = d.f0 + fl, ns = d.ns, ldw = ns + 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, rsub = lane >> 4, csub = lane & 15;
  if (tid < DF * DF) Ls[(tid / DF) * CTL + tid % DF] = Lf[(size_t)fl * DF * DF + tid];
  if (tid >= 64 && tid < 64 + CT) ds[tid - 64] = (tid - 64) < DF ? dcov[d.frame_to_x(f, tid - 64)] : 0.0;
  __syncthreads();
  // (1) V = L^-T W: back substitution per column; rows DF .. 15 and columns behind ns are zero
  const double* w = W + (size_t)fl * DF * ldw;
  for (int s = tid; s < nsp; s += COV_FRAME_THREADS) {
    double v[DF];
#pragma unroll
    for (int i = 0; i < DF; ++i) v[i] = s < ns ? w[(size_t)i * ldw + s] : 0.0;
#pragma unroll
    for (int i = DF - 1; i >= 0; --i) {
      double a = v[i];
#pragma unroll
      for (int m = i + 1; m < DF; ++m) a -= Ls[m * CTL + i] * v[m];
      v[i] = a * Ls[i * CTL + i];
    }
#pragma unroll
    for (int i = 0; i < CT; ++i) Vs[(size_t)i * ldv + s] = i < DF ? v[i] : 0.0;
  }
  if (tid < DF) {   // column tid of L^-1 by forward substitution
    double x[DF];
#pragma unroll
    for (int i = 0; i < DF; ++i) {
      double a = (i == tid) ? 1.0 : 0.0;
#pragma unroll
      for (int m = 0; m < i; ++m) a -= Ls[i * CTL + m] * x[m];
      x[i] = a * Ls[i * CTL + i];
    }
#pragma unroll
    for (int i = 0; i < DF; ++i) Li[i * CTL + tid] = x[i];
  }
  __syncthreads();
  // (2) Sigma_fs tiles on the matrix pipe
  double* tw = Ts + (size_t)wave * CT * CTL;
  double4_t ff = {0.0, 0.0, 0.0, 0.0};
  const int nct = nsp / CT;
  const double* va = Vs + (size_t)csub * ldv + rsub;         // A[i = csub][k = rsub] = V[csub][k0 + rsub]
  for (int ct = wave; ct < nct; ct += COV_FRAME_WAVES) {
    const double* sb = Sg + (size_t)rsub * nsp + CT * ct + csub;   // B[k = rsub][j = csub] = Sigma_ss[k0 + rsub][16 ct + csub]
    double4_t acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    constexpr int UB = 8;                                   // (eight K steps of loads in flight before their MFMAs)
    int k = 0;
    for (; k + 4 * UB <= nsp; k += 4 * UB) {
      double b[UB];
#pragma unroll
      for (int u = 0; u < UB; ++u) b[u] = sb[(size_t)(k + 4 * u) * nsp];
#pragma unroll
      for (int u = 0; u < UB; u += 2) {
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(va[k + 4 * u], b[u], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(va[k + 4 * u + 4], b[u + 1], acc1, 0, 0, 0);
      }
    }
    for (; k < nsp; k += 4) acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(va[k], sb[(size_t)k * nsp], acc0, 0, 0, 0);
    // lane holds Sigma_fs[i = rsub + 4 r][16 ct + csub]
    const int s = CT * ct + csub;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = rsub + 4 * r;
      const double v = -(acc0[r] + acc1[r]);
      tw[i * CTL + csub] = v;
      if (cov_fs != nullptr && i < DF && s < ns)
        cov_fs[((size_t)fl * DF + i) * ns + s] = sigma2 * ds[i] * v * dcov[d.shared_to_x(s)];
    }
    lds_fence();
    // Sigma_fs[:, tile] V[:, tile]^T: A[i][k] = Sigma_fs[i][16 ct + k], B[k][j] = V[j][16 ct + k]
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
      ff = __builtin_amdgcn_mfma_f64_16x16x4f64(tw[csub * CTL + 4 * kk + rsub], Vs[(size_t)csub * ldv + CT * ct + 4 * kk + rsub], ff, 0, 0,
                                                0);
    lds_fence();   // (the next tile rewrites tw)
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) red[wave * 256 + (rsub + 4 * r) * CT + csub] = ff[r];
  __syncthreads();
  // (3) Sigma_ff = L^-T L^-1 - Sigma_fs V^T, unscaled
  if (tid < DF * DF) {
    const int i = tid / DF, j = tid % DF;
    double a = 0.0;
#pragma unroll
    for (int m = 0; m < DF; ++m) a += Li[m * CTL + i] * Li[m * CTL + j];
    double b = 0.0;
#pragma unroll
    for (int q = 0; q < COV_FRAME_WAVES; ++q) b += red[q * 256 + i * CT + j];
    cov_ff[(size_t)fl * DF * DF + tid] = sigma2 * ds[i] * (a - b) * ds[j];
  }
}

}  // namespace mcba
