// Kernels of the per-observation prediction covariance (mcba_observation_covariance).
//
// The covariance of the predicted point of table slot i is C_i = J_i Sigma J_i^T (2 x 2), Sigma = sigma^2 (J^T J)^-1 of the
// covariance chain (mcba_cov_kernels.h).  With the per-view factorisation of the Jacobian, J_p = [E_p | K_p] That_e,
// That_e = diag(That, I_KI), NG = DE + KI (NV without the residual column), two routes:
//   whitened (default)  Q = M^-1 D That_e^T per VIEW from the block Cholesky factor M of the scaled system (k_obscov_whiten),
//                       z_p = Q [E_p | K_p]^T and C_p = sigma^2 z_p z_p^T per POINT: a sum of squares;
//   Sigma-route         G = That_e Sigma_view That_e^T per VIEW (NG x NG), C_p = [E_p | K_p] G [E_p | K_p]^T per POINT, Sigma_view the
//                       NL x NL sub-block of Sigma over the view's local parameters gathered from Sigma_ss, Sigma_ff[f], Sigma_fs[f].
//                       NL^2 NG instead of ns^2 NG flops per view, but J Sigma J^T cancels by 1e4 .. 1e7: good for the blocks, not
//                       for 1 - h of a near-unit-leverage inlier.  The fallback when a view's ns x NG panel does not fit LDS.
#pragma once

namespace mcba {

// an inlier whose leverage block H_ii = C_i / sigma^2 has its larger eigenvalue at or above 1 - OBSCOV_EXACT_FIT is fitted exactly
constexpr double OBSCOV_EXACT_FIT = 1e-9;

// larger eigenvalue of the symmetric 2 x 2 matrix (uu uv; uv vv).  One operation per statement: nothing is contracted into an
// FMA, so a caller that repeats these five operations in IEEE double arithmetic gets the same bits (mcba.h states the formula).
__device__ __forceinline__ double sym2_max_eig(double uu, double uv, double vv) {
  const double hs = 0.5 * (uu + vv);
  const double hd = 0.5 * (uu - vv);
  const double a = hd * hd;
  const double b = uv * uv;
  const double r = sqrt(a + b);
  return hs + r;
}

// ---------------------------------------------------------------------------------------------------------------
// k_obscov: ONE WAVEFRONT PER VIEW (single-wave workgroups, views dealt round-robin), over ALL table slots of the view (the mask
// form of the observation table: valid slots that are not inliers get a prediction covariance too).
//   per view : code[l]  = where local parameter l lives in Sigma (shared index / frame-block index / nowhere), flagged[] = the
//                         local parameters that are unobserved and not held (a slot whose row pair touches one is NaN);
//              Tm       = That, lane j forming column j from the pose table (view_that_column: k_tmat's construction);
//              (Sigma-route only:)
//              Sv       = Sigma_view, every lane gathering its entries with unconditional, independent loads;
//              M1       = That Sv[0 .. NPC, :]                       (DE x NL)
//              G        = [M1 That^T, M1[:, NPC ..]; sym, Sv[NPC .., NPC ..]]   in LDS
//   per point: (the valid / inlier slots of the view, ballot-compacted into dense 64-lane chunks; views without any skip the above)
//              the row pair [E_p | K_p | r_p] from point_state / point_row (linear loss, scan time from the OBSERVED row),
//              C_p = sigma^2 z z^T, z = Q rows^T (whitened) or rows G rows^T with G broadcast from LDS, the studentised error from r_p, 24 + 8 B per slot in the
//              reference's [C,F,B,P] order (a view's slots are one contiguous run);
//   per view : vpart[v] = sum over the view's inliers of tr(C_p) / sigma^2, vpart[views + v] = max over its valid slots of
//              sqrt(larger eigenvalue of C_p) -- folded in a fixed order by k_obscov_fold (no float atomics).
// gview != nullptr: the whitened route, Q [views][DF + ns][NG] of k_obscov_whiten (the default; the Sigma-route above stays for
// systems whose ns x NG panel does not fit the LDS of a workgroup).
// Sss: sigma^2 D Sigma_ss D [ns][ns] (internal shared order), Sff: [Fl][DF][DF], Sfs: [Fl][DF][ns] -- k_cov_fold / k_cov_frame.
// ---------------------------------------------------------------------------------------------------------------
template <int ND, int FISH, int MOTION, bool OPTK>
__global__ __launch_bounds__(64) void k_obscov(Dims d, Tables t, const double* __restrict__ Sss, const double* __restrict__ Sff,
                                               const double* __restrict__ Sfs, const uint8_t* __restrict__ pflag, double sigma2,
                                               double* __restrict__ pred_cov, double* __restrict__ student,
                                               double* __restrict__ vpart, const double* __restrict__ gview) {
  using VS = ViewShape<ND, MOTION, OPTK>;
  constexpr bool ROLL = VS::ROLL;
  constexpr int DE = VS::DE, NPC = VS::NPC, KI = VS::KI, NL = NPC + KI, NG = VS::NS, NV = VS::NV;
  constexpr int NE = (NL * NL + 63) / 64;
  static_assert(NL <= 64, "one lane per local parameter");
  __shared__ int code[NL], flagged[NL];
  __shared__ uint16_t pidx[LIN_MAX_POINTS];
  __shared__ double Sv[NL * NL], Tm[DE * NPC], M1[DE * NL], G[NG * NG];
  __shared__ double rowbuf[2 * NG * 64];   // [row a of r0 | r1][lane]
  const int lane = threadIdx.x, nv = d.views(), ns = d.ns, DF = d.DF;
  const double nan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
  for (int v = blockIdx.x; v < nv; v += gridDim.x) {
    const int b = v % d.B, c = (v / d.B) % d.C, fl = v / (d.B * d.C), f = d.f0 + fl;
    const size_t ri0 = (((size_t)c * d.F + f) * d.B + b) * d.P;   // the view's run in the reference's [C,F,B,P] order
    // a view without a valid slot (the camera does not see the board in this frame): zeros, no gather
    bool any = false;
    for (int q0 = 0; q0 < d.P; q0 += 64) {
      const int p = q0 + lane;
      const size_t s = (size_t)v * d.P + min(p, d.P - 1);
      any = any || __ballot(p < d.P && (t.evalid[s] | t.inlier[s]) != 0) != 0ull;
    }
    if (!any) {
      for (int p = lane; p < d.P; p += 64) {
        if (pred_cov != nullptr) pred_cov[3 * (ri0 + p)] = pred_cov[3 * (ri0 + p) + 1] = pred_cov[3 * (ri0 + p) + 2] = 0.0;
        if (student != nullptr) student[ri0 + p] = 0.0;
      }
      if (lane == 0) vpart[v] = vpart[(size_t)nv + v] = 0.0;
      continue;
    }
    // ---- per view: Sigma_view -> G ----
    bool fg = false;
    if (lane < NL) {
      const int xi = local_to_x(d, f, c, b, lane);
      int cd = -1;
      if (xi >= 0) {
        const int s = d.x_to_shared(xi);
        cd = s >= 0 ? s : -2 - (lane - 6);   // eliminated frame parameter lane - 6 of the frame (local_is_frame)
        fg = pflag[xi] != 0;
      }
      code[lane] = cd;
    }
    const unsigned long long fm = __ballot(fg);
    const int nflag = __popcll(fm);
    if (fg) flagged[__popcll(fm & ((1ull << lane) - 1ull))] = lane;
    // That of the view, lane j forming column j exactly as k_tmat does (view_that_column) -- NOT read from the That table: k_tmat
    // skips the views without inliers, and their valid slots are predicted too
    if (lane < NPC) view_that_column(d, global_pose_src(d, t), t.bwg, f, c, b, lane, Tm, NPC);
    lds_fence();
    if (gview == nullptr) {   // Sigma-route: G of the view (the whitened route reads Q of k_obscov_whiten per point instead)
    {
      double val[NE];
#pragma unroll
      for (int k = 0; k < NE; ++k) {
        const int e = min(lane + 64 * k, NL * NL - 1);
        const int i = e / NL, j = e % NL;
        const int ci = code[min(i, j)], cj = code[max(i, j)];   // (one triangle: Sv is symmetric to the bit)
        const bool ok = ci != -1 && cj != -1;
        const bool si = ci >= 0, sj = cj >= 0;
        const int fi = -2 - ci, fj = -2 - cj;
        const double* src = Sss;
        if (ok) {
          if (si && sj) src = Sss + (size_t)ci * ns + cj;
          else if (!si && !sj) src = Sff + ((size_t)fl * DF + fi) * DF + fj;
          else if (!si) src = Sfs + ((size_t)fl * DF + fi) * ns + cj;
          else src = Sfs + ((size_t)fl * DF + fj) * ns + ci;
        }
        val[k] = *src * (ok ? 1.0 : 0.0);   // (masked_load's form: the loads of a lane stay independent)
      }
#pragma unroll
      for (int k = 0; k < NE; ++k)
        if (lane + 64 * k < NL * NL) Sv[lane + 64 * k] = val[k];
    }
    lds_fence();
    for (int e = lane; e < DE * NL; e += 64) {
      const int a = e / NL, j = e % NL;
      double sum = 0.0;
#pragma unroll
      for (int l = 0; l < NPC; ++l) sum += Tm[a * NPC + l] * Sv[l * NL + j];
      M1[e] = sum;
    }
    lds_fence();
    for (int e = lane; e < NG * NG; e += 64) {
      const int a = e / NG, bb = e % NG;
      const int lo = min(a, bb), hi = max(a, bb);
      double g;
      if (hi < DE) {
        g = 0.0;
#pragma unroll
        for (int j = 0; j < NPC; ++j) g += M1[a * NL + j] * Tm[bb * NPC + j];
      } else if (lo < DE) {
        g = M1[lo * NL + NPC + (hi - DE)];
      } else {
        g = Sv[(NPC + a - DE) * NL + NPC + (bb - DE)];
      }
      G[e] = g;
    }
    }
    lds_fence();
    // ---- per point ----
    double tr_acc = 0.0, mx = 0.0;
    // The slots to predict (valid or inlier: ~30 % of a real rig's table) are ballot-compacted into a point list per segment of
    // LIN_MAX_POINTS slots, as inlier_list (mcba_kernels.h) compacts the inliers, and the forms below run on dense 64-lane chunks; the other slots
    // of the segment get their zeros on the way.
    for (int seg0 = 0; seg0 < d.P; seg0 += LIN_MAX_POINTS) {
    int count = 0;
#pragma unroll
    for (int k = 0; k < NPB64; ++k) {
      const int p = seg0 + k * 64 + lane;
      const bool ok = p < d.P;
      const size_t s = (size_t)v * d.P + (ok ? p : 0);
      const bool act = ok && (t.evalid[s] | t.inlier[s]) != 0;
      const unsigned long long m = __ballot(act);
      if (act) pidx[count + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)p;
      count += __popcll(m);
      if (ok && !act) {
        if (pred_cov != nullptr) pred_cov[3 * (ri0 + p)] = pred_cov[3 * (ri0 + p) + 1] = pred_cov[3 * (ri0 + p) + 2] = 0.0;
        if (student != nullptr) student[ri0 + p] = 0.0;
      }
    }
    lds_fence();
    for (int base = 0; base < count; base += 64) {
      const bool ok = base + lane < count;
      const int p = ok ? pidx[base + lane] : 0;
      const size_t s = (size_t)v * d.P + p;
      const bool ev = ok && t.evalid[s] != 0;
      const bool in = ok && t.inlier[s] != 0;
      double uu = 0.0, uv = 0.0, vv = 0.0, dd = 0.0;
      if (ev || in) {
        PointState<ND, ROLL> ps;
        point_state<ND, FISH, ROLL, false>(d, t, v, c, b, p, t.obs[s], ps);
        double r0[NV], r1[NV];
        point_row<ND, ROLL, OPTK>(ps, 0, r0);
        point_row<ND, ROLL, OPTK>(ps, 1, r1);
        // rows G rows^T with the a-loop ROLLED: the rows stay in registers for the inner products (static indices) and come back
        // from a per-lane LDS column for the outer index -- fully unrolled, the scheduler hoists all NG^2 LDS reads of G and
        // spills ~500 VGPRs
        if (gview != nullptr) {   // whitened: z = Q rows^T row by row of Q (wave-uniform reads), C = sigma^2 z z^T
          const int nr = DF + ns;
          const double* q = gview + (size_t)v * nr * NG;
#pragma unroll 1
          for (int i = 0; i < nr; ++i) {
            double z0 = 0.0, z1 = 0.0;
#pragma unroll
            for (int a = 0; a < NG; ++a) {
              const double qa = q[i * NG + a];
              z0 += qa * r0[a];
              z1 += qa * r1[a];
            }
            uu += z0 * z0;
            uv += z0 * z1;
            vv += z1 * z1;
          }
          uu *= sigma2;
          uv *= sigma2;
          vv *= sigma2;
        } else {
#pragma unroll
        for (int a = 0; a < NG; ++a) {
          rowbuf[a * 64 + lane] = r0[a];
          rowbuf[(NG + a) * 64 + lane] = r1[a];
        }
#pragma unroll 1
        for (int a = 0; a < NG; ++a) {
          const double ra0 = rowbuf[a * 64 + lane], ra1 = rowbuf[(NG + a) * 64 + lane];
          double s0 = 0.0, s1 = 0.0;
#pragma unroll
          for (int bb = 0; bb < NG; ++bb) {
            const double g = G[a * NG + bb];
            s0 += g * r0[bb];
            s1 += g * r1[bb];
          }
          uu += ra0 * s0;
          uv += ra1 * s0;
          vv += ra1 * s1;
        }
        }
        bool undetermined = false;   // the row pair touches an unobserved parameter that is not held
        for (int q = 0; q < nflag; ++q) {
          const int l = flagged[q];
          double j0 = 0.0, j1 = 0.0;
          if (l < NPC) {
#pragma unroll
            for (int e = 0; e < DE; ++e) {
              const double tm = Tm[e * NPC + l];
              j0 += r0[e] * tm;
              j1 += r1[e] * tm;
            }
          } else {
#pragma unroll
            for (int kk = 0; kk < KI; ++kk)
              if (l - NPC == kk) {
                j0 = r0[DE + kk];
                j1 = r1[DE + kk];
              }
          }
          undetermined = undetermined || j0 != 0.0 || j1 != 0.0;
        }
        if (undetermined) {
          uu = uv = vv = dd = nan;
        } else {
          const double lam = sym2_max_eig(uu, uv, vv);
          const double sg = in ? -1.0 : 1.0;   // Omega = sigma^2 I - C (residual of an inlier) / sigma^2 I + C (prediction error)
          const double oa = sigma2 + sg * uu, ob = sg * uv, oc = sigma2 + sg * vv;
          const double rx = r0[NV - 1], ry = r1[NV - 1];
          const double d2 = (oc * rx * rx - 2.0 * ob * rx * ry + oa * ry * ry) / (oa * oc - ob * ob);
          dd = sqrt(fmax(d2, 0.0));
          if (in && lam >= (1.0 - OBSCOV_EXACT_FIT) * sigma2) dd = inf;
          if (in) tr_acc += (uu + vv) / sigma2;
          if (ev) mx = fmax(mx, sqrt(fmax(lam, 0.0)));
        }
        if (!ev) uu = uv = vv = dd = 0.0;   // (an inlier outside the valid mask counts in the trace only)
      }
      if (ok) {
        const size_t ri = ri0 + p;
        if (pred_cov != nullptr) {
          pred_cov[3 * ri] = uu;
          pred_cov[3 * ri + 1] = uv;
          pred_cov[3 * ri + 2] = vv;
        }
        if (student != nullptr) student[ri] = dd;
      }
    }
    lds_fence();   // the next segment rewrites the list
    }
    const double ts = wave_sum(tr_acc), ms = wave_max(mx);
    if (lane == 0) {
      vpart[v] = ts;
      vpart[(size_t)nv + v] = ms;
    }
    lds_fence();   // the next view rewrites the tables
  }
}

// ---------------------------------------------------------------------------------------------------------------
// k_obscov_whiten: the WHITENED route.  C_p = sigma^2 z z^T with z = M^-1 D J_p^T is a sum of squares: none of
// the cancellation of J_p Sigma J_p^T (1e4 .. 1e7), which the studentised error of a near-unit-leverage inlier (1 - h) cannot
// afford.  With the block Cholesky factor of the scaled system A = D H D the covariance chain leaves on the device,
//     A = M M^T,  M = [L_f 0; W_f^T L]      (L_f, W_f = L_f^-1 A_fs of the view's frame;  L L^T = S, X = L^-1)
//     Q_f = L_f^-1 B_f,   Q_s = X (B_s - W_f^T Q_f),   z_p = [Q_f; Q_s] [E_p | K_p]^T      (Q: (DF + ns) x NG per VIEW)
// where B (n x NG) holds D_l That_e[:, l]^T in the row of every local parameter l of the view (frame rows B_f, shared rows B_s).
// (Forming G = Q^T Q first and then the quadratic form rows G rows^T brings the cancellation back at the point level.)
// One workgroup per view; Y = B_s - W_f^T Q_f (ns x NG) lives in dynamic LDS and becomes Q_s IN PLACE: X is lower triangular,
// so row i needs Y[k <= i] only and the rows are replaced bottom-up, THREADS / NG at a time.  (ns^2 NG flops per view.)
// Lf: [Fl][DF][DF] strict lower triangle + 1 / L_ii on the diagonal, W: [Fl][DF][ns + 1], X: [ns][ns] (k_schur_frame, k_cov_trinv).
// ---------------------------------------------------------------------------------------------------------------
__host__ __device__ inline size_t obscov_whiten_lds_bytes(const Dims& d) {
  const int NG = d.DE + d.KI;
  return ((size_t)d.ns * NG + (size_t)d.DE * 6 * d.NPB + 2 * (size_t)(d.DF > 0 ? d.DF : 1) * NG + d.NL) * sizeof(double) +
         (size_t)d.NL * sizeof(int) + 16;
}
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_obscov_whiten(Dims d, Tables t, const double* __restrict__ dcov,
                                                           const double* __restrict__ Lf, const double* __restrict__ W,
                                                           const double* __restrict__ X, double* __restrict__ qview) {
  extern __shared__ __attribute__((aligned(16))) double ocw[];
  const int DE = d.DE, NPC = 6 * d.NPB, NL = d.NL, NG = DE + d.KI, ns = d.ns, DF = d.DF, DFs = DF > 0 ? DF : 1;
  double* Y = ocw;                                   // [ns][NG]
  double* Tm = Y + (size_t)ns * NG;                  // [DE][NPC]
  double* Bf = Tm + DE * NPC;                        // [DF][NG]
  double* Qf = Bf + DFs * NG;                        // [DF][NG]
  double* dl = Qf + DFs * NG;                        // [NL] D of the local parameters (0: none / held / unobserved)
  int* code = reinterpret_cast<int*>(dl + NL);       // [NL] shared index, -2 - frame index, -1 none
  const int tid = threadIdx.x, v = blockIdx.x;
  const int b = v % d.B, c = (v / d.B) % d.C, fl = v / (d.B * d.C), f = d.f0 + fl;
  int any = 0;
  for (int p = tid; p < d.P; p += THREADS) any |= t.evalid[(size_t)v * d.P + p] | t.inlier[(size_t)v * d.P + p];
  if (!__syncthreads_or(any)) return;                // (k_obscov does not read Q of such a view)
  if (tid < NL) {
    const int xi = local_to_x(d, f, c, b, tid);
    int cd = -1;
    double dv = 0.0;
    if (xi >= 0) {
      const int s = d.x_to_shared(xi);
      cd = s >= 0 ? s : -2 - (tid - 6);
      dv = dcov[xi];
    }
    code[tid] = cd;
    dl[tid] = dv;
  }
  if (tid < NPC) view_that_column(d, global_pose_src(d, t), t.bwg, f, c, b, tid, Tm, NPC);
  for (int e = tid; e < ns * NG; e += THREADS) Y[e] = 0.0;
  for (int e = tid; e < DFs * NG; e += THREADS) Bf[e] = Qf[e] = 0.0;
  __syncthreads();
  for (int e = tid; e < NL * NG; e += THREADS) {     // B: row of local parameter l = D_l That_e[:, l]^T
    const int l = e / NG, a = e % NG;
    const double te = l < NPC ? (a < DE ? Tm[a * NPC + l] : 0.0) : (a == DE + l - NPC ? 1.0 : 0.0);
    const int cd = code[l];
    if (cd >= 0) Y[(size_t)cd * NG + a] = dl[l] * te;
    else if (cd <= -2) Bf[(-2 - cd) * NG + a] = dl[l] * te;
  }
  __syncthreads();
  if (DF > 0) {
    if (tid < NG) {                                  // Q_f = L_f^-1 B_f, column tid by forward substitution
      const double* L = Lf + (size_t)fl * DF * DF;
      for (int i = 0; i < DF; ++i) {
        double acc = Bf[i * NG + tid];
        for (int m = 0; m < i; ++m) acc -= L[i * DF + m] * Qf[m * NG + tid];
        Qf[i * NG + tid] = acc * L[i * DF + i];
      }
    }
    __syncthreads();
    const double* w = W + (size_t)fl * DF * (ns + 1);
    for (int e = tid; e < ns * NG; e += THREADS) {   // Y = B_s - W_f^T Q_f
      const int s = e / NG, a = e % NG;
      double acc = Y[e];
      for (int i = 0; i < DF; ++i) acc -= w[(size_t)i * (ns + 1) + s] * Qf[i * NG + a];
      Y[e] = acc;
    }
    __syncthreads();
  }
  const int RB = THREADS / NG, r = tid / NG, a = tid % NG;   // Q_s = X Y in place, RB rows at a time from the bottom
  for (int hi = ns; hi > 0; hi -= RB) {
    const int i = hi - 1 - r;
    const bool on = r < RB && i >= 0;
    double acc = 0.0;
    if (on) {
      const double* xr = X + (size_t)i * ns;
      for (int k = 0; k <= i; ++k) acc += xr[k] * Y[(size_t)k * NG + a];
    }
    __syncthreads();
    if (on) Y[(size_t)i * NG + a] = acc;
    __syncthreads();
  }
  double* q = qview + (size_t)v * (DF + ns) * NG;     // Q = [Q_f; Q_s], (DF + ns) x NG
  for (int e = tid; e < DF * NG; e += THREADS) q[e] = Qf[e];
  for (int e = tid; e < ns * NG; e += THREADS) q[(size_t)DF * NG + e] = Y[e];
}

// out[0] = sum of vpart[0 .. views) (the trace), out[1 + c] = max over the views of camera c of vpart[views + v].  One workgroup per
// output, every thread folding a fixed strided subsequence (eight independent loads in flight), then block_reduce: one order,
// the same bits on every call.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_obscov_fold(Dims d, const double* __restrict__ vpart, double* __restrict__ out) {
  __shared__ double scratch[16];
  constexpr int UB = 8;
  const int nv = d.views(), tid = threadIdx.x;
  if (blockIdx.x == 0) {
    double s = 0.0;
    for (int i0 = tid; i0 < nv; i0 += THREADS * UB) {
      double x[UB];
#pragma unroll
      for (int k = 0; k < UB; ++k) x[k] = vpart[min(i0 + THREADS * k, nv - 1)];
#pragma unroll
      for (int k = 0; k < UB; ++k)
        if (i0 + THREADS * k < nv) s += x[k];
    }
    s = block_reduce<false>(s, scratch);
    if (tid == 0) out[0] = s;
  } else {
    const int c = blockIdx.x - 1, n = d.Fl * d.B;   // view (fl, c, b) = (fl C + c) B + b
    double m = 0.0;
    for (int i0 = tid; i0 < n; i0 += THREADS * UB) {
      double x[UB];
#pragma unroll
      for (int k = 0; k < UB; ++k) {
        const int i = min(i0 + THREADS * k, n - 1);
        x[k] = vpart[(size_t)nv + ((size_t)(i / d.B) * d.C + c) * d.B + i % d.B];
      }
#pragma unroll
      for (int k = 0; k < UB; ++k)
        if (i0 + THREADS * k < n) m = fmax(m, x[k]);
    }
    m = block_reduce<true>(m, scratch);
    if (tid == 0) out[1 + c] = m;
  }
}

}  // namespace mcba
