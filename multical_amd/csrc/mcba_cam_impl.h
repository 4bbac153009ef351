// mcba_cam_impl.h -- body of one camera-model translation unit: define MCBA_ND, MCBA_FISH, MCBA_CAM_FN, include.
#include <algorithm>
#include "mcba_kernels.h"
#include "mcba_obscov_kernels.h"
#include "mcba_camops.h"
#include "mcba_dispatch.h"

namespace mcba {
namespace {

constexpr int ND_ = MCBA_ND;
constexpr int FISH_ = MCBA_FISH;   // 0 pinhole, 1 fisheye, 2 per camera (mixed rig)

inline int slot_grid(const Dims& d) {
  const int n = d.slots();
  int g = (n + 255) / 256;
  return g < 1 ? 1 : (g > 4096 ? 4096 : g);
}

// motion model and "intrinsics optimised" of the rig as template arguments: f(int_c<MOTION>, bool_constant<OPTK>)
template <class F>
void with_view_shape(const Dims& d, F&& f) {
  with_motion(d.motion, [&](auto mo) { with_flag(d.KI > 0, [&](auto ok) { f(mo, ok); }); });
}

void residual(const Dims& d, const Tables& t, hipStream_t s, const int32_t* first, double* r, double* proj, double* err,
              uint8_t* valid) {
  if (d.views() == 0) return;
  const dim3 grid(std::min(8192, (d.views() + 3) / 4)), block(256);   // one wavefront per view, four views per block
  with_flag(d.motion == MOTION_ROLLING, [&](auto roll) {
    hipLaunchKernelGGL((k_residual<ND_, FISH_, roll>), grid, block, 0, s, d, t, first, r, proj, err, valid);
  });
}

void project_model(const Dims& d, const Tables& t, hipStream_t s, int iterations, double* proj) {
  with_flag(d.motion == MOTION_ROLLING, [&](auto roll) {
    hipLaunchKernelGGL((k_project_model<ND_, FISH_, roll>), dim3(slot_grid(d)), dim3(256), 0, s, d, t, iterations, proj);
  });
}

void cost(const Dims& d, const Tables& t, hipStream_t s, double* partial, int nblk) {
  with_flag(d.motion == MOTION_ROLLING, [&](auto roll) { with_flag(d.loss != 0, [&](auto rob) {
    hipLaunchKernelGGL((k_cost<ND_, FISH_, roll, rob>), dim3(nblk), dim3(64), 0, s, d, t, partial);
  }); });
}

void jacobian(const Dims& d, const Tables& t, hipStream_t s, int row_nnz, double* vals, int32_t* cols) {
  with_flag(d.motion == MOTION_ROLLING, [&](auto roll) {
    hipLaunchKernelGGL((k_jacobian<ND_, FISH_, roll>), dim3(slot_grid(d)), dim3(128), 0, s, d, t, row_nnz, vals, cols);
  });
}

void linearize(const Dims& d, const Tables& t, hipStream_t s, double* rec, const uint16_t* tri, bool mfma, int epoch,
               const double* x, double* za, int na, double* zb, int nb, const LsmrCompact* cpp) {
  // table-fed fused form: za != nullptr (pose entries / intrinsics from the pose and camera tables; zeroes the assembly
  // targets za[na], zb[nb]); za == nullptr: table form (That / chains per view from k_tmat)
  const bool fused = za != nullptr;
  // cpp != nullptr (fused form only): the compacted observation tables of the current inlier set (form 3)
  const LsmrCompact cp = cpp != nullptr ? *cpp : LsmrCompact{nullptr, nullptr, nullptr, nullptr, nullptr};
  if (d.views() == 0 && !fused) return;   // empty frame shard (the fused form still zeroes the assembly targets)
  // persistent wavefronts: 8 single-wave workgroups per CU (2 per SIMD: 256-VGPR budget, 20 KB LDS each) x 256 CUs
  // (rigs with tens of thousands of views: four times as many workgroups for the dispatcher to hand out -- 16 x 1000 x 5, 80 000 views,
  //  4 waves per SIMD: 4096 -> 57.8 us, 8192 -> 54.5, 16384 -> 53.5; 8 x 500 x 2 stays at 4096: 41.6 against 42.3 us -- profiles/r06_lin_compact.txt)
  const int want = epoch > 0 ? epoch : (d.views() >= 32768 ? 4 * LIN_GRID_MAX : LIN_GRID_MAX);   // the last argument carries the debug grid override
  const dim3 grid(std::max(1, d.views() < want ? d.views() : want)), block(64);
  const int form = !fused ? 0 : (cpp != nullptr ? 3 : 2);   // k_linearize's FUSED_MODE
  with_view_shape(d, [&](auto mo, auto ok) {
    auto launch = [&](auto mf, auto rob, auto fm, auto prof) {
      hipLaunchKernelGGL((k_linearize<ND_, FISH_, mo, ok, mf, rob, fm, prof>), grid, block, 0, s, d, t, rec, tri,
                         epoch, x, za, na, zb, nb, cp);
    };
    // NOT a cross product: the per-phase cycle stamps (debug API, t.dbg) and the plain-FMA validation build exist in the table
    // form with the generic loss only.  The linear loss (the reference's default, calibration.py:199) has its own instantiation
    // of the MFMA kernel: no loss switch and no robust-scale constants in the hot loop.
    if (t.dbg != nullptr) launch(std::true_type{}, std::true_type{}, int_c<0>{}, std::true_type{});
    else if (!mfma) launch(std::false_type{}, std::true_type{}, int_c<0>{}, std::false_type{});
    else with_flag(d.loss != 0, [&](auto rob) { with_int<3, 2, 0>(form, [&](auto fm) {
      launch(std::true_type{}, rob, fm, std::false_type{});
    }); });
  });
}

void points(const Dims& d, const Tables& t, hipStream_t s, int nq, double* Hss, double* Hfs, double* g) {
  if (nq <= 0) return;
  with_view_shape(d, [&](auto mo, auto ok) {
    hipLaunchKernelGGL((k_points<ND_, FISH_, mo, ok>), dim3(nq), dim3(256), 0, s, d, t, Hss, Hfs, g);
  });
}

void lsmr_jv(const Dims& d, const Tables& t, hipStream_t s, const int32_t* first, int mode, const double* dscale, const double* v,
             double alpha, double* u, double* partial, int nblk, const double* ls) {
  with_view_shape(d, [&](auto mo, auto ok) { with_flag(d.loss != 0, [&](auto rob) {
    hipLaunchKernelGGL((k_lsmr_jv<ND_, FISH_, mo, ok, rob>), dim3(nblk), dim3(64), 0, s, d, t, first, mode, dscale, v, alpha, u,
                       partial, ls);
  }); });
}

void lsmr_jtu(const Dims& d, const Tables& t, hipStream_t s, const int32_t* first, double inv_beta, double* u, double* part,
              int part_stride, double* bpart, int nblk, const double* ls) {
  with_view_shape(d, [&](auto mo, auto ok) { with_flag(d.loss != 0, [&](auto rob) {
    hipLaunchKernelGGL((k_lsmr_jtu<ND_, FISH_, mo, ok, rob>), dim3(nblk), dim3(64), 0, s, d, t, first, inv_beta, u, part,
                       part_stride, bpart, ls);
  }); });
}

void lsmr_fused(const Dims& d, const Tables& t, hipStream_t s, const int32_t* first, const double* dscale, const double* v, double* u,
                double* partial, double* part, int part_stride, double* bpart, int nblk, const double* ls) {
  with_view_shape(d, [&](auto mo, auto ok) { with_flag(d.loss != 0, [&](auto rob) {
    hipLaunchKernelGGL((k_lsmr_fused<ND_, FISH_, mo, ok, rob>), dim3(nblk), dim3(64), 0, s, d, t, first, dscale, v, u, partial,
                       part, part_stride, bpart, ls);
  }); });
}

// mode (k_lsmr_fused2's MODE): 0 = masks (boards=True), 3 = compact tables (default), 4 = compact + store the per-observation state,
// 2 = stream the state back
void lsmr_fused2(const Dims& d, const Tables& t, hipStream_t s, const int32_t* first, const double* dscale, const double* v, double* u,
                 double* partial, double* xpart, double* part, int part_stride, double* bpart, int nblk, const double* lsIn,
                 double* lsOut, const double* vpart, int nv, double* hbar, double* x, double* h, double* cache, int mode, LsmrCompact cp) {
  with_view_shape(d, [&](auto mo, auto ok) { with_flag(d.loss != 0, [&](auto rob) { with_int<2, 3, 4, 0>(mode, [&](auto md) {
    hipLaunchKernelGGL((k_lsmr_fused2<ND_, FISH_, mo, ok, rob, md>), dim3(nblk), dim3(64), 0, s, d, t, first, dscale, v, u,
                       partial, xpart, part, part_stride, bpart, lsIn, lsOut, vpart, nv, hbar, x, h, cache, cp);
  }); }); });
}

void obs_cov(const Dims& d, const Tables& t, hipStream_t s, const double* Sss, const double* Sff, const double* Sfs, const uint8_t* pflag,
             double sigma2, double* pred_cov, double* student, double* vpart, double* out, const double* gview) {
  if (d.views() == 0) return;
  const int nblk = std::min(d.views(), 16384);   // single-wave workgroups, views dealt round-robin
  with_view_shape(d, [&](auto mo, auto ok) {
    hipLaunchKernelGGL((k_obscov<ND_, FISH_, mo, ok>), dim3(nblk), dim3(64), 0, s, d, t, Sss, Sff, Sfs, pflag, sigma2, pred_cov,
                       student, vpart, gview);
  });
  hipLaunchKernelGGL((k_obscov_fold<1024>), dim3(1 + d.C), dim3(1024), 0, s, d, (const double*)vpart, out);
}

const CamOps OPS = {residual, project_model, cost, jacobian, linearize, points, lsmr_jv, lsmr_jtu, lsmr_fused, lsmr_fused2, obs_cov};

}  // namespace

const CamOps* MCBA_CAM_FN() { return &OPS; }

}  // namespace mcba
