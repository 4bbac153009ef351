/* mcba.h -- C ABI of the MI355X bundle-adjustment back-end ("multical bundle adjust").
 *
 * Drop-in boundary for ONE path of oliver-batchelor/multical: the reprojection residual / Jacobian evaluation and
 * the damped normal-equation solve behind
 *     multical.optimization.Calibration.bundle_adjust      (multical/optimization/calibration.py:199-212)
 *     multical.workspace.Workspace.calibrate               (multical/workspace.py:228-247)
 * The reference has no FFI of its own (it is pure Python on top of scipy / OpenCV); this header is the interface a
 * ctypes stub inside `Calibration.bundle_adjust` binds.  Every entry point names the reference
 * function it replaces.
 *
 * Conventions
 *   - plain C: pointers + sizes, no C++/torch types; every function returns 0 on success, non-zero on error and
 *     never throws across the ABI; `mcba_last_error()` returns a thread-local message.
 *   - all floating point is IEEE double; masks are uint8 (0/1); arrays are C-contiguous.
 *   - host buffers are caller-owned and only read during the call; the handle owns device memory and runs every
 *     kernel on the HIP stream given at creation (NULL = the handle creates its own stream).
 *   - one handle per thread; handles are independent.
 *   - the library is HIP-only: `mcba_create` fails when no gfx950 device is present.  There is no CPU fallback.
 *   - limits of this implementation (the reference has none; all are checked by `mcba_create`, which fails with a
 *     message instead of producing a handle that cannot be solved):
 *     at most 65535 points per board; about 36 000 (camera, board) pairs when per-frame rig poses are optimised (their
 *     view-rank tables live in the 150 KB of LDS of a workgroup).  Cameras of one rig may carry different numbers of
 *     distortion coefficients (4, 5, 8, 12, 14: mcba_problem.camera_n_dist) and may mix pinhole and fisheye cameras
 *     (mcba_problem.camera_fisheye).
 *
 * Parameter vector `x` (length `n_params`): exactly `Calibration.param_vec` (optimization/parameters.py:44-46):
 * the ENABLED blocks, in the order camera_poses | board_poses | motion | cameras | boards
 * (optimization/calibration.py:146-161):
 *     camera_poses : C x (rx ry rz tx ty tz)                           pose_set.py:51-53
 *     board_poses  : B x 6
 *     motion       : static   F x 6                                    motion/static_frames.py:29
 *                    rolling  F x 6 (start) then F x 6 (end)           motion/rolling_frames.py:135-140
 *                    hand-eye 6 (world_wrt_base) 6 (gripper_wrt_camera) motion/hand_eye.py:75-80
 *     cameras      : C x [fx fy | cx cy | skew | dist(n_dist)]         camera.py:144-155
 *     boards       : sum_b P_b x 3                                     board/charuco.py:112-114
 * Disabled blocks keep the values given in `mcba_problem.x_full`.
 *
 * Residual vector `r` (length `n_residuals` = 2 * #inliers): C-order over (camera, frame, board, point) restricted
 * to the inlier mask, (u,v) interleaved -- `(reprojected.points - point_table.points)[inliers].ravel()`
 * (optimization/calibration.py:204-206).
 */
#ifndef MCBA_H
#define MCBA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCBA_VERSION 3

/* motion models (multical/motion/) */
#define MCBA_MOTION_STATIC   0   /* motion/static_frames.py  */
#define MCBA_MOTION_ROLLING  1   /* motion/rolling_frames.py (linear, scan time from the observed row) */
#define MCBA_MOTION_HAND_EYE 2   /* motion/hand_eye.py       */

/* camera models */
#define MCBA_CAMERA_PINHOLE 0    /* camera.py:124-128         -> cv2.projectPoints, n_dist in {5,8,12,14} */
#define MCBA_CAMERA_FISHEYE 1    /* camera_fisheye.py:113-117 -> cv2.fisheye.projectPoints, n_dist = 4     */

/* trust-region step of the solver (scipy `tr_solver`) */
#define MCBA_TR_EXACT 0          /* regularised Gauss-Newton step from the exact normal equations (Schur + Cholesky): fast,     */
                                 /* ends at the converged optimum                                                              */
#define MCBA_TR_LSMR  1          /* scipy's choice for the reference's sparse Jacobian: LSMR with atol = btol = 1e-6 -- the     */
                                 /* reference's trajectory and end point                                                       */

/* robust losses (scipy.optimize.least_squares `loss`, reachable through OptimizerOpts.loss, config/arguments.py:61) */
#define MCBA_LOSS_LINEAR  0
#define MCBA_LOSS_SOFT_L1 1
#define MCBA_LOSS_HUBER   2
#define MCBA_LOSS_CAUCHY  3
#define MCBA_LOSS_ARCTAN  4

/* parameter blocks, bit flags for mcba_problem.optimize (calibration.py:28-35 `default_optimize`) */
#define MCBA_OPT_CAMERA_POSES 1
#define MCBA_OPT_BOARD_POSES  2
#define MCBA_OPT_MOTION       4
#define MCBA_OPT_CAMERAS      8
#define MCBA_OPT_BOARDS       16

typedef struct mcba_problem {
  int32_t version;              /* MCBA_VERSION */
  int32_t n_cameras;            /* C */
  int32_t n_frames;             /* F */
  int32_t n_boards;             /* B */
  int32_t n_points;             /* P = max points per board (tables.stack_boards, tables.py:385-394) */

  const double*  points;        /* [C,F,B,P,2] point_table.points as float64, or NULL when points_f32   */
                                /* (last member) carries the table                                     */
  const uint8_t* point_valid;   /* [C,F,B,P]   point_table.valid                                       */
  const uint8_t* inlier_mask;   /* [C,F,B,P]   Calibration.inlier_mask, or NULL -> inliers = valid     */

  const int32_t* board_sizes;   /* [B]   P_b (number of real points of each board)                     */
  const uint8_t* camera_valid;  /* [C]   camera_poses.valid                                            */
  const uint8_t* frame_valid;   /* [F]   motion.valid                                                  */
  const uint8_t* board_valid;   /* [B]   board_poses.valid                                             */

  int32_t motion;               /* MCBA_MOTION_*                                                       */
  int32_t camera_model;         /* MCBA_CAMERA_*                                                       */
  int32_t n_dist;               /* distortion coefficients per camera (camera.dist.size)               */
  const double*  image_heights;    /* [C] camera.image_size[1]  (rolling_frames.py:15-19)              */
  const uint8_t* fix_aspect;       /* [C] Camera.fix_aspect (camera.py:147-148,159-160)                */
  const double*  base_wrt_gripper; /* [F,4,4] hand-eye only (motion/hand_eye.py:43-46), else NULL      */

  uint32_t optimize;            /* OR of MCBA_OPT_*                                                    */
  const double* x_full;         /* all five blocks in reference order, length mcba_full_size();        */
                                /* values of disabled blocks are taken from here                        */
  int32_t frame_begin;          /* frame shard owned by this handle: [frame_begin, frame_end) (may be empty);     */
  int32_t frame_end;            /* frame_begin < 0 = all frames.  Arrays above always describe ALL frames.       */
  const int32_t* camera_n_dist; /* [C] distortion coefficients of EACH camera (camera.dist.size), or NULL: every   */
                                /* camera carries n_dist.  The reference's ParamList holds independent Camera      */
                                /* objects (optimization/parameters.py:54-85, camera.py:144-155), so the cameras   */
                                /* block of x / x_full is ragged: camera c contributes 5 + camera_n_dist[c]        */
                                /* entries.  n_dist must then be the maximum; pinhole sizes (4, 5, 8, 12, 14) mix  */
                                /* freely (a smaller model is the larger one with its extra coefficients at zero). */
  const uint8_t* camera_fisheye;/* [C] 1 = CameraFisheye (camera_fisheye.py:28), 0 = Camera, or NULL: every camera is of  */
                                /* `camera_model`.  A rig may MIX the two families (the reference holds independent     */
                                /* objects, parameters.py:54-85); camera_n_dist is then required unless all carry 4.    */
  const float* points_f32;      /* [C,F,B,P,2] point_table.points as float32 -- the dtype the reference's table has in  */
                                /* use: fill_sparse keeps `values.dtype` (tables.py:15-17) and cv2 detects float32      */
                                /* corners.  Uploaded as it is (half the bytes) and widened on the device, exactly as   */
                                /* numpy promotes it in `reprojected.points - point_table.points`.  Exactly one of      */
                                /* points / points_f32 is non-NULL.                                                     */
} mcba_problem;

typedef struct mcba_options {          /* scipy.optimize.least_squares arguments used at calibration.py:209-210 */
  double ftol;                  /* `tolerance`      (default 1e-4, calibration.py:199)                  */
  double xtol;                  /* scipy default 1e-8                                                   */
  double gtol;                  /* scipy default 1e-8                                                   */
  int32_t max_nfev;             /* `max_iterations` (default 100)                                       */
  int32_t loss;                 /* MCBA_LOSS_*                                                          */
  double f_scale;               /* scipy `f_scale` (soft margin of the robust loss)                     */
  int32_t verbose;              /* 2: per-iteration rows are delivered to the log callback              */
  int32_t tr_solver;            /* MCBA_TR_EXACT (0): exact Schur / Cholesky steps; MCBA_TR_LSMR (1): scipy's own step,     */
                                /* gn_h = lsmr(J_h, f, damp) (trf.py:481), with the Jacobian products on the device.        */
                                /* (Until round 3 this field was `reserved`: ZERO-INITIALISE the struct -- an uninitialised */
                                /* value is rejected with "unknown trust-region solver".  MCBA_TR_LSMR is what reproduces   */
                                /* the reference's end point; the Python drop-in selects it by default.)                     */
} mcba_options;

typedef struct mcba_result {           /* scipy OptimizeResult fields the caller needs                    */
  double cost;                  /* 0.5 * sum(rho(f^2))                                                  */
  double initial_cost;
  double optimality;            /* |g|_inf                                                              */
  int32_t nfev;                 /* residual evaluations (trial steps + 1)                               */
  int32_t njev;                 /* linearisations (fused residual + Jacobian -> normal equations)       */
  int32_t status;               /* scipy status: 0 max_nfev, 1 gtol, 2 ftol, 3 xtol, 4 ftol+xtol         */
  int32_t iterations;
  double solve_seconds;         /* wall time inside mcba_solve                                          */
  double linearize_seconds;     /* GPU time (HIP events) spent in the fused linearisation kernels       */
} mcba_result;

typedef struct mcba_round_report {     /* one pass of Calibration.adjust_outliers (calibration.py:254-268)             */
  double rms_all, rms_inliers;  /* report(): RMS over all valid points / over the inliers                           */
  int64_t n_all, n_inliers;
  double quantiles[5];          /* numpy.quantile(errors over all valid points, [0, .25, .5, .75, 1])               */
  double f_scale;               /* f_scale of this round's solve (auto_scale: quantile x factor)                    */
  double threshold;             /* rejection threshold of this round (quantile x factor), -1 = none                 */
  int64_t n_kept, n_valid;      /* reject_outliers: inliers kept / valid points                                      */
  mcba_result solve;            /* bundle_adjust of this round                                                       */
} mcba_round_report;

typedef struct mcba_handle_s* mcba_handle;

/* iteration log: same columns as scipy's verbose=2 table (print_iteration_nonlinear), which the reference pipes
 * into its logger (calibration.py:208, io/logging.py:53-68).  cost_reduction / step_norm are NaN on row 0.      */
typedef void (*mcba_log_fn)(void* ctx, int32_t iteration, int32_t nfev, double cost, double cost_reduction,
                            double step_norm, double optimality);

/* cross-rank reduction hook for frame-sharded problems: called from inside mcba_solve /
 * mcba_normal_equations with a DEVICE buffer of `count` doubles that must be reduced IN PLACE over all ranks,
 * ordered on `stream`.  op: 0 = sum, 1 = max.  The Python side implements it with torch.distributed
 * (backend "nccl" = RCCL over xGMI on the GPU box, "gloo" in CPU-side tests).  Return 0 on success.            */
typedef int32_t (*mcba_allreduce_fn)(void* ctx, void* device_buf, size_t count, int32_t op, void* stream);

/* --- sizes ------------------------------------------------------------------------------------------------- */
/* length of mcba_problem.x_full for the given shape (all five blocks)                                          */
int32_t mcba_full_size(const mcba_problem* p, int64_t* out);

/* --- lifetime ---------------------------------------------------------------------------------------------- */
/* Lowers a Calibration (flat arrays) to device tables: frame-major observation table, inlier prefix sums, index
 * maps.  Replaces the per-call object graph of Calibration.with_param_vec (calibration.py:164-171) and the
 * sparsity build (calibration.py:173-196).  `hip_stream` may be NULL.                                          */
int32_t mcba_create(const mcba_problem* p, void* hip_stream, mcba_handle* out);
int32_t mcba_destroy(mcba_handle h);
/* mcba_destroy parks the handle's device buffers, pinned buffers and stream in a process-wide cache (bounded: 4 GB of device
 * memory) so that the next mcba_create of a problem of the same shape does not pay for ~50 allocations again
 * (Workspace.calibrate creates one handle per call).  This returns everything in the cache to the HIP runtime.         */
int32_t mcba_release_cached_memory(void);
const char* mcba_last_error(void);
/* "gfx950:<device name>" of the device the handle lives on                                                    */
int32_t mcba_device_info(mcba_handle h, char* buf, size_t buf_len);

int32_t mcba_num_params(mcba_handle h, int64_t* n_params);
int32_t mcba_num_residuals(mcba_handle h, int64_t* n_residuals);   /* 2 * #inliers (all frames of the shard)   */

/* Replace the inlier mask (Calibration.reject_outliers -> copy(inlier_mask=...), calibration.py:240-252).
 * mask = NULL restores inliers = valid.                                                                       */
int32_t mcba_set_inliers(mcba_handle h, const uint8_t* mask);

int32_t mcba_set_allreduce(mcba_handle h, mcba_allreduce_fn fn, void* ctx);
/* Native alternative to the callback: RCCL over xGMI driven from inside the library (librccl is loaded at run time).
 * One rank calls mcba_rccl_unique_id and hands the 128 bytes to all ranks (multical_amd.distributed broadcasts them with
 * torch.distributed); then EVERY rank calls mcba_rccl_init (collective).  From then on all reductions of the handle are
 * in-place ncclAllReduce calls on the handle's stream.  mcba_rccl_shutdown leaves the native path again.            */
int32_t mcba_rccl_unique_id(uint8_t* id_out /*[128]*/);
int32_t mcba_rccl_init(mcba_handle h, const uint8_t* id /*[128]*/, int32_t rank, int32_t world);
int32_t mcba_rccl_shutdown(mcba_handle h);
/* version of the librccl the native path binds (ncclGetVersion: major * 10000 + minor * 100 + patch; 0 = library not found or
 * its ABI refused) -- reported per rank by bench.py                                                                     */
int32_t mcba_rccl_version(int32_t* version_out);
/* exactly one rank of a sharded problem is the root: it contributes the replicated (shared) right-hand side to the
 * reduced system.  Default: root.  Ranks other than 0 call this with 0.                                          */
int32_t mcba_set_shard_root(mcba_handle h, int32_t is_root);
/* rank of this handle among the `world` (<= 64) handles of one frame-sharded problem; rank 0 is the root.  Needed with a
 * callback (mcba_set_allreduce); mcba_rccl_init sets it itself.  The messages of a sharded handle are per-rank partial sums
 * gathered by summation (block `rank` of a zeroed buffer) and the SHARED entries of [g | diag]: none grows with the number
 * of frames (mcba_allreduce_stats).                                                                                  */
int32_t mcba_set_shard_rank(mcba_handle h, int32_t rank, int32_t world);
int32_t mcba_set_log(mcba_handle h, mcba_log_fn fn, void* ctx);

/* Calibration.adjust_outliers (calibration.py:254-268; what Workspace.calibrate drives, workspace.py:238-244) in ONE call:
 * `num_adjustments` rounds of {report, optional f_scale = quantile(errors, scale_quantile) * scale_factor, reject_outliers at
 * quantile(errors, outlier_quantile) * outlier_factor, bundle_adjust}, then the final report.  rounds[num_adjustments + 1];
 * a negative factor disables that step; inliers_out (may be NULL) receives the final mask [C,F,B,P]
 * (complete on every rank of a frame-sharded problem: mcba_gather_inliers).                                       */
int32_t mcba_adjust_outliers(mcba_handle h, double* x_inout, const mcba_options* opt, int32_t num_adjustments,
                             double outlier_quantile, double outlier_factor, double scale_quantile, double scale_factor,
                             mcba_round_report* rounds, uint8_t* inliers_out);

/* --- evaluation -------------------------------------------------------------------------------------------- */
/* r = evaluate(x)                                                   (calibration.py:204-206)                   */
int32_t mcba_residuals(mcba_handle h, const double* x, double* r);

/* Analytic Jacobian of `evaluate` in the sparsity pattern of Calibration.sparsity_matrix (calibration.py:173-196):
 * row pair i (one inlier observation) has `row_nnz` structurally non-zero columns (same count for every row);
 * cols[i*row_nnz + k] are ascending column indices into x, vals[(2i+a)*row_nnz + k] the entries of row 2i+a.
 * Call with vals = cols = NULL to query row_nnz.                                                               */
int32_t mcba_jacobian(mcba_handle h, const double* x, int32_t* row_nnz, double* vals, int32_t* cols);

/* Reprojection error per table slot: err[c,f,b,p] = |proj - obs|_2, valid = proj.valid & obs.valid, err = 0 where
 * invalid (tables.reprojection_error, tables.py:244-249; feeds Calibration.reprojection_error / reject_outliers /
 * report, calibration.py:134-141,240-252,290-310).  Arrays are in the reference's [C,F,B,P] order.             */
int32_t mcba_reprojection_error(mcba_handle h, const double* x, double* err, uint8_t* valid);

/* Errors reduced ON THE DEVICE (no [C,F,B,P] array crosses PCIe): n = number of masked points, sum_sq = sum of squared
 * errors, values[i] = exact order statistic of (0-based, ascending) rank ranks[i] -- what error_stats / numpy.quantile
 * need (calibration.py:37-40,304-310).  inliers_only = 0: mask of Calibration.reprojection_error; 1: of
 * reprojection_inliers (calibration.py:138-141).  Sharded handles combine over all ranks.                         */
int32_t mcba_error_stats(mcba_handle h, const double* x, int32_t inliers_only, int32_t n_ranks, const int64_t* ranks,
                         double* values, int64_t* n, double* sum_sq);
/* n of mcba_error_stats known without a device pass (single-GPU handles; -1 for a frame-sharded handle): the caller can
 * derive the quantile ranks first and make ONE mcba_error_stats call                                                  */
int32_t mcba_error_count(mcba_handle h, int32_t inliers_only, int64_t* n);
/* Calibration.reject_outliers on the device (calibration.py:240-252): inliers = (err < threshold) & valid at x;
 * replaces the handle's inlier table.  n_inliers / n_valid (over all ranks) may be NULL.                            */
int32_t mcba_reject_outliers(mcba_handle h, const double* x, double threshold, int64_t* n_inliers, int64_t* n_valid);
/* current inlier table in the reference's [C,F,B,P] order (a frame-sharded handle writes its own frames only, the
 * others are zero)                                                                                                 */
int32_t mcba_get_inliers(mcba_handle h, uint8_t* mask);
/* the COMPLETE inlier table in [C,F,B,P] order on every rank of a frame-sharded problem: each rank packs the bits of its
 * own frames 32 per double, ONE sum-all-reduce of ceil(C F B P / 32) doubles through the hook / RCCL ORs them (the
 * bits are disjoint, every word is an integer below 2^32), unpacked on the device.  Collective: every rank calls it.
 * On a handle that is not sharded it is mcba_get_inliers.                                                           */
int32_t mcba_gather_inliers(mcba_handle h, uint8_t* mask);

/* Projected points [C,F,B,P,2] of Calibration.reprojected (calibration.py:124-130).                            */
int32_t mcba_project(mcba_handle h, const double* x, double* projected);

/* Projected points [C,F,B,P,2] of Calibration.projected (calibration.py:113-119): the projection WITHOUT the measured
 * points, consumed by the GUI / reprojection tables (interface/view_table.py:43-52).  Rolling shutter iterates the scan
 * time from the projected row: 0.5 first, then max_iterations fixed-point passes (motion/rolling_frames.py:115-133,
 * RollingFrames.max_iterations, default 4); the other motion models ignore max_iterations.                           */
int32_t mcba_project_model(mcba_handle h, const double* x, int32_t max_iterations, double* projected);

/* One fused residual+Jacobian evaluation reduced to the normal equations at x (what one scipy `jac` call plus
 * J^T J / J^T f would produce): cost = 0.5 |f|^2 (robust-loss scaled), g = J^T f [n_params],
 * diag = diag(J^T J) [n_params].  Any output pointer may be NULL.  Sharded handles all-reduce through the hook. */
int32_t mcba_normal_equations(mcba_handle h, const double* x, const mcba_options* opt,
                              double* cost, double* g, double* diag);
/* The same evaluation at the x already resident on the device (from the last mcba_normal_equations / mcba_solve),
 * enqueued on the handle's stream without host transfer or synchronisation -- the way the solver itself evaluates.
 * Results stay in HBM; mcba_synchronize waits for the stream.                                                    */
int32_t mcba_normal_equations_device(mcba_handle h, const mcba_options* opt);
int32_t mcba_synchronize(mcba_handle h);
/* dense J^T J [n_params x n_params] assembled from the block form (debug / parity tests; small problems only)  */
int32_t mcba_dense_hessian(mcba_handle h, double* H);

/* --- parameter covariance ------------------------------------------------------------------- */
/* Gauss-Newton covariance of x at x:  Sigma = sigma2 (J^T J)^-1 over the FREE parameters, with J the Jacobian of the LINEAR
 * loss over the current inliers (exactly mcba_jacobian's).  Not part of the reference (its bundle_adjust reports no
 * uncertainty); the counterpart of the standard deviations cv2.calibrateCameraExtended returns for intrinsics.
 *   - free = not held and observed.  hold: [n_params] uint8 in the caller's x order, 1 = held (removed from the system; its
 *     rows and columns of Sigma are 0, std 0), or NULL = none held.  The problem has a 12-dimensional gauge freedom (camera
 *     poses x rig poses, rig poses x board poses): the caller holds it (multical_amd.gauge.default_hold), or the call fails.
 *   - unobserved: diag(J^T J) == 0 exactly (invalid frames / cameras / boards, frozen intrinsic columns, a skew no residual
 *     depends on).  Excluded from the system and from p_free; std NaN, covariance 0.
 *   - sigma2 <= 0: estimated as |r|^2 / (m - p_free), m = n_residuals; m <= p_free is an error.  *sigma2_out receives the
 *     value used, *dof_out = m - p_free.
 *   - rank deficiency: the system is factored in the Jacobi-scaled space (D = diag(J^T J)^-1/2, unit diagonal); any
 *     Cholesky pivot L_kk^2 < 1e-10 -- of a frame block or of the reduced system -- fails the call with a message that names
 *     the parameter ("covariance: rank deficient at x[37] (cameras[1].cx); hold more parameters").
 *   - outputs (any may be NULL): the per-frame motion parameters (DF = 6 static, 12 rolling shutter: start then end pose)
 *     are eliminated; every other parameter is SHARED.
 *       cov_shared        [n_shared, n_shared]  rows / columns in the order of shared_index (ascending caller x index)
 *       cov_frames        [F, DF, DF]           marginal block of each frame (x indices of mcba_problem's motion block)
 *       cov_frame_shared  [F, DF, n_shared]     cross blocks frame x shared (only computed when asked for)
 *       std_out           [n_params]            sqrt(diag(Sigma)) in the caller's x order
 *     Covariances between two different frames are not produced.
 *   - single handle only (a frame-sharded handle is refused); reduced systems of at most 1023 shared parameters.
 * The call evaluates the linear-loss normal equations at x on the handle; the solver's own state is rebuilt by every solve. */
/* n_shared, DF and the caller-order x index of every shared parameter (shared_index: [n_shared] or NULL) */
int32_t mcba_covariance_layout(mcba_handle h, int32_t* n_shared, int32_t* df, int32_t* shared_index);
int32_t mcba_covariance(mcba_handle h, const double* x, const uint8_t* hold, double sigma2, double* cov_shared,
                        double* cov_frames, double* cov_frame_shared, double* std_out, double* sigma2_out, int64_t* dof_out);

/* --- per-observation prediction covariance, leverage and studentised errors ------------------- */
/* The covariance of the PREDICTED point of every table slot under the covariance above:  C_i = J_i Sigma J_i^T  (2 x 2).
 * J, Sigma = sigma2 (J^T J)^-1, hold, "unobserved", sigma2, dof and the rank-deficiency rule are exactly mcba_covariance's
 * (linear loss, current inliers, Jacobi-scaled factorisation, pivot < 1e-10 -> error that names the parameter, m <= p_free
 * -> error).  Not part of the reference.
 *   - slots: every slot (c, f, b, p) of the mask mcba_reprojection_error returns as `valid`, inlier or not.  J_i is the 2 x n
 *     row pair of the model at the slot -- the row pair mcba_jacobian produces where the slot is an inlier; rolling shutter:
 *     scan time from the OBSERVED row, as in mcba_project.  Held parameters contribute nothing.  If J_i has a non-zero entry
 *     on a parameter that is unobserved and not held (a valid point in a frame without inliers: the prediction is not
 *     constrained), C_i is NaN.  Invalid slots: 0.
 *   - leverage: H_ii = C_i / sigma2 for an inlier; the covariance of its residual is sigma2 (I - H_ii), the covariance of
 *     the prediction error of a valid slot that is not an inlier is sigma2 I + C_i.
 *   - studentised error  d_i = sqrt(r_i^T Omega_i^-1 r_i),  r_i = projected - observed,  Omega_i = sigma2 I - C_i (inlier)
 *     or sigma2 I + C_i (valid, not an inlier); under the model d_i^2 is chi-square with 2 degrees of freedom.  An inlier
 *     whose H_ii has its larger eigenvalue >= 1 - 1e-9 is fitted exactly: d_i = +inf.  NaN where C_i is NaN, 0 at invalid slots.
 *   - larger eigenvalue of a symmetric 2 x 2 (uu uv; uv vv), each operation rounded once:
 *         (0.5 (uu + vv)) + sqrt((0.5 (uu - vv))^2 + uv^2)
 *   - outputs (any may be NULL), per-slot arrays in the reference's [C,F,B,P] order:
 *       pred_cov     [C,F,B,P,3]  (uu, uv, vv) of C_i
 *       student      [C,F,B,P]    d_i
 *       cam_max_std  [C]          max over the camera's valid slots of sqrt(max(larger eigenvalue of C_i, 0)); NaN slots are skipped
 *       *trace_out                sum over the inliers of tr(H_ii), reduced on the device in a fixed order (bit-repeatable);
 *                                 mathematically p_free = m - dof
 *   - not supported (refused with a message): a frame-sharded handle; the `boards` block optimised (B P 3 board-point
 *     parameters would join the shared system); reduced systems of more than 1023 shared parameters.
 * Nothing of Sigma leaves the device: the covariance chain runs once, then one pass over all table slots forms C_i = sigma2 z z^T,
 * z = M^-1 D J_i^T, from the block Cholesky factor M of the scaled system (csrc/mcba_obscov_kernels.h; a sum of squares: J_i Sigma
 * J_i^T itself cancels by 1e4 .. 1e7).                                                                                */
int32_t mcba_observation_covariance(mcba_handle h, const double* x, const uint8_t* hold, double sigma2,
                                    double* pred_cov, double* student, double* cam_max_std,
                                    double* sigma2_out, int64_t* dof_out, double* trace_out);

/* --- initialisation tables (the producer of the hot path's inputs) ---------------------------- */
/* matrix.align_transforms_robust (transform/matrix.py:140-153) for a batch of problems: problem p owns the pose pairs
 * [offsets[p], offsets[p+1]) of A and B (row-major 4x4 "points-transforming" matrices), `mask` (or NULL = all) selects
 * the pairs that enter the estimate.  Per problem: relative poses B_k A_k^-1 -> robust mean (Ward clustering of the
 * whitened rotation-vector | translation 6-vectors, most common of max(n/10, 3) clusters, transform/common.py:6-21) ->
 * errors |m A_k - B_k|_F of ALL pairs -> pairs with error < threshold * upper quartile stay -> robust mean again.
 * out[p] = the transform (identity and out_valid[p] = 0 when no pair is selected: tables.relative_between,
 * tables.py:326-332); inliers (or NULL) = pairs that passed the test.  invert != 0: relative_between_inv semantics
 * (inputs inverted, result inverted, tables.py:334-335).  This is the numeric core of tables.estimate_transform
 * (tables.py:153-176; default threshold 1.5) and tables.relative_between_n (tables.py:337-345).                      */
int32_t mcba_align_poses_robust(int32_t n_problems, const int64_t* offsets, const double* A, const double* B,
                                const uint8_t* mask, double threshold, int32_t invert, double* out, uint8_t* out_valid,
                                uint8_t* inliers);
/* The same batch with the pairs given as INDICES into pose tables: entry k of a problem is the pair
 * (table_a[index_a[k]], table_b[index_b[k]]), the tables hold n_a / n_b poses (row-major 4x4; table_a == table_b is one upload).
 * tables.estimate_relative_poses (tables.py:207-227) aligns `np.take(table, i, axis)` with `np.take(table, j, axis)` for
 * every pair of its spanning tree: the pose table [C,F,B] goes up ONCE and the pair lists as 32-bit indices, instead of two
 * gathered copies of it per pair.                                                                                      */
int32_t mcba_align_poses_indexed(int32_t n_problems, const int64_t* offsets, const double* table_a, int64_t n_a,
                                 const int32_t* index_a, const double* table_b, int64_t n_b, const int32_t* index_b,
                                 const uint8_t* mask, double threshold, int32_t invert, double* out, uint8_t* out_valid,
                                 uint8_t* inliers);

/* --- per-view board poses: the pose table tables.make_pose_table builds (tables.py:44-66) ------------------------ */
/* One board pose per (camera, frame, board) view from its detections: board.estimate_pose_points (board/common.py:36-47:
 * camera.undistort_points, then cv2.solvePnPGeneric with K and no distortion) for every view of the table in one launch
 * (csrc/mcba_pnp.h: exact undistortion by Newton's method, planar homography start, Levenberg-Marquardt to convergence on
 * sum |K pi(R X + t) - K (x, y, 1)|^2 in pixels).  Handle-less like mcba_align_poses_*.                                  */
#define MCBA_VIEW_OK 0             /* pose, sse and n_used are those of the converged optimum                          */
#define MCBA_VIEW_TOO_FEW 1        /* fewer than 4 usable corners (after corners that do not undistort are dropped)     */
#define MCBA_VIEW_MASKED 2         /* view_mask[view] == 0                                                             */
#define MCBA_VIEW_DEGENERATE 3     /* no homography: corners collinear or coincident                                   */
#define MCBA_VIEW_NOT_CONVERGED 4  /* the step test was not met within max_iterations (the last iterate is returned)   */
typedef struct mcba_view_pose_problem {
  int32_t C, F, B, P;             /* cameras, frames, boards, padded corners per board                                 */
  const double* points;           /* [C,F,B,P,2] detected corners (pixels)                                             */
  const uint8_t* valid;           /* [C,F,B,P]                                                                         */
  const double* board_points;     /* [B,P,3] board geometry, padded                                                    */
  const int32_t* board_sizes;     /* [B] corners of every board (the rest of P is padding), or NULL = P                */
  const double* cameras;          /* [C, 5 + n_dist] parameter blocks [fx fy cx cy skew dist...] (camera.py:144-171)    */
  int32_t n_dist;                 /* width of the dist part of every block                                             */
  const int32_t* camera_n_dist;   /* [C] coefficients each camera really has (4, 5, 8, 12 or 14), or NULL = n_dist      */
  const uint8_t* is_fisheye;      /* [C] Kannala-Brandt (4 coefficients) instead of Brown-Conrady, or NULL = none       */
  const uint8_t* fix_aspect;      /* [C] fy = fx (camera.py:159-160), or NULL = none                                    */
  const uint8_t* view_mask;       /* [C,F,B] views to estimate (has_min_detections), or NULL = every view; views with   */
                                  /* fewer than 4 corners are never estimated                                          */
  const double* init_poses;       /* [C,F,B,4,4] start of the refinement, or NULL = planar homography start; required   */
                                  /* for a board whose points are not coplanar                                         */
  int32_t max_iterations;         /* Levenberg-Marquardt linearisations per view; <= 0: 50                              */
  int32_t* lm_iterations;         /* OUT [C,F,B] linearisations used, or NULL                                          */
} mcba_view_pose_problem;
/* poses [C,F,B,4,4] board -> camera; sse [C,F,B] sum of squared pixel distances at the optimum (raw: no error norm is baked
 * in); n_used [C,F,B] corners that entered; status [C,F,B] MCBA_VIEW_*.  Views without a pose: identity, sse 0, n_used 0.  */
int32_t mcba_view_poses(const mcba_view_pose_problem* p, double* poses, double* sse, int32_t* n_used, uint8_t* status);
/* timing of the last mcba_view_poses call of this thread, milliseconds: [0] host preparation + compaction of the active views,
 * [1] uploads, [2] kernel, [3] downloads + scatter; *n_active (or NULL) = views launched                               */
int32_t mcba_debug_view_poses_ms(double* ms /*[4]*/, int64_t* n_active);

/* --- single-camera intrinsic calibration: Camera.calibrate / CameraFisheye.calibrate (camera.py:69-105) ------------ */
/* Intrinsics of every camera from its own detections, all cameras in one call (csrc/mcba_intrinsic.h: homography + focal start,
 * per-view poses by the mathematics of mcba_view_poses, then Levenberg-Marquardt over fx fy cx cy | dist | one pose per view with
 * the views eliminated by a Schur complement, iterated to convergence).  A view is one (frame, board) slot.  Handle-less like
 * mcba_view_poses; same error convention, the caller owns every array.                                                     */
#define MCBA_CAMERA_OK 0             /* the converged optimum                                                            */
#define MCBA_CAMERA_TOO_FEW_VIEWS 1  /* fewer than 3 usable views                                                        */
#define MCBA_CAMERA_DEGENERATE 2     /* no focal start (e.g. every view fronto-parallel) or a non-finite cost            */
#define MCBA_CAMERA_NOT_CONVERGED 3  /* the step test was not met within max_iterations (the last iterate is returned)   */
#define MCBA_CAMERA_MASKED 4         /* every view of the camera is masked out                                           */
typedef struct mcba_intrinsic_problem {
  int32_t C, F, B, P;             /* cameras, frames, boards, padded corners per board                                 */
  const double* points;           /* [C,F,B,P,2] detected corners (pixels)                                             */
  const uint8_t* valid;           /* [C,F,B,P]                                                                         */
  const double* board_points;     /* [B,P,3] board geometry, padded                                                    */
  const int32_t* board_sizes;     /* [B] corners of every board, or NULL = P                                           */
  const double* image_sizes;      /* [C,2] width, height                                                               */
  int32_t n_dist;                 /* width of the dist part of every camera block (4 .. 14)                            */
  const int32_t* camera_n_dist;   /* [C] coefficients each camera really has (4, 5, 8, 12 or 14), or NULL = n_dist      */
  const uint8_t* is_fisheye;      /* [C] Kannala-Brandt (4 coefficients), or NULL = none                                */
  const uint8_t* fix_aspect;      /* [C] fy = fx, or NULL = none                                                        */
  const uint8_t* free_dist;       /* [C,n_dist] 1 = estimated, 0 = held at its start value; NULL = all of the camera's  */
  const uint8_t* view_mask;       /* [C,F,B] views to use, or NULL = every view; views under 4 corners are never used   */
  const double* init_cameras;     /* [C, 5 + n_dist] warm start, or NULL = the homography start                         */
  const double* init_poses;       /* [C,F,B,4,4] warm start (given exactly when init_cameras is)                        */
  int32_t max_iterations;         /* Levenberg-Marquardt passes per camera; <= 0: 100                                   */
  int32_t* lm_iterations;         /* OUT [C] passes used, or NULL                                                       */
} mcba_intrinsic_problem;
/* cameras [C, 5 + n_dist] blocks [fx fy cx cy skew dist...] (skew 0; under fix_aspect fy = fx); poses [C,F,B,4,4] board ->
 * camera; sse [C,F,B] sum of squared pixel distances of the view at the optimum; n_used [C,F,B]; view_status MCBA_VIEW_*;
 * camera_status [C] MCBA_CAMERA_*.  Views that are not used: identity, sse 0, n_used 0.                                  */
int32_t mcba_calibrate_intrinsics(const mcba_intrinsic_problem* p, double* cameras, double* poses, double* sse, int32_t* n_used,
                                  uint8_t* view_status, uint8_t* camera_status);
/* timing of the last mcba_calibrate_intrinsics call of this thread, milliseconds: [0] host preparation + compaction, [1] uploads,
 * [2] kernels (start, view poses, refinement), [3] downloads + scatter; *n_views (or NULL) = views uploaded             */
int32_t mcba_debug_calibrate_intrinsics_ms(double* ms /*[4]*/, int64_t* n_views);

/* --- robot-world hand-eye start: HandEye.initialise_camera_poses / HandEyeCalibration.initialise ------------------- */
/* cv2.calibrateRobotWorldHandEye(..., CALIB_ROBOT_WORLD_HAND_EYE_SHAH) for a batch of independent problems: find X, Z with
 * A_i X = Z B_i over pairs of "points-transforming" poses (csrc/mcba_handeye.h: Shah's Kronecker-product closed form -- the
 * rotations from the leading singular vectors of sum kron(R_A_i, R_B_i), the translations from a 6x6 least-squares system).
 * The reference makes one such call per (master camera, slave camera, master board, slave board) combination of a
 * non-overlapping rig (hand_eye/hand_eye.py:35-57 through master_slave_pair, :82-107, and hand_eye_robot_world, :110-121) and
 * one more in HandEyeCalibration.initialise (optimization/hand_eye.py:22-36 through transform/hand_eye.py:20-50); here the pose
 * tables go up once and the problems are index pairs, as in mcba_align_poses_indexed.  Handle-less like mcba_view_poses; same
 * error convention, the caller owns every array.                                                                          */
#define MCBA_HANDEYE_OK 0          /* X, Z and err are those of the closed form                                           */
#define MCBA_HANDEYE_TOO_FEW 1     /* fewer than 3 usable pairs (hand_eye/hand_eye.py:94)                                  */
#define MCBA_HANDEYE_DEGENERATE 2  /* the rotations do not determine (X, Z): all equal (pure translations) or about one     */
                                   /* common axis; or non-finite input                                                     */
typedef struct mcba_hand_eye_problem {
  int32_t F;                      /* frames: poses per table row                                                        */
  int64_t n_a, n_b;               /* rows of the two tables                                                             */
  const double* table_a;          /* [n_a,F,4,4] the A side                                                             */
  const uint8_t* valid_a;         /* [n_a,F]                                                                            */
  const double* table_b;          /* [n_b,F,4,4] the B side; table_b == table_a and valid_b == valid_a: one upload      */
  const uint8_t* valid_b;         /* [n_b,F]                                                                            */
  int32_t n_problems;             /* problem p pairs row index_a[p] of A with row index_b[p] of B over every frame that  */
  const int32_t* index_a;         /* [n_problems]                                  is valid in both                      */
  const int32_t* index_b;         /* [n_problems]                                                                       */
  int32_t invert_inputs;          /* != 0: every pose is inverted (rigidly) on the device before it enters --            */
                                  /* master_slave_pair inverts the board -> camera poses (hand_eye/hand_eye.py:96-97)    */
} mcba_hand_eye_problem;
/* Outputs, any of which may be NULL: X [n_problems,4,4], Z [n_problems,4,4]; n_pairs [n_problems] frames that entered; status
 * [n_problems] MCBA_HANDEYE_*; err [n_problems,F] |A_i X - Z B_i|_F of the frames that entered (transform/hand_eye.py:47-50), 0
 * elsewhere.  Problems without a result: identities, err 0.  With the reference's argument order (world_wrt_camera,
 * base_wrt_gripper) = (A, B): X = base_wrt_world, Z = gripper_wrt_camera.                                                  */
int32_t mcba_hand_eye(const mcba_hand_eye_problem* p, double* X, double* Z, int32_t* n_pairs, uint8_t* status, double* err);
/* timing of the last mcba_hand_eye call of this thread, milliseconds: [0] host preparation, [1] uploads, [2] kernel,
 * [3] downloads; *n_problems (or NULL) = problems launched                                                              */
int32_t mcba_debug_hand_eye_ms(double* ms /*[4]*/, int64_t* n_problems);

/* --- using a calibration: project, undistort points, undistortion maps, bicubic remap ------------------------------- */
/* The numeric surface of the reference's Camera / CameraFisheye beyond the bundle adjustment (csrc/mcba_undistort.h: the
 * projection of the kernels and its exact Newton inverse; maps in float32; cv2's bicubic kernel, A = -0.75, in float32 with a
 * constant border).  Handle-less like mcba_view_poses; same error convention, the caller owns every array.  An unsupported
 * camera family, channel count or pixel type is an error, never another route.                                          */
typedef struct mcba_camera_set {
  int32_t C;                      /* cameras                                                                            */
  const double* cameras;          /* [C, 5 + n_dist] parameter blocks [fx fy cx cy skew dist...] (camera.py:144-171); the   */
                                  /* projections read fx fy cx cy, the skew enters only the default P of the maps          */
  int32_t n_dist;                 /* width of the dist part of every block                                              */
  const int32_t* camera_n_dist;   /* [C] coefficients each camera really has (4, 5, 8, 12 or 14), or NULL = n_dist       */
  const uint8_t* is_fisheye;      /* [C] Kannala-Brandt (4 coefficients) instead of Brown-Conrady, or NULL = none        */
} mcba_camera_set;
#define MCBA_PIXEL_U8 0
#define MCBA_PIXEL_F32 1
#define MCBA_UNDISTORT_OK 0             /* the inverse converged                                                         */
#define MCBA_UNDISTORT_NOT_CONVERGED 1  /* the pixel lies outside the model's monotone range: the output is NaN            */
/* Camera.project (camera.py:124-128, camera_fisheye.py:113-117): uv [n,2] pixels of the camera-frame points X [n,3];
 * camera_of_point [n], or NULL = camera 0.  n == 0 launches nothing.                                                     */
int32_t mcba_project_points(const mcba_camera_set* cams, int64_t n, const int32_t* camera_of_point, const double* X, double* uv);
/* Camera.undistort_points (camera.py:119-122, camera_fisheye.py:108-111): out [n,2] = P [X/W, Y/W, 1], [X Y W] = R [x y 1] of
 * the undistorted normalised point; R, P [C,3,3] or NULL (identity; the normalised point itself); status [n] MCBA_UNDISTORT_*.  */
int32_t mcba_undistort_points(const mcba_camera_set* cams, int64_t n, const int32_t* camera_of_point, const double* uv,
                              const double* R, const double* P, double* out, uint8_t* status);
/* Camera.undistort_map (camera.py:113-117, camera_fisheye.py:102-106: initUndistortRectifyMap, CV_32FC2): maps [C,height,width,2]
 * source coordinate (x, y) of every destination pixel; R [C,3,3] or NULL = identity, P [C,3,3] or NULL = the camera's own matrix.
 * A pixel that looks behind the camera: NaN.                                                                            */
int32_t mcba_undistort_maps(const mcba_camera_set* cams, const double* R, const double* P, int32_t width, int32_t height,
                            float* maps);
/* cv2.remap(image, map, None, INTER_CUBIC) (camera.py:244-246) of N images [N,Hs,Ws,channels] of one size, image i through map
 * map_of_image[i] of maps [M,Hd,Wd,2]: dst [N,Hd,Wd,channels].  channels 1 or 3; dtype MCBA_PIXEL_*; constant border.          */
int32_t mcba_remap(const void* src, int32_t N, int32_t Hs, int32_t Ws, int32_t channels, int32_t dtype, const float* maps,
                   int32_t M, int32_t Hd, int32_t Wd, const int32_t* map_of_image, double border, void* dst);
/* camera.undistort_images (camera.py:249-258) in one launch: the map coordinate is computed in registers where the remap needs
 * it, the result is that of the remap through the undistortion maps of the same R, P, byte for byte.                    */
int32_t mcba_undistort_images(const mcba_camera_set* cams, const double* R, const double* P, const void* src, int32_t N,
                              int32_t Hs, int32_t Ws, int32_t channels, int32_t dtype, const int32_t* camera_of_image, int32_t Hd,
                              int32_t Wd, double border, void* dst);

/* --- using a calibration: triangulate points through the rig --------------------------------------------------------- */
/* The 3-D point behind the pixels that the cameras of a calibrated rig saw at once, for F frames of M points each in one launch
 * (csrc/mcba_triangulate.h: exact undistortion, plane-intersection start, Levenberg-Marquardt on the pixel residuals of the
 * project's own projection to a whitened step of 1e-10 px).  A view is a (camera, frame) pair with the row-major 3 x 4 matrix that
 * takes a point into the camera frame: the top three rows of camera_pose[c] @ rig_pose[f].  Rolling shutter: an observation at row
 * v sees (1 - t) views + t views_end, t = v / image_heights[c].  Handle-less like mcba_view_poses; same error convention, the
 * caller owns every array.  The records of a frame are staged in LDS: more than MCBA_TRI_MAX_CAMERAS cameras are refused.        */
#define MCBA_TRI_MAX_CAMERAS 64
#define MCBA_TRI_OK 0              /* converged                                                                          */
#define MCBA_TRI_TOO_FEW 1         /* fewer than 2 usable views (valid, finite, inside the model's monotone range): no point  */
#define MCBA_TRI_DEGENERATE 2      /* the rays are parallel or one and the same: no point                                 */
#define MCBA_TRI_NOT_CONVERGED 3   /* max_iterations linearisations did not meet the stop rule: the last iterate         */
#define MCBA_TRI_BEHIND 4          /* the returned point lies at or behind the plane of a view that entered              */
typedef struct mcba_triangulate_problem {
  mcba_camera_set cams;          /* C cameras */
  int32_t F; int64_t M;          /* frames, points per frame */
  const double* views;           /* [C,F,3,4] */
  const double* views_end;       /* [C,F,3,4] or NULL (no rolling shutter) */
  const double* image_heights;   /* [C], required with views_end */
  const uint8_t* view_valid;     /* [C,F] or NULL */
  const double* points;          /* [C,F,M,2] pixels */
  const uint8_t* valid;          /* [C,F,M] */
  double sigma_px; int32_t max_iterations;   /* sigma_px <= 0: sse / (2 n - 3) per point; max_iterations <= 0: 20, at most 100 */
} mcba_triangulate_problem;
/* Outputs: X [F,M,3]; cov [F,M,6] upper triangle (xx xy xz yy yz zz) of sigma^2 (J^T J)^-1 at X; sse [F,M] squared pixel residuals;
 * err [C,F,M] reprojection error of every view that entered, 0 elsewhere; n_views [F,M] usable views; status [F,M] MCBA_TRI_*.
 * Points without a result: NaN in X and cov, sse 0.  cov, sse, err and n_views may be NULL.  F * M == 0 launches nothing.       */
int32_t mcba_triangulate(const mcba_triangulate_problem* p, double* X, double* cov, double* sse, double* err, int32_t* n_views,
                         uint8_t* status);
/* timing of the last mcba_triangulate call of this thread, milliseconds: [0] uploads, [1] kernel (HIP events around the launch),
 * [2] downloads, [3] the whole call; *n_points (or NULL) = points launched                                                 */
int32_t mcba_debug_triangulate_ms(double* ms /*[4]*/, int64_t* n_points);

/* --- using a calibration: localise the rig in frames that were not part of it (multi-camera PnP) ---------------------- */
/* The dual of mcba_triangulate: cameras, camera poses, boards and board poses are held, and the rig pose of each of F frames is
 * found from that frame's detections alone (csrc/mcba_localize.h: one workgroup per frame, Levenberg-Marquardt on the pixel
 * residuals of the project's own projection over the global rotation vector and the translation of the frame's pose -- start, then
 * end under rolling shutter, t = v / image_heights[c] -- to a whitened step of 1e-10 px).  An observation is usable where valid and
 * board_valid say so and the pixel is finite.  Without `init` a frame starts from the best of up to four candidates
 * camera_pose[c]^-1 T_view board_pose[b]^-1 of its largest views (the mathematics of mcba_view_poses; status OK, most corners first),
 * scored over all its observations; a frame none of whose views gives a pose has no start.  Handle-less like mcba_view_poses; same
 * error convention, the caller owns every array.  More than MCBA_RIG_MAX_CAMERAS cameras are refused.                            */
#define MCBA_RIG_MAX_CAMERAS 64
#define MCBA_RIG_OK 0              /* converged                                                                          */
#define MCBA_RIG_TOO_FEW 1         /* fewer than 3 usable observations (6 under rolling shutter): no pose                 */
#define MCBA_RIG_DEGENERATE 2      /* a vanishing pivot of the scaled normal matrix (collinear points), a cost that is not  */
                                   /* finite, or no start: no pose                                                        */
#define MCBA_RIG_NOT_CONVERGED 3   /* max_iterations linearisations did not meet the stop rule: the last iterate         */
#define MCBA_RIG_BEHIND 4          /* an observation that entered ends at or behind its camera                            */
typedef struct mcba_rig_pose_problem {
  mcba_camera_set cams;          /* C cameras */
  int32_t F, B, P;               /* frames, boards, padded corners per board */
  const double* camera_poses;    /* [C,4,4] rig -> camera */
  const double* board_poses;     /* [B,4,4] board -> world */
  const double* board_points;    /* [B,P,3] board geometry, padded at the end of a row */
  const uint8_t* board_valid;    /* [B,P] or NULL = every point; holes allowed (a masked point enters nothing, the start's plane fit included) */
  const double* points;          /* [C,F,B,P,2] pixels */
  const uint8_t* valid;          /* [C,F,B,P] */
  const double* init;            /* [F,4,4] start poses world -> rig, or NULL = from the frame's views */
  const double* init_end;        /* [F,4,4] start of the end poses (rolling), or NULL = init */
  int32_t rolling;               /* != 0: 12 unknowns a frame */
  const double* image_heights;   /* [C], required with rolling */
  double sigma_px; int32_t max_iterations;   /* sigma_px <= 0: the frame's own sse / (2 n - k); max_iterations <= 0: 20, at most 100 */
} mcba_rig_pose_problem;
/* Outputs: poses [F,4,4]; poses_end [F,4,4] (rolling; identity otherwise); cov [F,21] or [F,78] upper triangle by rows of
 * sigma^2 (J^T J)^-1 over (rx ry rz tx ty tz) of the start, then of the end; sse [F]; n_obs [F] usable observations; iters [F]
 * linearisations; err [C,F,B,P] reprojection error of every observation that entered, 0 elsewhere; status [F] MCBA_RIG_*.  Frames
 * without a result: identity, sse 0, NaN in cov (also where sigma_px <= 0 and 2 n = k).  Every output but poses and status may be
 * NULL.  F == 0 or a table without a usable observation launches nothing.                                                  */
int32_t mcba_rig_poses(const mcba_rig_pose_problem* p, double* poses, double* poses_end, double* cov, double* sse, int32_t* n_obs,
                       int32_t* iters, double* err, uint8_t* status);
/* timing of the last mcba_rig_poses call of this thread, milliseconds: [0] uploads, [1] start kernel (k_view_pose; 0 with init),
 * [2] refinement kernel (both by HIP events), [3] downloads, [4] the whole call; *n_frames (or NULL) = frames launched       */
int32_t mcba_debug_rig_poses_ms(double* ms /*[5]*/, int64_t* n_frames);

/* --- stereo calibration of camera pairs with the cameras held (batched stereoCalibrate) -------------------------------- */
/* The relative pose of n_pairs pairs (l, r) of cameras of one detection table, every pair from its own common views, all pairs in
 * one launch (csrc/mcba_stereo.h: one workgroup per pair, Levenberg-Marquardt over T_rel -- left-camera frame -> right-camera
 * frame, X_r = R X_l + T, the reference's matrix.join(R, T) -- and one board pose per view, on the pixel residuals of the
 * project's own projection in both cameras).  A view of a pair is a (frame, board) slot whose view_valid is set for both cameras
 * and which holds at least min_common corners that are valid in both cameras and in board_valid, with finite pixels; only those
 * corners enter; a slot whose common corners lie on one line (to 1e-6 of their extent) is dropped.  The view starts from the left
 * camera's view_poses entry, T_rel from the best of up to four candidates T_{r,v} T_{l,v}^-1 of the views with the most common
 * corners, scored over all the pair's views.  The model is cv2's static one with CALIB_FIX_INTRINSIC: no rolling shutter, no free
 * intrinsics.  Handle-less like mcba_view_poses; same error convention, the caller owns every array.                        */
#define MCBA_STEREO_OK 0              /* converged                                                                        */
#define MCBA_STEREO_TOO_FEW 1         /* the pair has no view: no pose                                                    */
#define MCBA_STEREO_DEGENERATE 2      /* all the pair has are slots of collinear common corners; or a vanishing pivot of a  */
                                      /* scaled view block or of the scaled reduced matrix at the returned point, a cost     */
                                      /* that is not finite, no start candidate with a finite score: no pose               */
#define MCBA_STEREO_NOT_CONVERGED 3   /* max_iterations passes did not meet the step rule: the last iterate                */
typedef struct mcba_stereo_problem {
  mcba_camera_set cams;          /* C cameras */
  int32_t F, B, P;               /* frames, boards, padded corners per board */
  const double* board_points;    /* [B,P,3] board geometry, padded at the end of a row */
  const uint8_t* board_valid;    /* [B,P] or NULL = every point */
  const double* points;          /* [C,F,B,P,2] pixels */
  const uint8_t* valid;          /* [C,F,B,P] */
  const double* view_poses;      /* [C,F,B,4,4] start poses board -> camera (what mcba_view_poses returns) */
  const uint8_t* view_valid;     /* [C,F,B] the start pose of the view may be used */
  int32_t n_pairs;
  const int32_t* pairs;          /* [n_pairs,2] left, right; l == r or an index out of range is an error */
  int32_t min_common;            /* <= 0: 4; below 3 is an error */
  int32_t max_iterations;        /* passes of the loop (rejected steps count); <= 0: 100, at most 1000 */
  double sigma_px;               /* <= 0: the pair's own sse / (4 n_points - 6 - 6 n_views) */
} mcba_stereo_problem;
/* Outputs: T [n_pairs,4,4]; cov [n_pairs,6,6] = sigma^2 (H_rr - sum_v S_v)^-1 over (rx ry rz tx ty tz) of T_rel, the view poses
 * eliminated, at the returned point; sse [n_pairs] squared pixel residuals of both cameras; n_views, n_points [n_pairs] views and
 * common corners that entered (a corner counts once); iterations [n_pairs]; view_poses_out [n_pairs,F,B,4,4] board -> left
 * camera, identity where the slot is no view of the pair; view_sse [n_pairs,F,B,2] left | right; status [n_pairs] MCBA_STEREO_*.
 * Pairs without a result: identity, NaN covariance (also where the degree of freedom is not positive), sse 0.  Every output but
 * T and status may be NULL.  Pairs without a view are not launched; n_pairs == 0 or no pair with a view touches no device.     */
int32_t mcba_stereo_calibrate(const mcba_stereo_problem* p, double* T, double* cov, double* sse, int32_t* n_views, int32_t* n_points,
                              int32_t* iterations, double* view_poses_out, double* view_sse, uint8_t* status);
/* timing of the last mcba_stereo_calibrate call of this thread, milliseconds: [0] host preparation, [1] uploads, [3] downloads +
 * scatter by host clock, [2] the kernel by HIP events around its launch; *n_pairs (or NULL) = pairs launched               */
int32_t mcba_debug_stereo_calibrate_ms(double* ms /*[4]*/, int64_t* n_pairs);

/* --- using a calibration: projection uncertainty where no board was ------------------------------------------------- */
/* The 2 x 2 covariance of where a point projects into camera b when the shared parameters vary with their covariance
 * (csrc/mcba_uncertainty.h), for pixels anywhere in the image.  A job is one camera, one reference, one inverse
 * distance and one factor W of the covariance; its queries are a grid generated on the device or a list of pixels.
 *   reference < 0   the point n_b(q) / inv_distance is fixed in the rig frame; intrinsics and pose of `camera` vary: K = KI_b + 6
 *   reference = a   camera a sees the point at pixel q at that distance; the result is the covariance of where `camera` sees it:
 *                   K = KI_b + 6 + 6 + KI_a.  reference == camera returns exactly 0.
 * KI_c = 4 + the camera's own coefficient count; n(q) the unit ray of the pixel through the exact inverse; inv_distance = 0: a
 * direction.  W [K, r] row-major with W W^T = the covariance of the job's columns, in the order
 *   fx fy cx cy dist.. of b | left perturbation (omega, tau) of camera_poses[b] | the same of a | fx fy cx cy dist.. of a
 * (T -> exp(omega, tau) T; the caller folds d(omega, tau) / d(stored pose parameters) into W).  unconstrained [K] flags columns that
 * no residual constrains and that are not held: a query whose row pair J has a non-zero entry there is MCBA_UNC_UNCONSTRAINED.
 * C = (J W)(J W)^T.  Handle-less like mcba_view_poses; same error convention, the caller owns every array.                  */
#define MCBA_UNC_MAX_K 48
#define MCBA_UNC_OK 0
#define MCBA_UNC_NOT_CONVERGED 1   /* the pixel (or where it lands in b) lies outside the monotone range of a model: NaN      */
#define MCBA_UNC_BEHIND 2          /* transfer: the point lies at or behind the plane of camera b: NaN                        */
#define MCBA_UNC_UNCONSTRAINED 3   /* J is non-zero on an unconstrained column: NaN                                           */
typedef struct mcba_uncertainty_job {
  int32_t camera, reference;     /* b; a or < 0 = the rig frame */
  double inv_distance;           /* >= 0, finite */
  int32_t K, r;                  /* rows and columns of W; r = 0 .. MCBA_UNC_MAX_K (0: C = 0) */
  const double* W;               /* [K, r] */
  const uint8_t* unconstrained;  /* [K] or NULL = none */
  int32_t grid_w, grid_h;        /* grid_w > 0: grid_w x grid_h queries, row-major, query (ix, iy) = (u0 + ix du, v0 + iy dv) */
  double u0, v0, du, dv;
  int64_t n;                     /* grid_w == 0: n queries */
  const double* uv;              /* [n,2] pixels */
} mcba_uncertainty_job;
/* Outputs, the jobs' queries one after the other (n_total of them): cov [n_total,3] (uu, uv, vv); std [n_total] or NULL = sqrt of
 * the larger eigenvalue by the formula of mcba_observation_covariance (one rounding per operation); status [n_total] MCBA_UNC_*.
 * camera_poses [C,4,4] rig -> camera.  Zero queries launch nothing.                                                          */
int32_t mcba_projection_uncertainty(const mcba_camera_set* cams, const double* camera_poses, int32_t n_jobs,
                                    const mcba_uncertainty_job* jobs, double* cov, double* std, uint8_t* status);
/* timing of the last mcba_projection_uncertainty call of this thread, milliseconds: [0] uploads, [1] kernel (HIP events around the
 * launch), [2] downloads, [3] the whole call; *n_queries (or NULL) = queries launched                                        */
int32_t mcba_debug_projection_uncertainty_ms(double* ms /*[4]*/, int64_t* n_queries);

/* --- comparing two calibrations: projection difference maps --------------------------------------------------------- */
/* Where calibration 1 projects what calibration 0 sees at a pixel (csrc/mcba_projdiff.h).  The two camera sets
 * have the same camera count; the families may differ.  A job is one camera, one reference, one inverse distance and one fit
 * mode; its queries are a grid generated on the device or a list of pixels, as in mcba_uncertainty_job.
 *   reference < 0   intrinsics difference: Y = n_b^0(q), q' = project_b^1(R(omega) Y + inv_distance tau), diff = q' - q.
 *                   (omega, tau) is the job's implied transform, fitted on the device before the map: it minimises sum |diff|^2
 *                   over the job's FIT PIXELS (a grid fit_grid_w x fit_grid_h or a list fit_uv of their own, at most
 *                   MCBA_PDIFF_MAX_FIT), of which those inside the focus disc take part (focus_radius <= 0: all) whose inverse
 *                   under calibration 0 converges and whose projection under calibration 1 is valid at the identity.
 *                   fit: NONE (identity), ROTATION (3 unknowns), RIGID (6; refused at inv_distance = 0).
 *   reference = a   transfer difference: Y_a^k = n_a^k(q), Y_b^k = R_ba^k Y_a^k + inv_distance t_ba^k, q_b^k = project_b^k(Y_b^k),
 *                   diff = q_b^1 - q_b^0 and landing = q_b^0.  No fit (fit and the fit pixels are ignored).  a == camera: exactly 0.
 * n_c^k(q): the unit ray of the pixel through the exact inverse of camera c under calibration k; poses [C,4,4] rig -> camera.
 * Handle-less like mcba_projection_uncertainty; same error convention, the caller owns every array.                          */
#define MCBA_PDIFF_MAX_FIT 65536
#define MCBA_PDIFF_OK 0
#define MCBA_PDIFF_NOT_CONVERGED 1     /* the pixel (or where it lands) lies outside the monotone range of a model: NaN        */
#define MCBA_PDIFF_BEHIND 2            /* the point lies at or behind the plane of the camera, under either calibration: NaN  */
#define MCBA_PDIFF_NO_FIT 3            /* the job's fit did not end MCBA_PDIFF_FIT_OK: NaN                                      */
#define MCBA_PDIFF_FIT_OK 0
#define MCBA_PDIFF_FIT_TOO_FEW 1       /* fewer than 2 (ROTATION) or 3 (RIGID) fit pixels take part                            */
#define MCBA_PDIFF_FIT_NOT_CONVERGED 2
#define MCBA_PDIFF_FIT_DEGENERATE 3    /* the damped system is not well posed                                                  */
#define MCBA_PDIFF_MODE_NONE 0
#define MCBA_PDIFF_MODE_ROTATION 1
#define MCBA_PDIFF_MODE_RIGID 2
typedef struct mcba_projdiff_job {
  int32_t camera, reference;     /* b; a or < 0 = the camera itself */
  double inv_distance;           /* >= 0, finite */
  int32_t fit;                   /* MCBA_PDIFF_MODE_* */
  int32_t fit_grid_w, fit_grid_h;  /* fit_grid_w > 0: the fit pixels are a grid (fit_u0 + ix fit_du, fit_v0 + iy fit_dv) */
  double fit_u0, fit_v0, fit_du, fit_dv;
  int64_t fit_n;                 /* fit_grid_w == 0: fit_n fit pixels */
  const double* fit_uv;          /* [fit_n,2] */
  double focus_u, focus_v, focus_radius;   /* pixels; focus_radius <= 0: the whole image */
  int32_t grid_w, grid_h;        /* the queries, as in mcba_uncertainty_job */
  double u0, v0, du, dv;
  int64_t n;
  const double* uv;              /* [n,2] pixels */
} mcba_projdiff_job;
/* Outputs.  Per job: transform [n_jobs,6] rotation vector | translation (0 for a job without a fit, NaN for a fit that did not
 * end OK); fit_info [n_jobs,5] = n_fit, iterations (linearisations), RMS of |diff| over the fit pixels before and after the fit,
 * MCBA_PDIFF_FIT_* (each an exact double; NaN RMS where there is none).  Either may be NULL.  Per query, the jobs' queries one after
 * the other (n_total): diff [n_total,2]; magnitude [n_total] or NULL; landing [n_total,2] or NULL (NaN for intrinsics jobs); status
 * [n_total] MCBA_PDIFF_*.  Everything of a query is NaN unless its status is OK.  Zero queries launch nothing, the fit
 * included: transform and fit_info are then those of jobs without a fit (0, n_fit 0, NaN RMS, MCBA_PDIFF_FIT_OK).            */
int32_t mcba_projection_diff(const mcba_camera_set* cams0, const double* poses0, const mcba_camera_set* cams1, const double* poses1,
                             int32_t n_jobs, const mcba_projdiff_job* jobs, double* transform, double* fit_info, double* diff,
                             double* magnitude, double* landing, uint8_t* status);
/* timing of the last mcba_projection_diff call of this thread, milliseconds: [0] uploads, [1] fit kernel, [2] map kernel (both by
 * HIP events), [3] downloads, [4] the whole call; *n_queries (or NULL) = queries launched                                       */
int32_t mcba_debug_projection_diff_ms(double* ms /*[5]*/, int64_t* n_queries);

/* --- planning the next captures: information gain of candidate views -------------------------------------------------- */
/* What a new view of a board adds to the intrinsics of the camera that sees it, and what it does to the projection uncertainty
 * over a focus region (csrc/mcba_guidance.h).  Per camera c: W [KI_c, r] row-major with W W^T = the covariance of
 * its columns fx fy cx cy dist.. (KI_c = 4 + the camera's own coefficient count; the W of a rig-frame job of
 * mcba_projection_uncertainty, camera rows only), r = 0 .. MCBA_GUIDE_MAX_R (0: everything held), `unconstrained` != 0: an
 * intrinsic that no residual constrains and that is not held, and the image size.
 * A view is a set of points seen by `camera` with n_nuisance = 0, 3 or 6 free parameters of its own (nothing | a rotation | a
 * rigid motion), eliminated before anything is reported:
 *   board >= 0   the points of that board (board_points [n_boards, board_stride, 3], the first board_n[board] of a board) at
 *                the board-in-camera pose `pose` (3 x 4, row-major); a point is visible in front of the camera, inside the image
 *                by `margin` pixels, where the model is monotone;
 *   board < 0    a focus: the unit rays of a grid or a list of pixels (as in mcba_uncertainty_job) at inv_distance (0: directions;
 *                n_nuisance = 6 needs inv_distance > 0); a pixel is visible where the exact inverse converges.
 * S_v [r, r] is the Schur complement of the nuisance block in the Gram matrix of the rows [Kc W | E] of the visible points.
 * A_v = S_v / sigma2; against a base B_c (I at first, + A of every pick):  gain = (log det(B_c + A_v) - log det B_c) / 2 in nats,
 * focus_rms = sqrt(trace((B_c + A_v)^-1 Q_c) / n) in pixels, Q_c and n the S and the visible count of foci[c].
 * Greedy selection: n_picks rounds; a round scores every candidate, takes per camera the best by `criterion` (ties: the lowest
 * index; a view is picked once), adds its A to B_c.  Handle-less like mcba_projection_uncertainty; same error convention, the
 * caller owns every array.                                                                                                     */
#define MCBA_GUIDE_MAX_R 18
#define MCBA_GUIDE_OK 0
#define MCBA_GUIDE_TOO_FEW 1        /* fewer than min_points points are visible                                               */
#define MCBA_GUIDE_DEGENERATE 2     /* the nuisance block is not positive definite (collinear points, ...)                    */
#define MCBA_GUIDE_UNCONSTRAINED 3  /* the camera has an unconstrained intrinsic: no finite prior                             */
#define MCBA_GUIDE_BY_FOCUS 0
#define MCBA_GUIDE_BY_GAIN 1
typedef struct mcba_guidance_camera {
  int32_t r, unconstrained;
  const double* W;               /* [KI_c, r] */
  double image_w, image_h;
} mcba_guidance_camera;
typedef struct mcba_guidance_view {
  int32_t camera, n_nuisance, min_points, board;
  double pose[12];               /* board >= 0 */
  double inv_distance;           /* board < 0: >= 0, finite */
  int32_t grid_w, grid_h;        /* board < 0, grid_w > 0: a grid, as in mcba_uncertainty_job */
  double u0, v0, du, dv;
  int64_t n;                     /* board < 0, grid_w == 0: n pixels */
  const double* uv;              /* [n,2] */
} mcba_guidance_view;
/* Outputs; rs = max(1, the largest r of the call) is the row stride of every matrix, camera c uses the leading r_c x r_c block.
 * Per view: n_visible, status MCBA_GUIDE_*, gain and focus_rms against B = I (NaN unless OK; a camera with r = 0: OK, 0, 0, and
 * n_visible 0: nothing is launched for it), S [n_views, rs, rs] or NULL (0 unless OK).  Per camera: focus_status, focus_n_visible,
 * focus_before (focus_rms of the base I; NaN without an OK focus), Q [C, rs, rs] (each or NULL); picks [C, n_picks] (view index, -1:
 * none left), pick_gain (conditional on the earlier picks), pick_focus_rms (after the pick); posterior [C, rs, rs] or NULL =
 * (B_c)^-1 after the last pick.  round_gain / round_focus_rms [n_picks, n_views] or NULL: the scores of every round.           */
typedef struct mcba_guidance_result {
  int32_t* n_visible;
  uint8_t* status;
  double* gain;
  double* focus_rms;
  double* S;
  uint8_t* focus_status;
  int32_t* focus_n_visible;
  double* focus_before;
  double* Q;
  int32_t* picks;
  double* pick_gain;
  double* pick_focus_rms;
  double* posterior;
  double* round_gain;
  double* round_focus_rms;
} mcba_guidance_result;
/* info [C]; views [n_views]: board views, or views of pixels (board < 0) scored like them; foci [C] or NULL (an entry with
 * camera < 0: no focus for that camera; otherwise camera == its index, board < 0).
 * Zero views launch nothing (picks -1, NaN).                                                                                  */
int32_t mcba_view_information(const mcba_camera_set* cams, const mcba_guidance_camera* info, int32_t n_boards, int32_t board_stride,
                              const int32_t* board_n, const double* board_points, double margin, double sigma2, int32_t n_views,
                              const mcba_guidance_view* views, const mcba_guidance_view* foci, int32_t n_picks, int32_t criterion,
                              const mcba_guidance_result* out);
/* timing of the last mcba_view_information call of this thread, milliseconds: [0] uploads, [1] k_view_schur and the scoring
 * rounds with their transfers (HIP events), [2] downloads, [3] the whole call; *n_views (or NULL) = views launched (foci too)  */
int32_t mcba_debug_view_information_ms(double* ms /*[4]*/, int64_t* n_views);

/* --- planning the next captures: views seen by several cameras ------------------------------------------------------- */
/* What a new view of a board that several cameras of a group see at once adds to their intrinsics AND their poses, and what it
 * does to the transfer uncertainty between them (csrc/mcba_rigview.h).  `cams` is the group; camera_poses
 * [C, 3, 4] rig -> camera.  The prior is Sigma = F F^T over the stored parameters of the group, F of rank r; per camera c
 * W [MCBA_RIG_COLUMNS, r] row-major = the rows of F in the device columns of c: fx fy cx cy k0..k13 (18, rows of coefficients the
 * camera lacks are 0) | the left perturbation (omega, tau) of camera_poses[c] (6) -- blockdiag(camera map, pose map) F[rows of c];
 * `unconstrained` != 0: a parameter of c that no residual constrains and that is not held.
 * A view is board `board` at the board-in-rig pose `pose` (3 x 4, row-major) in a new frame whose rig pose is free; camera c sees
 * the points that pass the visibility test of mcba_view_information and CONTRIBUTES with at least min_points (and one) of them.
 * A [r, r] = sigma2 A_v is the Schur complement of the frame pose in the Gram matrix of the contributing cameras' rows; against a
 * base B (I at first, + A_v of every pick): gain = (log det(B + A_v) - log det B) / 2 in nats.  The focus: the pixels of a grid of
 * camera `reference` at inv_distance, transferred into every member camera b (mcba_projection_uncertainty with reference = a);
 * Q = sum_b sum_pixels (J W_ab)^T (J W_ab) over the n_ok queries that are MCBA_UNC_OK, focus_rms = sqrt(trace((B + A_v)^-1 Q) / n_ok).
 * Greedy selection of n_picks views for the rig by `criterion` (MCBA_GUIDE_BY_*; ties: the lowest index; a view is picked once).
 * Refused, with nothing launched: r > MCBA_RIG_MAX_R (use a smaller camera group), n_views r^2 8 bytes above workspace_mb (pass
 * fewer candidates per call), boards != 0 (the board points are parameters of the calibration).  r = 0 or n_views = 0: nothing is
 * launched, every gain is 0.  Handle-less like mcba_view_information; same error convention, the caller owns every array.       */
#define MCBA_RIG_MAX_R 128
#define MCBA_RIG_COLUMNS 24
typedef struct mcba_rig_camera {
  int32_t unconstrained, reserved;
  const double* W;               /* [MCBA_RIG_COLUMNS, r] */
  double image_w, image_h;
} mcba_rig_camera;
typedef struct mcba_rig_view {
  int32_t board, min_points;
  double pose[12];
} mcba_rig_view;
typedef struct mcba_rig_focus {
  int32_t reference, n_members;
  const int32_t* members;        /* [n_members] the cameras b (the reference itself is skipped) */
  int32_t grid_w, grid_h;        /* pixel (ix, iy) = (u0 + ix du, v0 + iy dv) of the reference camera */
  double u0, v0, du, dv;
  double inv_distance;           /* >= 0, finite */
} mcba_rig_focus;
/* Outputs; rs = max(1, r) is the row stride of every matrix.  Per view: n_cameras (contributing), n_visible [n_views, C], status
 * MCBA_GUIDE_* (TOO_FEW: fewer than min_cameras contribute; UNCONSTRAINED: a contributing camera is; DEGENERATE: the frame pose is
 * not determined), gain and focus_rms against B = I (NaN unless OK), A [n_views, rs, rs] or NULL (0 unless OK).  The focus:
 * focus_status, focus_n (n_ok), focus_before, Q [rs, rs] (each or NULL).  picks [n_picks] (view, -1: none left), pick_gain
 * (conditional on the earlier picks), pick_focus_rms (after the pick); posterior [rs, rs] or NULL = B^-1 after the last pick;
 * round_gain / round_focus_rms [n_picks, n_views] or NULL.                                                                     */
typedef struct mcba_rig_result {
  int32_t* n_cameras;
  int32_t* n_visible;
  uint8_t* status;
  double* gain;
  double* focus_rms;
  double* A;
  uint8_t* focus_status;
  int32_t* focus_n;
  double* focus_before;
  double* Q;
  int32_t* picks;
  double* pick_gain;
  double* pick_focus_rms;
  double* posterior;
  double* round_gain;
  double* round_focus_rms;
} mcba_rig_result;
int32_t mcba_rig_view_information(const mcba_camera_set* cams, const double* camera_poses, int32_t r, const mcba_rig_camera* info,
                                  int32_t boards, int32_t n_boards, int32_t board_stride, const int32_t* board_n,
                                  const double* board_points, int32_t n_views, const mcba_rig_view* views, int32_t min_cameras,
                                  double margin, double sigma2, const mcba_rig_focus* focus, int32_t n_picks, int32_t criterion,
                                  int32_t workspace_mb, const mcba_rig_result* out);
/* timing of the last mcba_rig_view_information call of this thread, milliseconds: [0] uploads, [1] the kernels and the scoring
 * rounds with their transfers (HIP events), [2] downloads, [3] the whole call; *n_slots (or NULL) = (view, camera) slots launched */
int32_t mcba_debug_rig_view_information_ms(double* ms /*[4]*/, int64_t* n_slots);

/* --- using a calibration: 3-D uncertainty of triangulated points ---------------------------------------------------- */
/* The 3 x 3 covariance of the point a camera group triangulates, under the covariance of the calibration itself (cov_cal) and
 * under the pixel noise of the point alone (cov_noise = sigma2 H^-1, what mcba_triangulate reports) (csrc/mcba_recon.h, DESIGN.md
 * 3.20).  A job is a group of G = 2 .. MCBA_RECON_MAX_CAMERAS cameras of `cams` (slot s = cameras[s], no camera twice), a reference
 * (< 0: the point is expressed in the rig frame; a camera of the group: in that camera's frame, the gauge-free form in which a common
 * motion of all camera poses cancels), and per slot W [MCBA_RIG_COLUMNS, r] row-major in the columns of mcba_rig_camera.W: fx fy cx cy
 * k0..k13 | left perturbation (omega, tau) of camera_poses[c]; one r = 0 .. MCBA_RIG_MAX_R for the job, the image size and
 * `unconstrained` != 0: a parameter of the camera that no residual constrains and that is not held.  The job's n points follow those
 * of the job before it in `points` [n_total, 3] (rig frame); masks [n_total] or NULL: bit s set = slot s may be used.
 * Camera s is a VIEW of a point when the point lies in front of it, inside the monotone range of its model and projects into
 * [-margin, W + margin) x [-margin, H + margin); the other cameras drop out for that point.  With J_c the 2 x 3 derivative of the
 * pixel, P_c the 2 x 24 derivative by the columns of c and H = sum J_c^T J_c over the views: d X = -H^-1 sum_c J_c^T P_c W_c per
 * column of the factor -- exact at the noise-free pixels of X; for a point triangulated from noisy pixels the Gauss-Newton
 * approximation at the model-projected pixels.  cov_cal = sum over the columns of dX dX^T, positive semi-definite by construction;
 * r = 0 returns exactly 0.  camera_poses [C, 3, 4] rig -> camera.
 * Outputs: cov_cal, cov_noise [n_total, 6] upper triangles (xx xy xz yy yz zz), NaN unless OK; n_views [n_total]; views [n_total]
 * the mask of the slots that are views; status [n_total] MCBA_RECON_*.  Refused, with nothing launched: G outside 2 .. 8, r above
 * MCBA_RIG_MAX_R, a reference that is no camera of the group, a camera twice in a group, points that are not finite, an
 * unsupported camera family.  Zero points launch nothing.  Handle-less like mcba_projection_uncertainty; same error convention,
 * the caller owns every array.                                                                                                  */
#define MCBA_RECON_MAX_CAMERAS 8
#define MCBA_RECON_OK 0
#define MCBA_RECON_TOO_FEW 1        /* fewer than two views                                                                  */
#define MCBA_RECON_DEGENERATE 2     /* a Cholesky pivot of H at or below 1e-12 trace(H): the rays do not fix a point          */
#define MCBA_RECON_UNCONSTRAINED 3  /* a view, or the reference camera, is flagged unconstrained                              */
typedef struct mcba_recon_job {
  int32_t G;                                     /* cameras of the group */
  int32_t cameras[MCBA_RECON_MAX_CAMERAS];       /* slot -> camera of `cams` */
  int32_t reference;                             /* a camera of the group, or < 0: the rig frame */
  int32_t r;                                     /* columns of every W */
  const double* W[MCBA_RECON_MAX_CAMERAS];       /* [MCBA_RIG_COLUMNS, r] per slot */
  uint8_t unconstrained[MCBA_RECON_MAX_CAMERAS];
  double image_w[MCBA_RECON_MAX_CAMERAS], image_h[MCBA_RECON_MAX_CAMERAS];
  int64_t n;                                     /* points of this job */
} mcba_recon_job;
int32_t mcba_reconstruction_uncertainty(const mcba_camera_set* cams, const double* camera_poses, int32_t n_jobs,
                                        const mcba_recon_job* jobs, const double* points, const uint64_t* masks, double sigma2,
                                        double margin, double* cov_cal, double* cov_noise, int32_t* n_views, uint64_t* views,
                                        uint8_t* status);
/* timing of the last mcba_reconstruction_uncertainty call of this thread, milliseconds: [0] uploads, [1] kernel (HIP events around
 * the launch), [2] downloads, [3] the whole call; *n_points (or NULL) = points launched                                        */
int32_t mcba_debug_reconstruction_uncertainty_ms(double* ms /*[4]*/, int64_t* n_points);

/* --- using a calibration: uncertainty of measured lengths (covariance between triangulated points) --------------------- */
/* The covariance of the DIFFERENCE of two triangulated points and of the length between them (csrc/mcba_recon.h).
 * The calibration's error is common to all points of a scene: it moves both ends of a short bar by nearly the same vector, so the
 * error of a length is far below sqrt(var_a + var_b) of the per-point cov_cal.  The arguments of mcba_reconstruction_uncertainty,
 * and per job n_pairs[j] pairs (a, b) of indices into the job's own points: pairs [n_pairs_total, 2], those of a job after those of
 * the job before it.  With z_j(X) the response of mcba_reconstruction_uncertainty to column j of the factor:
 *   cov_diff_cal   [K, 6]  sum_j d_j d_j^T, d_j = z_j(X_a) - z_j(X_b): subtracted per column before squaring, positive semi-definite
 *                          by construction (never formed as C_a + C_b - C_ab - C_ab^T); exactly 0 for a == b and for r = 0
 *   cross_cal      [K, 9]  sum_j z_j(X_a) z_j(X_b)^T, row-major 3 x 3: cross(b, a) = cross(a, b)^T, cross(a, a) = cov_cal of a; from
 *                          these and cov_cal a caller assembles the joint covariance of a small set of points
 *   cov_diff_noise [K, 6]  sigma2 (H_a^-1 + H_b^-1) (the pixel noise of two points is independent); exactly 0 for a == b
 *   length         [K]     |X_a - X_b|
 *   length_var_cal, length_var_noise [K]  u^T cov_diff_* u, u the unit vector between the points; NaN where length == 0.  To first
 *                          order they do not depend on the reference or the rig frame (a common motion of the output frame moves
 *                          both ends rigidly, and its rotation term is perpendicular to u)
 *   views_a, views_b [K]   the view masks of the two ends (each end keeps its own views, masks and margin as for a single point)
 *   status         [K]     MCBA_RECON_*: that of a unless it is OK, then that of b.  Unless OK every output is NaN except length and
 *                          the view masks.
 * Any output pointer may be NULL.  Refused, with nothing launched: what mcba_reconstruction_uncertainty refuses, a negative
 * n_pairs[j], an index of `pairs` outside [0, n) of its job.  Zero pairs launch nothing.                                          */
int32_t mcba_reconstruction_pairs(const mcba_camera_set* cams, const double* camera_poses, int32_t n_jobs, const mcba_recon_job* jobs,
                                  const double* points, const uint64_t* masks, const int64_t* n_pairs, const int64_t* pairs,
                                  double sigma2, double margin, double* cov_diff_cal, double* cross_cal, double* cov_diff_noise,
                                  double* length, double* length_var_cal, double* length_var_noise, uint64_t* views_a,
                                  uint64_t* views_b, uint8_t* status);
/* timing of the last mcba_reconstruction_pairs call of this thread, milliseconds: [0] uploads, [1] kernel (HIP events around the
 * launch), [2] downloads, [3] the whole call; *n_pairs (or NULL) = pairs launched                                                */
int32_t mcba_debug_reconstruction_pairs_ms(double* ms /*[4]*/, int64_t* n_pairs);

/* --- residual field: the systematic part of the reprojection error ------------------------ */
/* Gram matrices of a smooth vector field fitted to the residuals as a function of the OBSERVED pixel.  Not part of the reference.
 *   - model: per camera a tensor-product uniform cubic B-spline field e(u, v) in R^2 over [0, W] x [0, H] with nx x ny intervals:
 *     K = (nx + 3)(ny + 3) control points, control point (a along y, b along x) in column a (nx + 3) + b, both components on the
 *     same grid.  A pixel in interval (ix, iy) = floor(u nx / W), floor(v ny / H) (the far edge in the last interval, fraction 1)
 *     has 16 non-zero weights wy[a] wx[b] >= 0 on the control points (iy + a, ix + b), a, b = 0 .. 3, which sum to 1; wx, wy are
 *     the cubic B-spline weights ((1 - t)^3, 3 t^3 - 6 t^2 + 4, -3 t^3 + 3 t^2 + 3 t + 1, t^3) / 6 of the fraction t.
 *   - row of an observation: [ b(u, v) (K entries) | r_x | r_y ],  r = projected - observed (the residual of mcba_residuals /
 *     mcba_observation_covariance; rolling shutter: scan time from the observed row, as in mcba_project), NC = K + 2 columns.
 *   - rows: every slot (c, f, b, p) of the mask mcba_reprojection_error returns as `valid` -- only the inliers among them if
 *     inliers_only != 0 -- whose observed pixel lies in the closed image rectangle; the others of these slots are counted in
 *     outside[c].  Weights are 0 / 1.
 *   - gram [C][n_folds][NC][NC]: the sum of row^T row over the rows of camera c in the frames f with f mod n_folds == fold: B^T B
 *     (K x K), B^T r_x, B^T r_y (columns K, K + 1), r_x^T r_x, r_x^T r_y, r_y^T r_y; full symmetric storage, the two triangles
 *     equal to the bit.  A fold without frames or rows is exactly zero.  count [C][n_folds]: its rows.  Summed in a fixed order:
 *     two calls on one handle return the same bytes.
 *   - coverage [C][2][cov_h][cov_w] (or NULL; 1 <= cov_w cov_h <= 512): valid slots inside the image per cell (ix, iy) =
 *     floor(u cov_w / W), floor(v cov_h / H) of the observed pixel, plane 0 the inliers, plane 1 the valid slots that are not
 *     (whatever inliers_only says).
 *   - refused with a message: a frame-sharded handle; nx, ny or n_folds below 1; n_folds > 16; NC > 64 (nx = 6, ny = 4 has
 *     K = 63); an image size that is not positive.  Handles with the `boards` block optimised are fine.
 * One pass over the observation table on the device (csrc/mcba_residual_field_kernels.h): the table evaluation and k_residual of
 * mcba_project, then one wavefront per (camera, fold, frame chunk) accumulating the upper 16 x 16 tiles by FP64 MFMA and a fold of
 * the chunk partials.  Only the blocks, the counts and the maps leave the device.  x is not changed, nor is any other state
 * a later call reads.                                                                                                            */
int32_t mcba_residual_gram(mcba_handle h, const double* x, const int32_t* image_size /*[C][2] W,H*/,
                           int32_t nx, int32_t ny, int32_t n_folds, int32_t inliers_only,
                           double* gram      /*[C][n_folds][NC][NC], full symmetric*/,
                           int64_t* count    /*[C][n_folds] rows that entered*/,
                           int64_t* outside  /*[C] slots skipped: observed pixel outside the image*/,
                           int32_t cov_w, int32_t cov_h,
                           int32_t* coverage /*[C][2][cov_h][cov_w]: inliers | valid but rejected; may be NULL*/);
/* timing of the last mcba_residual_gram call of this thread, milliseconds: [0] the projection pass (table evaluation + k_residual),
 * [1] k_residual_gram, [2] k_residual_gram_fold (HIP events), [3] the whole call; *n_rows (or NULL) = rows that entered           */
int32_t mcba_debug_residual_gram_ms(double* ms /*[4]*/, int64_t* n_rows);

/* --- applying the residual field: corrected points, maps and images ------------------------------------------------- */
/* The fitted field as a warp of the image plane (csrc/mcba_warp.h).  Definitions -- they decide every sign:
 *   - field: e_c(u, v) = sum_k b_k(u, v) coef[c][k][:], grid nx x ny over the image (W_c, H_c), control point (a, b) (a along y, b
 *     along x) in column a (nx + 3) + b -- the coefficients of the fit of mcba_residual_gram's rows, r = projected - observed as a
 *     function of the observed pixel.  Outside the closed image rectangle the field is that of the pixel clamped to it.
 *   - forward warp, raw -> corrected: w(p) = p + e(p): the corrected observation is what the parametric model predicts.
 *   - inverse warp, corrected -> raw: p + e(p) = q by Newton (analytic Jacobian I + De, start q - e(q), stop at max |dp| <= 1e-11 px
 *     or a step that no longer moves p, at most 50 steps): status MCBA_UNDISTORT_OK / MCBA_UNDISTORT_NOT_CONVERGED (NaN).  A
 *     non-finite input gives NaN and NOT_CONVERGED in both directions.
 *   - fold bound: L = max over the two components of max |D_x coef| nx / W + max |D_y coef| ny / H (D: first difference of
 *     neighbouring control values) bounds the infinity norm of De.  Below 0.2 Newton contracts by 2 L / (1 - L) <= 0.5 a step from
 *     any start, so a finite input always converges; a field set with L >= 0.2 is refused ("the field folds the image").
 *   - corrected camera: project_corrected(X) = w^-1(pi(X)), undistort_corrected(p) = pi^-1(w(p)); a corrected map holds
 *     w^-1(pi(iR [u v 1])) of every destination pixel, FP64 throughout and rounded once to float32.
 * Handle-less, the error convention of the undistortion entries.  Refused with a message: a field set whose C differs from the
 * camera set's; nx or ny below 1; (nx + 3)(ny + 3) > 62; an image size that is not positive; a coefficient that is not finite;
 * L >= 0.2; a camera index out of range; the image-format refusals of mcba_undistort_images.                                     */
typedef struct mcba_field_set {
  int32_t C;                      /* cameras                                                                            */
  const int32_t* image_size;      /* [C][2] W, H                                                                        */
  int32_t nx, ny;                 /* intervals of the spline grid, the same for every camera                            */
  const double* coef;             /* [C][(nx + 3)(ny + 3)][2]                                                           */
} mcba_field_set;
/* out [n,2] = w(uv) (inverse == 0) or w^-1(uv) (inverse != 0) through the field of camera_of_point[i] (NULL = camera 0); status [n]
 * MCBA_UNDISTORT_*, or NULL.  A whole [C,F,B,P,2] observation table is one call over its flat list of slots.  n == 0 launches
 * nothing.                                                                                                              */
int32_t mcba_warp_points(const mcba_field_set* f, int64_t n, const int32_t* camera_of_point, int32_t inverse, const double* uv,
                         double* out, uint8_t* status);
/* mcba_undistort_maps of the corrected cameras: maps [C,height,width,2].  With an all-zero field the bytes of mcba_undistort_maps. */
int32_t mcba_undistort_maps_corrected(const mcba_camera_set* cams, const mcba_field_set* f, const double* R, const double* P,
                                      int32_t width, int32_t height, float* maps);
/* mcba_undistort_images of the corrected cameras: the corrected maps are made in device memory the call owns and feed the map-fed
 * remap kernel on the same stream -- byte for byte mcba_remap through mcba_undistort_maps_corrected; no map leaves the device.  */
int32_t mcba_undistort_images_corrected(const mcba_camera_set* cams, const mcba_field_set* f, const double* R, const double* P,
                                        const void* src, int32_t N, int32_t Hs, int32_t Ws, int32_t channels, int32_t dtype,
                                        const int32_t* camera_of_image, int32_t Hd, int32_t Wd, double border, void* dst);
/* timing of the last corrected call of this thread, milliseconds: [0] uploads, [1] the kernels (HIP events), [2] downloads, [3] the
 * whole call; *n (or NULL) = points or pixels written                                                                   */
int32_t mcba_debug_warp_ms(double* ms /*[4]*/, int64_t* n);

/* --- before the detection table: sub-pixel refinement of detected corners ----------------------------------------------- */
/* board.subpix_corners (board/common.py:50-54: cv2.cornerSubPix) for n corners in N grey images [N,H,W] of one size in one launch
 * (csrc/mcba_subpix.h).  Pixel centres are at integer coordinates.  One iteration at the position c: bilinear
 * samples S(i, j) of the image at c + (j, i) with one fractional offset and a replicate border; gx = S(i, j+1) - S(i, j-1),
 * gy = S(i+1, j) - S(i-1, j) on the window |i| <= win_y, |j| <= win_x; weight m = e^-(i/win_y)^2 e^-(j/win_x)^2, zero where
 * |i| <= zero_y and |j| <= zero_x if zero_x, zero_y >= 0 and the zone is smaller than the window on both axes (otherwise no zone);
 * a = sum m gx^2, b = sum m gx gy, d = sum m gy^2, p = sum m (gx^2 j + gx gy i), q = sum m (gx gy j + gy^2 i); |a d - b^2| <=
 * DBL_EPSILON^2 stops and keeps c; else c <- c + (d p - b q, a q - b p) / (a d - b^2).  The iteration stops when c leaves
 * [0, W) x [0, H), when the squared step is <= eps^2, or after max_iter iterations; a result further from the start than win_x in x
 * or win_y in y is given up for the start.  FP64 throughout (cv2 holds the patch and the result in float32: parity is at formula
 * level).  refined [n,2] is the position the stopping rule leaves; status [n] MCBA_SUBPIX_*; iterations [n] (or NULL) the evaluations
 * of the sums; quality [n] (or NULL) the smaller eigenvalue of [[a, b], [b, d]] / sum m at the last evaluation: the mean squared
 * gradient along the weakest direction in grey levels squared, NaN when nothing was evaluated.  dtype MCBA_PIXEL_*.
 * Handle-less, the error convention of the undistortion entries.  Refused with a message: a half window outside 1 .. 15, max_iter
 * outside 1 .. 100, eps negative or not finite, an unknown pixel type, H or W below 2, an image index outside 0 .. N - 1 (the
 * message names the first such corner).  n == 0 launches nothing.                                                            */
#define MCBA_SUBPIX_OK 0           /* stopped on eps                                                                      */
#define MCBA_SUBPIX_MAX_ITER 1     /* max_iter iterations without reaching eps                                            */
#define MCBA_SUBPIX_SINGULAR 2     /* no gradient structure in the window: the position before that iteration             */
#define MCBA_SUBPIX_LEFT_IMAGE 3   /* the iteration left the image                                                        */
#define MCBA_SUBPIX_REVERTED 4     /* moved further than the window: the start is returned (overrides the others)         */
#define MCBA_SUBPIX_INVALID 5      /* start not finite or outside the image: returned unchanged, nothing read             */
int32_t mcba_refine_corners(const void* images, int32_t N, int32_t H, int32_t W, int32_t dtype, int32_t n,
                            const double* corners /*[n][2]*/, const int32_t* image_of_corner /*[n] or NULL: image 0*/,
                            int32_t win_x, int32_t win_y, int32_t zero_x, int32_t zero_y, int32_t max_iter, double eps,
                            double* refined /*[n][2]*/, uint8_t* status /*[n]*/, int32_t* iterations /*[n] or NULL*/,
                            double* quality /*[n] or NULL*/);
/* timing of the last mcba_refine_corners call of this thread, milliseconds: [0] uploads, [1] k_refine_corners (HIP events), [2]
 * downloads, [3] the whole call; *n (or NULL) = corners                                                                   */
int32_t mcba_debug_subpix_ms(double* ms /*[4]*/, int64_t* n);

/* --- solve -------------------------------------------------------------------------------------------------- */
/* Trust-region least squares: replaces scipy.optimize.least_squares(method='trf', x_scale='jac', jac_sparsity=S,
 * loss, f_scale, ftol, max_nfev) at calibration.py:209-210.  x is updated in place to `res.x`.                 */
int32_t mcba_solve(mcba_handle h, double* x_inout, const mcba_options* opt, mcba_result* result);

/* Collectives issued by a frame-sharded handle since the last reset (observability of SURVEY 8(e)): number of
 * all-reduce calls, doubles moved, and the element counts of the first `cap` calls in issue order (negative = max
 * reduction).  Any of the output pointers may be NULL.                                                           */
int32_t mcba_allreduce_stats(mcba_handle h, int32_t reset, int64_t* calls, int64_t* doubles, int64_t* sizes, int32_t cap,
                             int32_t* n_sizes);

/* --- measurement ------------------------------------------------------------------------------------------- */
/* Run the fused linearisation `repeats` times at x and return the average GPU time per pass in milliseconds
 * measured with HIP events on the handle's stream (bench.py roofline leg).                                     */
int32_t mcba_time_linearize(mcba_handle h, const double* x, const mcba_options* opt, int32_t repeats,
                            double* avg_ms);
int32_t mcba_time_residuals(mcba_handle h, const double* x, int32_t repeats, double* avg_ms);
/* ... and of the two kernels of one LSMR iteration of the default solver (tr_solver = MCBA_TR_LSMR): ms[0] = the product kernel
 * (J_h v and J_h^T u from one evaluation of the analytic rows), ms[1] = the gather; bench.py: parity_route.roofline             */
int32_t mcba_time_lsmr_iteration(mcba_handle h, const double* x, int32_t repeats, double* ms /*[2]*/);

#ifdef __cplusplus
}
#endif
#endif /* MCBA_H */
