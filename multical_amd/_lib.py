"""ctypes binding of the C ABI in include/mcba.h (libmcba.so, built by multical_amd.build).

The library is HIP-only.  Importing this module never falls back to a CPU implementation: if the shared object
is missing, `load()` raises with the build command; if no gfx950 device is present, `mcba_create` fails.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MCBA_LIB_PATH") or os.path.join(HERE, "_build", "libmcba.so")   # (override: kernel experiments)

MCBA_VERSION = 3
MOTION_STATIC, MOTION_ROLLING, MOTION_HAND_EYE = 0, 1, 2
CAMERA_PINHOLE, CAMERA_FISHEYE = 0, 1
LOSSES = dict(linear=0, soft_l1=1, huber=2, cauchy=3, arctan=4)
TR_SOLVERS = dict(exact=0, lsmr=1)     # mcba_options.tr_solver (MCBA_TR_*)
OPT_BITS = dict(camera_poses=1, board_poses=2, motion=4, cameras=8, boards=16)
PARAM_ORDER = ["camera_poses", "board_poses", "motion", "cameras", "boards"]   # calibration.py:146-153

c_double_p = C.POINTER(C.c_double)
c_uint8_p = C.POINTER(C.c_uint8)
c_int32_p = C.POINTER(C.c_int32)


class Problem(C.Structure):
  _fields_ = [
    ("version", C.c_int32), ("n_cameras", C.c_int32), ("n_frames", C.c_int32), ("n_boards", C.c_int32),
    ("n_points", C.c_int32),
    ("points", c_double_p), ("point_valid", c_uint8_p), ("inlier_mask", c_uint8_p),
    ("board_sizes", c_int32_p), ("camera_valid", c_uint8_p), ("frame_valid", c_uint8_p), ("board_valid", c_uint8_p),
    ("motion", C.c_int32), ("camera_model", C.c_int32), ("n_dist", C.c_int32),
    ("image_heights", c_double_p), ("fix_aspect", c_uint8_p), ("base_wrt_gripper", c_double_p),
    ("optimize", C.c_uint32), ("x_full", c_double_p),
    ("frame_begin", C.c_int32), ("frame_end", C.c_int32),
    ("camera_n_dist", c_int32_p),
    ("camera_fisheye", c_uint8_p),
    ("points_f32", C.POINTER(C.c_float)),
  ]


class Options(C.Structure):
  _fields_ = [("ftol", C.c_double), ("xtol", C.c_double), ("gtol", C.c_double), ("max_nfev", C.c_int32),
              ("loss", C.c_int32), ("f_scale", C.c_double), ("verbose", C.c_int32), ("tr_solver", C.c_int32)]


class Result(C.Structure):
  _fields_ = [("cost", C.c_double), ("initial_cost", C.c_double), ("optimality", C.c_double), ("nfev", C.c_int32),
              ("njev", C.c_int32), ("status", C.c_int32), ("iterations", C.c_int32), ("solve_seconds", C.c_double),
              ("linearize_seconds", C.c_double)]


class RoundReport(C.Structure):   # mcba_round_report
  _fields_ = [("rms_all", C.c_double), ("rms_inliers", C.c_double), ("n_all", C.c_int64), ("n_inliers", C.c_int64),
              ("quantiles", C.c_double * 5), ("f_scale", C.c_double), ("threshold", C.c_double), ("n_kept", C.c_int64),
              ("n_valid", C.c_int64), ("solve", Result)]


class ViewPoseProblem(C.Structure):   # mcba_view_pose_problem
  _fields_ = [("C", C.c_int32), ("F", C.c_int32), ("B", C.c_int32), ("P", C.c_int32),
              ("points", c_double_p), ("valid", c_uint8_p), ("board_points", c_double_p), ("board_sizes", c_int32_p),
              ("cameras", c_double_p), ("n_dist", C.c_int32), ("camera_n_dist", c_int32_p), ("is_fisheye", c_uint8_p),
              ("fix_aspect", c_uint8_p), ("view_mask", c_uint8_p), ("init_poses", c_double_p),
              ("max_iterations", C.c_int32), ("lm_iterations", c_int32_p)]


class HandEyeProblem(C.Structure):   # mcba_hand_eye_problem
  _fields_ = [("F", C.c_int32), ("n_a", C.c_int64), ("n_b", C.c_int64), ("table_a", c_double_p), ("valid_a", c_uint8_p),
              ("table_b", c_double_p), ("valid_b", c_uint8_p), ("n_problems", C.c_int32), ("index_a", c_int32_p),
              ("index_b", c_int32_p), ("invert_inputs", C.c_int32)]


class IntrinsicProblem(C.Structure):   # mcba_intrinsic_problem
  _fields_ = [("C", C.c_int32), ("F", C.c_int32), ("B", C.c_int32), ("P", C.c_int32),
              ("points", c_double_p), ("valid", c_uint8_p), ("board_points", c_double_p), ("board_sizes", c_int32_p),
              ("image_sizes", c_double_p), ("n_dist", C.c_int32), ("camera_n_dist", c_int32_p), ("is_fisheye", c_uint8_p),
              ("fix_aspect", c_uint8_p), ("free_dist", c_uint8_p), ("view_mask", c_uint8_p), ("init_cameras", c_double_p),
              ("init_poses", c_double_p), ("max_iterations", C.c_int32), ("lm_iterations", c_int32_p)]


class CameraSet(C.Structure):   # mcba_camera_set
  _fields_ = [("C", C.c_int32), ("cameras", c_double_p), ("n_dist", C.c_int32), ("camera_n_dist", c_int32_p),
              ("is_fisheye", c_uint8_p)]


class FieldSet(C.Structure):   # mcba_field_set
  _fields_ = [("C", C.c_int32), ("image_size", c_int32_p), ("nx", C.c_int32), ("ny", C.c_int32), ("coef", c_double_p)]


class TriangulateProblem(C.Structure):   # mcba_triangulate_problem
  _fields_ = [("cams", CameraSet), ("F", C.c_int32), ("M", C.c_int64), ("views", c_double_p), ("views_end", c_double_p),
              ("image_heights", c_double_p), ("view_valid", c_uint8_p), ("points", c_double_p), ("valid", c_uint8_p),
              ("sigma_px", C.c_double), ("max_iterations", C.c_int32)]


class RigPoseProblem(C.Structure):   # mcba_rig_pose_problem
  _fields_ = [("cams", CameraSet), ("F", C.c_int32), ("B", C.c_int32), ("P", C.c_int32), ("camera_poses", c_double_p),
              ("board_poses", c_double_p), ("board_points", c_double_p), ("board_valid", c_uint8_p), ("points", c_double_p),
              ("valid", c_uint8_p), ("init", c_double_p), ("init_end", c_double_p), ("rolling", C.c_int32),
              ("image_heights", c_double_p), ("sigma_px", C.c_double), ("max_iterations", C.c_int32)]


class StereoProblem(C.Structure):   # mcba_stereo_problem
  _fields_ = [("cams", CameraSet), ("F", C.c_int32), ("B", C.c_int32), ("P", C.c_int32), ("board_points", c_double_p),
              ("board_valid", c_uint8_p), ("points", c_double_p), ("valid", c_uint8_p), ("view_poses", c_double_p),
              ("view_valid", c_uint8_p), ("n_pairs", C.c_int32), ("pairs", c_int32_p), ("min_common", C.c_int32),
              ("max_iterations", C.c_int32), ("sigma_px", C.c_double)]


class UncertaintyJob(C.Structure):   # mcba_uncertainty_job
  _fields_ = [("camera", C.c_int32), ("reference", C.c_int32), ("inv_distance", C.c_double), ("K", C.c_int32), ("r", C.c_int32),
              ("W", c_double_p), ("unconstrained", c_uint8_p), ("grid_w", C.c_int32), ("grid_h", C.c_int32), ("u0", C.c_double),
              ("v0", C.c_double), ("du", C.c_double), ("dv", C.c_double), ("n", C.c_int64), ("uv", c_double_p)]


class ProjDiffJob(C.Structure):   # mcba_projdiff_job
  _fields_ = [("camera", C.c_int32), ("reference", C.c_int32), ("inv_distance", C.c_double), ("fit", C.c_int32),
              ("fit_grid_w", C.c_int32), ("fit_grid_h", C.c_int32), ("fit_u0", C.c_double), ("fit_v0", C.c_double),
              ("fit_du", C.c_double), ("fit_dv", C.c_double), ("fit_n", C.c_int64), ("fit_uv", c_double_p), ("focus_u", C.c_double),
              ("focus_v", C.c_double), ("focus_radius", C.c_double), ("grid_w", C.c_int32), ("grid_h", C.c_int32), ("u0", C.c_double),
              ("v0", C.c_double), ("du", C.c_double), ("dv", C.c_double), ("n", C.c_int64), ("uv", c_double_p)]


class GuidanceCamera(C.Structure):   # mcba_guidance_camera
  _fields_ = [("r", C.c_int32), ("unconstrained", C.c_int32), ("W", c_double_p), ("image_w", C.c_double), ("image_h", C.c_double)]


class GuidanceView(C.Structure):   # mcba_guidance_view
  _fields_ = [("camera", C.c_int32), ("n_nuisance", C.c_int32), ("min_points", C.c_int32), ("board", C.c_int32),
              ("pose", C.c_double * 12), ("inv_distance", C.c_double), ("grid_w", C.c_int32), ("grid_h", C.c_int32), ("u0", C.c_double),
              ("v0", C.c_double), ("du", C.c_double), ("dv", C.c_double), ("n", C.c_int64), ("uv", c_double_p)]


class GuidanceResult(C.Structure):   # mcba_guidance_result
  _fields_ = [("n_visible", C.POINTER(C.c_int32)), ("status", c_uint8_p), ("gain", c_double_p), ("focus_rms", c_double_p),
              ("S", c_double_p), ("focus_status", c_uint8_p), ("focus_n_visible", C.POINTER(C.c_int32)), ("focus_before", c_double_p),
              ("Q", c_double_p), ("picks", C.POINTER(C.c_int32)), ("pick_gain", c_double_p), ("pick_focus_rms", c_double_p),
              ("posterior", c_double_p), ("round_gain", c_double_p), ("round_focus_rms", c_double_p)]


TRI_OK, TRI_TOO_FEW, TRI_DEGENERATE, TRI_NOT_CONVERGED, TRI_BEHIND = 0, 1, 2, 3, 4   # MCBA_TRI_*
TRI_MAX_CAMERAS = 64                                  # MCBA_TRI_MAX_CAMERAS
RIG_OK, RIG_TOO_FEW, RIG_DEGENERATE, RIG_NOT_CONVERGED, RIG_BEHIND = 0, 1, 2, 3, 4   # MCBA_RIG_*
RIG_MAX_CAMERAS = 64                                  # MCBA_RIG_MAX_CAMERAS
STEREO_OK, STEREO_TOO_FEW, STEREO_DEGENERATE, STEREO_NOT_CONVERGED = 0, 1, 2, 3   # MCBA_STEREO_*
UNC_OK, UNC_NOT_CONVERGED, UNC_BEHIND, UNC_UNCONSTRAINED = 0, 1, 2, 3   # MCBA_UNC_*
UNC_MAX_K = 48                                        # MCBA_UNC_MAX_K
PDIFF_OK, PDIFF_NOT_CONVERGED, PDIFF_BEHIND, PDIFF_NO_FIT = 0, 1, 2, 3   # MCBA_PDIFF_*
class RigCamera(C.Structure):   # mcba_rig_camera
  _fields_ = [("unconstrained", C.c_int32), ("reserved", C.c_int32), ("W", c_double_p), ("image_w", C.c_double), ("image_h", C.c_double)]


class ReconJob(C.Structure):   # mcba_recon_job
  _fields_ = [("G", C.c_int32), ("cameras", C.c_int32 * 8), ("reference", C.c_int32), ("r", C.c_int32), ("W", c_double_p * 8),
              ("unconstrained", C.c_uint8 * 8), ("image_w", C.c_double * 8), ("image_h", C.c_double * 8), ("n", C.c_int64)]


class RigView(C.Structure):   # mcba_rig_view
  _fields_ = [("board", C.c_int32), ("min_points", C.c_int32), ("pose", C.c_double * 12)]


class RigFocus(C.Structure):   # mcba_rig_focus
  _fields_ = [("reference", C.c_int32), ("n_members", C.c_int32), ("members", C.POINTER(C.c_int32)), ("grid_w", C.c_int32),
              ("grid_h", C.c_int32), ("u0", C.c_double), ("v0", C.c_double), ("du", C.c_double), ("dv", C.c_double),
              ("inv_distance", C.c_double)]


class RigResult(C.Structure):   # mcba_rig_result
  _fields_ = [("n_cameras", C.POINTER(C.c_int32)), ("n_visible", C.POINTER(C.c_int32)), ("status", c_uint8_p), ("gain", c_double_p),
              ("focus_rms", c_double_p), ("A", c_double_p), ("focus_status", c_uint8_p), ("focus_n", C.POINTER(C.c_int32)),
              ("focus_before", c_double_p), ("Q", c_double_p), ("picks", C.POINTER(C.c_int32)), ("pick_gain", c_double_p),
              ("pick_focus_rms", c_double_p), ("posterior", c_double_p), ("round_gain", c_double_p), ("round_focus_rms", c_double_p)]


PDIFF_FIT_OK, PDIFF_FIT_TOO_FEW, PDIFF_FIT_NOT_CONVERGED, PDIFF_FIT_DEGENERATE = 0, 1, 2, 3   # MCBA_PDIFF_FIT_*
PDIFF_MODE_NONE, PDIFF_MODE_ROTATION, PDIFF_MODE_RIGID = 0, 1, 2   # MCBA_PDIFF_MODE_*
PDIFF_MAX_FIT = 65536                                 # MCBA_PDIFF_MAX_FIT
GUIDE_OK, GUIDE_TOO_FEW, GUIDE_DEGENERATE, GUIDE_UNCONSTRAINED = 0, 1, 2, 3   # MCBA_GUIDE_*
GUIDE_BY_FOCUS, GUIDE_BY_GAIN = 0, 1                  # MCBA_GUIDE_BY_*
GUIDE_MAX_R = 18                                      # MCBA_GUIDE_MAX_R
RIG_MAX_R, RIG_COLUMNS = 128, 24                      # MCBA_RIG_MAX_R, MCBA_RIG_COLUMNS
RECON_OK, RECON_TOO_FEW, RECON_DEGENERATE, RECON_UNCONSTRAINED = 0, 1, 2, 3   # MCBA_RECON_*
RECON_MAX_CAMERAS = 8                                 # MCBA_RECON_MAX_CAMERAS
PIXEL_U8, PIXEL_F32 = 0, 1                            # MCBA_PIXEL_*
UNDISTORT_OK, UNDISTORT_NOT_CONVERGED = 0, 1          # MCBA_UNDISTORT_*
SUBPIX_OK, SUBPIX_MAX_ITER, SUBPIX_SINGULAR, SUBPIX_LEFT_IMAGE, SUBPIX_REVERTED, SUBPIX_INVALID = 0, 1, 2, 3, 4, 5   # MCBA_SUBPIX_*

LOG_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p)

# every symbol include/mcba.h declares: (name, restype, argtypes)
H = C.c_void_p
SYMBOLS = [
  ("mcba_last_error", C.c_char_p, []),
  ("mcba_full_size", C.c_int32, [C.POINTER(Problem), C.POINTER(C.c_int64)]),
  ("mcba_create", C.c_int32, [C.POINTER(Problem), C.c_void_p, C.POINTER(H)]),
  ("mcba_destroy", C.c_int32, [H]),
  ("mcba_release_cached_memory", C.c_int32, []),
  ("mcba_device_info", C.c_int32, [H, C.c_char_p, C.c_size_t]),
  ("mcba_num_params", C.c_int32, [H, C.POINTER(C.c_int64)]),
  ("mcba_num_residuals", C.c_int32, [H, C.POINTER(C.c_int64)]),
  ("mcba_set_inliers", C.c_int32, [H, c_uint8_p]),
  ("mcba_set_allreduce", C.c_int32, [H, ALLREDUCE_FN, C.c_void_p]),
  ("mcba_set_shard_root", C.c_int32, [H, C.c_int32]),
  ("mcba_set_shard_rank", C.c_int32, [H, C.c_int32, C.c_int32]),
  ("mcba_allreduce_stats", C.c_int32, [H, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                       C.c_int32, C.POINTER(C.c_int32)]),
  ("mcba_set_log", C.c_int32, [H, LOG_FN, C.c_void_p]),
  ("mcba_residuals", C.c_int32, [H, c_double_p, c_double_p]),
  ("mcba_jacobian", C.c_int32, [H, c_double_p, c_int32_p, c_double_p, c_int32_p]),
  ("mcba_reprojection_error", C.c_int32, [H, c_double_p, c_double_p, c_uint8_p]),
  ("mcba_project", C.c_int32, [H, c_double_p, c_double_p]),
  ("mcba_project_model", C.c_int32, [H, c_double_p, C.c_int32, c_double_p]),
  ("mcba_align_poses_robust", C.c_int32, [C.c_int32, C.POINTER(C.c_int64), c_double_p, c_double_p, c_uint8_p, C.c_double,
                                          C.c_int32, c_double_p, c_uint8_p, c_uint8_p]),
  ("mcba_align_poses_indexed", C.c_int32, [C.c_int32, C.POINTER(C.c_int64), c_double_p, C.c_int64, c_int32_p, c_double_p, C.c_int64,
                                           c_int32_p, c_uint8_p, C.c_double, C.c_int32, c_double_p, c_uint8_p, c_uint8_p]),
  ("mcba_view_poses", C.c_int32, [C.POINTER(ViewPoseProblem), c_double_p, c_double_p, c_int32_p, c_uint8_p]),
  ("mcba_debug_view_poses_ms", C.c_int32, [c_double_p, C.POINTER(C.c_int64)]),
  ("mcba_calibrate_intrinsics", C.c_int32, [C.POINTER(IntrinsicProblem), c_double_p, c_double_p, c_double_p, c_int32_p, c_uint8_p,
                                            c_uint8_p]),
  ("mcba_debug_calibrate_intrinsics_ms", C.c_int32, [c_double_p, C.POINTER(C.c_int64)]),
  ("mcba_hand_eye", C.c_int32, [C.POINTER(HandEyeProblem), c_double_p, c_double_p, c_int32_p, c_uint8_p, c_double_p]),
  ("mcba_debug_hand_eye_ms", C.c_int32, [c_double_p, C.POINTER(C.c_int64)]),
  ("mcba_project_points", C.c_int32, [C.POINTER(CameraSet), C.c_int64, c_int32_p, c_double_p, c_double_p]),
  ("mcba_undistort_points", C.c_int32, [C.POINTER(CameraSet), C.c_int64, c_int32_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                        c_uint8_p]),
  ("mcba_undistort_maps", C.c_int32, [C.POINTER(CameraSet), c_double_p, c_double_p, C.c_int32, C.c_int32, C.POINTER(C.c_float)]),
  ("mcba_remap", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_int32,
                             C.c_int32, C.c_int32, c_int32_p, C.c_double, C.c_void_p]),
  ("mcba_undistort_images", C.c_int32, [C.POINTER(CameraSet), c_double_p, c_double_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_int32, c_int32_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p]),
  ("mcba_debug_undistort_ms", C.c_int32, [c_double_p, C.POINTER(C.c_int64)]),
  ("mcba_triangulate", C.c_int32, [C.POINTER(TriangulateProblem), c_double_p, c_double_p, c_double_p, c_double_p, c_int32_p,
                                   c_uint8_p]),
  ("mcba_debug_triangulate_ms", C.c_int32, [c_double_p, C.POINTER(C.c_int64)]),
  ("mcba_rig_poses", C.c_int32, [C.POINTER(RigPoseProblem), c_double_p, c_double_p, c_double_p, c_double_p, c_int32_p, c_int32_p,
                                 c_double_p, c_uint8_p]),
  ("mcba_debug_rig_poses_ms", C.c_int32, [c_double_p, C.POINTER(C.c_int64)]),
  ("mcba_stereo_calibrate", C.c_int32, [C.POINTER(StereoProblem), c_double_p, c_double_p, c_double_p, c_int32_p, c_int32_p, c_int32_p,
                                        c_double_p, c_double_p, c_uint8_p]),
  ("mcba_debug_stereo_calibrate_ms", C.c_int32, [c_double_p, C.POINTER(C.c_int64)]),
  ("mcba_projection_uncertainty", C.c_int32, [C.POINTER(CameraSet), c_double_p, C.c_int32, C.POINTER(UncertaintyJob), c_double_p,
                                              c_double_p, c_uint8_p]),
  ("mcba_debug_projection_uncertainty_ms", C.c_int32, [c_double_p, C.POINTER(C.c_int64)]),
  ("mcba_projection_diff", C.c_int32, [C.POINTER(CameraSet), c_double_p, C.POINTER(CameraSet), c_double_p, C.c_int32,
                                       C.POINTER(ProjDiffJob), c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_uint8_p]),
  ("mcba_debug_projection_diff_ms", C.c_int32, [c_double_p, C.POINTER(C.c_int64)]),
  ("mcba_view_information", C.c_int32, [C.POINTER(CameraSet), C.POINTER(GuidanceCamera), C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                        c_double_p, C.c_double, C.c_double, C.c_int32, C.POINTER(GuidanceView), C.POINTER(GuidanceView),
                                        C.c_int32, C.c_int32, C.POINTER(GuidanceResult)]),
  ("mcba_debug_view_information_ms", C.c_int32, [c_double_p, C.POINTER(C.c_int64)]),
  ("mcba_rig_view_information", C.c_int32, [C.POINTER(CameraSet), c_double_p, C.c_int32, C.POINTER(RigCamera), C.c_int32, C.c_int32,
                                            C.c_int32, C.POINTER(C.c_int32), c_double_p, C.c_int32, C.POINTER(RigView), C.c_int32,
                                            C.c_double, C.c_double, C.POINTER(RigFocus), C.c_int32, C.c_int32, C.c_int32,
                                            C.POINTER(RigResult)]),
  ("mcba_debug_rig_view_information_ms", C.c_int32, [c_double_p, C.POINTER(C.c_int64)]),
  ("mcba_reconstruction_uncertainty", C.c_int32, [C.POINTER(CameraSet), c_double_p, C.c_int32, C.POINTER(ReconJob), c_double_p,
                                                  C.POINTER(C.c_uint64), C.c_double, C.c_double, c_double_p, c_double_p, c_int32_p,
                                                  C.POINTER(C.c_uint64), c_uint8_p]),
  ("mcba_debug_reconstruction_uncertainty_ms", C.c_int32, [c_double_p, C.POINTER(C.c_int64)]),
  ("mcba_reconstruction_pairs", C.c_int32, [C.POINTER(CameraSet), c_double_p, C.c_int32, C.POINTER(ReconJob), c_double_p,
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_double, C.c_double,
                                            c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), c_uint8_p]),
  ("mcba_debug_reconstruction_pairs_ms", C.c_int32, [c_double_p, C.POINTER(C.c_int64)]),
  ("mcba_error_stats", C.c_int32, [H, c_double_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), c_double_p,
                                   C.POINTER(C.c_int64), c_double_p]),
  ("mcba_error_count", C.c_int32, [H, C.c_int32, C.POINTER(C.c_int64)]),
  ("mcba_reject_outliers", C.c_int32, [H, c_double_p, C.c_double, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
  ("mcba_get_inliers", C.c_int32, [H, c_uint8_p]),
  ("mcba_gather_inliers", C.c_int32, [H, c_uint8_p]),
  ("mcba_adjust_outliers", C.c_int32, [H, c_double_p, C.POINTER(Options), C.c_int32, C.c_double, C.c_double, C.c_double,
                                       C.c_double, C.POINTER(RoundReport), c_uint8_p]),
  ("mcba_normal_equations", C.c_int32, [H, c_double_p, C.POINTER(Options), c_double_p, c_double_p, c_double_p]),
  ("mcba_normal_equations_device", C.c_int32, [H, C.POINTER(Options)]),
  ("mcba_synchronize", C.c_int32, [H]),
  ("mcba_dense_hessian", C.c_int32, [H, c_double_p]),
  ("mcba_covariance_layout", C.c_int32, [H, c_int32_p, c_int32_p, c_int32_p]),
  ("mcba_covariance", C.c_int32, [H, c_double_p, c_uint8_p, C.c_double, c_double_p, c_double_p, c_double_p, c_double_p,
                                  c_double_p, C.POINTER(C.c_int64)]),
  ("mcba_observation_covariance", C.c_int32, [H, c_double_p, c_uint8_p, C.c_double, c_double_p, c_double_p, c_double_p,
                                              c_double_p, C.POINTER(C.c_int64), c_double_p]),
  ("mcba_debug_observation_covariance_ms", C.c_int32, [H, c_double_p]),
  ("mcba_debug_set_observation_covariance_route", C.c_int32, [H, C.c_int32]),
  ("mcba_residual_gram", C.c_int32, [H, c_double_p, c_int32_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_double_p,
                                     C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_int32, c_int32_p]),
  ("mcba_debug_residual_gram_ms", C.c_int32, [c_double_p, C.POINTER(C.c_int64)]),
  ("mcba_warp_points", C.c_int32, [C.POINTER(FieldSet), C.c_int64, c_int32_p, C.c_int32, c_double_p, c_double_p, c_uint8_p]),
  ("mcba_undistort_maps_corrected", C.c_int32, [C.POINTER(CameraSet), C.POINTER(FieldSet), c_double_p, c_double_p, C.c_int32, C.c_int32,
                                                C.POINTER(C.c_float)]),
  ("mcba_undistort_images_corrected", C.c_int32, [C.POINTER(CameraSet), C.POINTER(FieldSet), c_double_p, c_double_p, C.c_void_p,
                                                  C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_int32_p, C.c_int32, C.c_int32,
                                                  C.c_double, C.c_void_p]),
  ("mcba_debug_warp_ms", C.c_int32, [c_double_p, C.POINTER(C.c_int64)]),
  ("mcba_refine_corners", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_double_p, c_int32_p,
                                      C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, c_double_p, c_uint8_p,
                                      c_int32_p, c_double_p]),
  ("mcba_debug_subpix_ms", C.c_int32, [c_double_p, C.POINTER(C.c_int64)]),
  ("mcba_solve", C.c_int32, [H, c_double_p, C.POINTER(Options), C.POINTER(Result)]),
  ("mcba_time_linearize", C.c_int32, [H, c_double_p, C.POINTER(Options), C.c_int32, c_double_p]),
  ("mcba_time_residuals", C.c_int32, [H, c_double_p, C.c_int32, c_double_p]),
  ("mcba_time_lsmr_iteration", C.c_int32, [H, c_double_p, C.c_int32, c_double_p]),
  ("mcba_rccl_unique_id", C.c_int32, [C.POINTER(C.c_uint8)]),
  ("mcba_rccl_init", C.c_int32, [H, C.POINTER(C.c_uint8), C.c_int32, C.c_int32]),
  ("mcba_rccl_shutdown", C.c_int32, [H]),
  ("mcba_rccl_version", C.c_int32, [C.POINTER(C.c_int32)]),
  ("mcba_set_mfma", C.c_int32, [H, C.c_int32]),
  ("mcba_debug_set_lin_grid", C.c_int32, [H, C.c_int32]),
  ("mcba_debug_set_frame_groups", C.c_int32, [H, C.c_int32]),
  ("mcba_debug_pipe_probe", C.c_int32, [C.c_int32, C.POINTER(C.c_double)]),
  ("mcba_debug_dot3", C.c_int32, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
  ("mcba_debug_dispatch_probe", C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_longlong)]),
  ("mcba_debug_xcd_probe", C.c_int32, [C.c_int32, C.POINTER(C.c_longlong)]),
  ("mcba_debug_gn_step", C.c_int32, [H, C.c_double, c_double_p, c_double_p, c_double_p]),
  ("mcba_debug_mfma_probe", C.c_int32, [c_double_p, c_double_p]),
  ("mcba_debug_chol", C.c_int32, [H, C.c_int32, c_double_p, c_double_p, C.c_double, C.c_int32, c_double_p]),
  ("mcba_debug_set_error_table", C.c_int32, [H, c_double_p, c_double_p]),
  ("mcba_debug_linearize_profile", C.c_int32, [H, c_double_p, C.POINTER(C.c_longlong)]),
  ("mcba_debug_lsmr_products", C.c_int32, [H, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
  ("mcba_debug_lsmr_fused_products", C.c_int32, [H, c_double_p, c_double_p, c_double_p, c_double_p]),
  ("mcba_debug_lsmr_info", C.c_int32, [H, C.POINTER(C.c_int64)]),
  ("mcba_debug_set_lsmr_fused", C.c_int32, [H, C.c_int32]),
  ("mcba_debug_set_switch", C.c_int32, [C.c_char_p, C.c_char_p]),
  ("mcba_debug_lsmr_solve", C.c_int32, [H, c_double_p, C.POINTER(Options), C.c_double, c_double_p, C.c_int32, c_double_p, c_double_p, c_double_p]),
  ("mcba_debug_lsmr_trace", C.c_int32, [H, C.c_int32, c_double_p, C.POINTER(C.c_int32)]),
  ("mcba_debug_set_lsmr_trace", C.c_int32, [H, C.c_int32]),
  ("mcba_debug_set_lsmr_grid", C.c_int32, [H, C.c_int32]),
  ("mcba_debug_set_allreduce_trace", C.c_int32, [H, C.c_int32]),
  ("mcba_debug_set_lsmr_masks_form", C.c_int32, [H, C.c_int32]),
  ("mcba_debug_set_grid_cap", C.c_int32, [C.c_int32]),
  ("mcba_debug_last_capped_grid", C.c_int32, [C.POINTER(C.c_int32)]),
]

_lib = None


def load():
  global _lib
  if _lib is not None:
    return _lib
  if not os.path.exists(LIB_PATH):
    raise RuntimeError(f"{LIB_PATH} is missing: build the HIP back-end first (python -m multical_amd.build). "
                       "multical_amd has no CPU fallback.")
  lib = C.CDLL(LIB_PATH)
  for name, restype, argtypes in SYMBOLS:
    try:
      fn = getattr(lib, name)
    except AttributeError:
      # only a side-by-side build loaded through MCBA_LIB_PATH (A/B measurements against an older library) may lack an
      # entry point; the product library must export everything
      if os.environ.get("MCBA_LIB_PATH"):
        continue
      raise
    fn.restype = restype
    fn.argtypes = argtypes
  _lib = lib
  return lib


def set_switch(name, value):
  """Experiment / path-forcing switch of the library (mcba_debug_set_switch): tests and profiling scripts only; process-wide, before
  the first Handle.  The product library does not read these from the environment."""
  rc = load().mcba_debug_set_switch(name.encode(), str(value).encode())
  if rc != 0:
    raise RuntimeError(load().mcba_last_error().decode("utf-8", "replace"))


def set_grid_cap(cap):
  """Upper bound on the grid of the handle-less families' grid-stride kernels (mcba_debug_set_grid_cap): tests only; process-wide,
  effective from the next launch, 0 restores the built-in caps."""
  check(load().mcba_debug_set_grid_cap(int(cap)))


def last_capped_grid():
  """grid.x of this thread's last launch of a capped grid-stride kernel (mcba_debug_last_capped_grid)."""
  grid = C.c_int32(0)
  check(load().mcba_debug_last_capped_grid(C.byref(grid)))
  return int(grid.value)


class McbaError(RuntimeError):
  pass


def check(rc):
  if rc != 0:
    msg = load().mcba_last_error().decode("utf-8", "replace")
    # scipy raises ValueError for non-finite initial residuals (least_squares.py:844-845); keep that convention
    if "not finite" in msg:
      raise ValueError(msg)
    raise McbaError(msg)


# ---- what the wrappers of the handle-less entry points share -----------------------------------------------------------------
def f64(a):
  return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def u8(a, shape, what):
  a = np.ascontiguousarray(np.asarray(a).astype(np.uint8))
  assert a.shape == shape, f"{what} is {a.shape}, not {shape}"
  return a


def _pointer_cast(ctype):
  pointer = C.POINTER(ctype)
  return lambda a: None if a is None else a.ctypes.data_as(pointer)


# the array's data as double* / int32_t* / uint8_t* / float*; None (an argument left out) stays None
dp, ip, up, fp = (_pointer_cast(t) for t in (C.c_double, C.c_int32, C.c_uint8, C.c_float))


def entry(name):
  """The library function behind a wrapper: raises with the library's message.  (Every wrapper module calls it through its own
  `_entry` attribute: the host tests put the g++ build of the same header there.)"""
  fn = getattr(load(), "mcba_" + name)
  return lambda *args: check(fn(*args))


def call_ms(getter, labels):
  """mcba_debug_<getter>_ms of this thread's last call of that family: (dict(label -> milliseconds), the family's count)."""
  ms, n = np.zeros(len(labels)), C.c_int64(0)
  check(getattr(load(), f"mcba_debug_{getter}_ms")(dp(ms), C.byref(n)))
  return dict(zip(labels, ms)), int(n.value)
