"""Minimal mirror of multical.workspace.Workspace for the optimisation phase only (workspace.py:228-247).

Image loading, detection, export and the pickle checkpoint are upstream / downstream of the hot path and stay with the reference
(SURVEY.md section 2 rows 11-16); a Workspace here is seeded with an initial Calibration -- given, or built from a detection table
by `calibrate_single` (workspace.py:165-194) and `initialise_poses` (workspace.py:196-226) on the device -- and reproduces
`calibrate`'s enable -> adjust_outliers sequence and argument mapping.
"""
import numpy as np

from . import tables
from .calibration import Calibration, select_threshold
from .motion import StaticFrames
from .parameters import ParamList
from .pose_set import PoseSet


class Workspace(object):
  def __init__(self, initialisation=None, name="calibration"):
    self.name = name
    self.calibrations = {}
    if initialisation is not None:
      self.calibrations["initialisation"] = initialisation

  @property
  def initialisation(self) -> Calibration:
    return self.calibrations["initialisation"]

  @property
  def latest_calibration(self) -> Calibration:
    return list(self.calibrations.values())[-1]

  def calibrate_single(self, point_table, boards, image_sizes, camera_model='standard', fix_aspect=False, has_skew=False,
                       max_images=None, intrinsic_error_limit=1.0):
    """workspace.py:165-194 from a detection table: the intrinsics of every camera from its own detections
    (camera.calibrate_cameras: all cameras of a rejection round in one device call), stored as self.cameras.  camera_model
    'fisheye' calibrates CameraFisheye objects (camera.calibrate_cameras_fisheye: one device call, no rejection rounds, as in the reference)."""
    from . import camera as camera_mod
    from .structs import struct
    valid = np.asarray(point_table.valid).astype(bool)
    pts = np.asarray(point_table.points)
    C_, F, B = valid.shape[:3]
    detections = [[[struct(ids=np.flatnonzero(valid[c, f, b]), corners=pts[c, f, b][valid[c, f, b]]) for b in range(B)]
                   for f in range(F)] for c in range(C_)]
    if camera_model == 'fisheye':
      self.cameras, errs = camera_mod.calibrate_cameras_fisheye(boards, detections, image_sizes, fix_aspect=fix_aspect,
                                                                has_skew=has_skew, max_images=max_images)
    else:
      self.cameras, errs = camera_mod.calibrate_cameras(boards, detections, image_sizes, intrinsic_error_limit, model=camera_model,
                                                        fix_aspect=fix_aspect, has_skew=has_skew, max_images=max_images)
    self.intrinsic_errors = errs
    return self.cameras

  def initialise_poses(self, point_table, boards, cameras=None, motion_model=StaticFrames, camera_poses=None, exclude_bad_poses=True,
                       pose_error_limit=1.0, names=None, is_non_overlapping=False) -> Calibration:
    """workspace.py:196-226 from a detection table: per-view board poses (tables.make_pose_table), the pose-graph initialisation
    (tables.initialise_poses) and the initial Calibration, stored as calibrations["initialisation"].  camera_poses: {camera name:
    4x4} like the reference's, or an array [C, 4, 4]; cameras=None: those of calibrate_single; names: struct(camera, board, image) of name lists (default: cam0, ...).
    is_non_overlapping (workspace.py:204-207): without given camera_poses, the camera poses come from the robot-world hand-eye
    start of a rig whose cameras share no board (hand_eye.HandEye: every camera pair x board pair in one device call)."""
    if cameras is None:
      cameras = getattr(self, "cameras", None)
      assert cameras is not None, "initialise_poses: no cameras given, first use calibrate_single"
    C_, F, B = np.asarray(point_table.valid).shape[:3]
    cam_names = list(names.camera) if names is not None else [f"cam{i}" for i in range(C_)]
    board_names = list(names.board) if names is not None else [f"board{i}" for i in range(B)]
    image_names = list(names.image) if names is not None else [f"frame{i}" for i in range(F)]
    self.pose_table = tables.make_pose_table(point_table, boards, cameras, exclude_bad_poses, pose_error_limit)
    if isinstance(camera_poses, dict):
      camera_poses = np.array([camera_poses[k] for k in cam_names])
    if is_non_overlapping and camera_poses is None:
      from .hand_eye import HandEye
      self.hand_eye = HandEye(self.pose_table, cam_names)
      cam_init = self.hand_eye.initialise_camera_poses()
      camera_poses = np.array([cam_init[k] for k in cam_names])
    pose_init = tables.initialise_poses(self.pose_table, camera_poses=camera_poses)
    calib = Calibration(ParamList(cameras, cam_names), ParamList(boards, board_names), point_table,
                        PoseSet(pose_init.camera, cam_names), PoseSet(pose_init.board, board_names),
                        motion_model.init(pose_init.times, image_names))
    self.calibrations["initialisation"] = calib
    return calib

  def calibrate(self, name="calibration", camera_poses=True, motion=True, board_poses=True, cameras=False, boards=False,
                loss='linear', tolerance=1e-4, num_adjustments=3, quantile=0.75, auto_scale=None,
                outlier_threshold=5.0) -> Calibration:
    calib = self.latest_calibration.enable(cameras=cameras, boards=boards, camera_poses=camera_poses, motion=motion,
                                           board_poses=board_poses)
    calib = calib.adjust_outliers(
      loss=loss, tolerance=tolerance, num_adjustments=num_adjustments,
      select_outliers=select_threshold(quantile=quantile, factor=outlier_threshold),
      select_scale=select_threshold(quantile=quantile, factor=auto_scale) if auto_scale is not None else None)
    self.calibrations[name] = calib
    return calib
