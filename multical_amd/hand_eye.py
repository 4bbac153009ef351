"""The robot-world hand-eye start of a non-overlapping rig, with every solve on the MI355X.

Mirrors of three reference modules; the numeric core of all of them is cv2.calibrateRobotWorldHandEye, here mcba_hand_eye
(csrc/mcba_handeye.h: Shah's closed form, a batch of problems per device call):

  transform/hand_eye.py:8-50   `hand_eye_robot_world`, `hand_eye_robot_world_t`
  hand_eye/hand_eye.py         `HandEye`: camera poses of a rig whose cameras see no common board, from one A X = Z B solve per
                               (master camera, slave camera, master board, slave board) combination and a vote per camera pair
  hand_eye/helper.py           `probabilistic_guess`, `relative_to_cam`
  optimization/hand_eye.py     `HandEyeCalibration`

Deviations from the reference, all of them where the reference stops with an exception:
  * `hand_eye_robot_world` always uses the robot-world solve (no AX = XB fallback for OpenCV < 4.5) and raises a ValueError when
    the poses do not determine the result (fewer than 3, or rotations about one common axis) where cv2 returns numbers;
  * `probabilistic_guess`: scipy.stats.gaussian_kde needs at least 4 candidates with a non-singular covariance and raises
    otherwise (some camera pairs of the cfg5 rigs have exactly 4).  Then the candidate of the problem with the most pose pairs is
    taken (the first on ties), with density 0;
  * with EXACTLY 4 candidates the kernel density is the same at every one of them (the covariance whitens any 4 points in 3-D to a
    regular simplex: computed densities agree to 1e-14) and the reference's argmax is decided by rounding.  Candidates whose
    density is within 1e-9 (relative) of the largest count as tied, and the tie goes to the problem with the most pose pairs (the
    first on ties) -- for 4 candidates the same rule as the fallback; with 5 or more the densities differ by O(1) and the rule
    does not act;
  * a camera pair with no candidate at all raises a ValueError that names the two cameras (the reference fails inside
    probabilistic_guess on the empty list);
  * when no master camera passes the reference-camera rule (possible only when every pair fell back to density 0) the master
    with the most candidates is the reference camera (first on ties); the reference fails on `camera_poses[None]`;
  * `camera_groups.pkl` / `initial_guess.json` are written only when `image_path` is given; `camera_groups` stays on the object;
  * `HandEyeCalibration.report_error` is left out (io.report has no mirror here).
"""
import json
import os
import pickle
from functools import cached_property

import numpy as np

from . import tables
from .motion import HandEye as HandEyeMotion
from .structs import Table, subset


def _solve_pairs(A, B, solver=None):
  """one problem over all pairs of A, B [n, 4, 4]: (X, Z, status, err [n])"""
  A, B = np.asarray(A, dtype=np.float64).reshape(-1, 4, 4), np.asarray(B, dtype=np.float64).reshape(-1, 4, 4)
  assert A.shape[0] == B.shape[0]
  ok = np.ones((1, A.shape[0]), dtype=bool)
  X, Z, _, status, err = (solver or tables.hand_eye_batch)(A[None], ok, B[None], ok, [0], [0])
  return X[0], Z[0], int(status[0]), err[0]


def hand_eye_robot_world(world_wrt_camera, base_wrt_gripper, solver=None):
  """transform/hand_eye.py:20-50: solve world_wrt_camera[i] @ base_wrt_world = gripper_wrt_camera @ base_wrt_gripper[i] (the
  data-centric convention: matrices transform points).  Returns (base_wrt_world, gripper_wrt_camera, err [n])."""
  X, Z, status, err = _solve_pairs(world_wrt_camera, base_wrt_gripper, solver)
  if status != tables.HANDEYE_OK:
    raise ValueError("hand_eye_robot_world: " + ("fewer than 3 pose pairs" if status == tables.HANDEYE_TOO_FEW else
                                                 "the rotations do not determine the result (all equal or about one axis)"))
  return X, Z, err


def hand_eye_robot_world_t(camera_wrt_world, gripper_wrt_base, solver=None):
  """transform/hand_eye.py:8-16: the opposite convention (poses OF the camera / the gripper)."""
  base_wrt_world, gripper_wrt_camera, err = hand_eye_robot_world(tables.inverse_poses(camera_wrt_world),
                                                                 tables.inverse_poses(gripper_wrt_base), solver)
  return np.linalg.inv(base_wrt_world), np.linalg.inv(gripper_wrt_camera), err


KDE_TIE = 1e-9   # relative: densities this close to the largest count as equal to it


def vote(translations, n_pairs=None):
  """(index, density) of the candidate a camera pair takes: the largest Gaussian kernel density among the candidates' translations
  [n, 3] (hand_eye/helper.py:10-17); ties and the cases scipy cannot serve go to the problem with the most pairs (the module's
  deviations)."""
  from scipy import stats
  xyz = np.asarray(translations, dtype=np.float64).reshape(-1, 3).T
  n = xyz.shape[1]
  weight = np.zeros(n) if n_pairs is None else np.asarray(n_pairs)
  if n >= 4:
    try:
      density = stats.gaussian_kde(xyz)(xyz)
      if np.all(np.isfinite(density)):
        top = np.flatnonzero(density >= density.max() * (1.0 - KDE_TIE))
        k = int(top[np.argmax(weight[top])])
        return k, float(density[k])
    except (np.linalg.LinAlgError, ValueError):
      pass
  return int(np.argmax(weight)), 0.0


def probabilistic_guess(transformations_list, n_pairs=None):
  """hand_eye/helper.py:5-18: (density, chosen 4x4 as nested lists) of a list of candidate poses; n_pairs: pose pairs behind every
  candidate, for ties and the fallback."""
  assert isinstance(transformations_list, list) and len(transformations_list) > 0 and transformations_list[0].shape == (4, 4)
  k, density = vote([np.asarray(p)[:3, 3] for p in transformations_list], n_pairs)
  return density, np.asarray(transformations_list[k]).tolist()


def relative_to_cam(new_ref, camera_poses):
  """hand_eye/helper.py:20-24: every pose of {name: 4x4} expressed relative to camera `new_ref` (a new dictionary; the reference
  overwrites its argument)."""
  to_ref = np.linalg.inv(np.asarray(camera_poses[new_ref], dtype=np.float64))
  return {name: to_ref @ np.asarray(pose, dtype=np.float64) for name, pose in camera_poses.items()}


class HandEye(object):
  """hand_eye/hand_eye.py: camera poses of a non-overlapping rig.  pose_table: poses [C, F, B, 4, 4] board -> camera, valid
  [C, F, B]."""
  limit_board_image = 6

  def __init__(self, pose_table, cam_names, image_path=None, solver=None):
    assert isinstance(pose_table, Table)
    self.cam_names = list(cam_names)
    self.pose_table = pose_table
    self.image_path = image_path
    self.num_cameras, self.num_images, self.num_boards = np.asarray(pose_table.valid).shape[:3]
    assert len(self.cam_names) == self.num_cameras
    self._solver = solver or tables.hand_eye_batch
    self.viewed_boards = self.check_viewed_boards()
    self.camera_poses = {}
    self.camera_groups = {}
    self.reference_camera = None
    self.cam_init = {}
    self.handeye_df = []

  def check_viewed_boards(self):
    valid = np.asarray(self.pose_table.valid)
    return {cam: [b for b in range(self.num_boards) if valid[idx][:, b].sum() > self.limit_board_image]
            for idx, cam in enumerate(self.cam_names)}

  # rows (camera, board) x frames: the layout the device call indexes
  @cached_property
  def _rows(self):
    C_, F, B = self.num_cameras, self.num_images, self.num_boards
    poses = np.ascontiguousarray(np.moveaxis(np.asarray(self.pose_table.poses, dtype=np.float64), 2, 1)).reshape(C_ * B, F, 4, 4)
    valid = np.ascontiguousarray(np.moveaxis(np.asarray(self.pose_table.valid).astype(bool), 2, 1)).reshape(C_ * B, F)
    return poses, valid

  def _solve(self, combos):
    """[(master, slave, boardM, boardS)] -> X [n, 4, 4] slave camera w.r.t. master camera, n_pairs, status: ONE device call"""
    poses, valid = self._rows
    B = self.num_boards
    ia = np.array([m * B + bm for m, _, bm, _ in combos], dtype=np.int32)
    ib = np.array([s * B + bs for _, s, _, bs in combos], dtype=np.int32)
    # master_slave_pair inverts the board -> camera poses (hand_eye/hand_eye.py:96-97): the device inverts as it loads
    X, _, n_pairs, status, _ = self._solver(poses, valid, poses, valid, ia, ib, invert=True)
    return X, n_pairs, status

  def _common(self, master_cam, slave_cam, boardM, boardS):
    _, valid = self._rows
    B = self.num_boards
    return np.flatnonzero(valid[master_cam * B + boardM] & valid[slave_cam * B + boardS])

  def master_slave_pair(self, master_cam, slave_cam, boardM, boardS):
    """hand_eye/hand_eye.py:82-107 (camera indices): (slaveCam_wrt_masterCam, image_ids), or (None, None) with fewer than 3
    common frames or no result."""
    image_ids = self._common(master_cam, slave_cam, boardM, boardS)
    if len(image_ids) < 3:
      return None, None
    X, _, status = self._solve([(master_cam, slave_cam, boardM, boardS)])
    if status[0] != tables.HANDEYE_OK:
      return None, None
    return X[0], image_ids

  def initialise_camera_poses(self):
    """hand_eye/hand_eye.py:35-79: all combinations with at least 3 common frames in ONE device call, then the vote per camera
    pair, the reference-camera rule, and cam_init = {camera: pose} relative to cam_names[0]."""
    combos, ids = [], []
    for idm, master_cam in enumerate(self.cam_names):
      for ids_, slave_cam in enumerate(self.cam_names):
        if slave_cam == master_cam:
          continue
        for boardM in self.viewed_boards[master_cam]:
          for boardS in self.viewed_boards[slave_cam]:
            image_ids = self._common(idm, ids_, boardM, boardS)
            if len(image_ids) >= 3:
              combos.append((idm, ids_, boardM, boardS))
              ids.append(image_ids)
    if combos:
      X, n_pairs, status = self._solve(combos)
    groups = {}
    for k, (idm, ids_, boardM, boardS) in enumerate(combos):
      if status[k] != tables.HANDEYE_OK:
        continue
      master_cam, slave_cam = self.cam_names[idm], self.cam_names[ids_]
      self.handeye_df.append({"master_cam": master_cam, "slave_cam": slave_cam, "boardM": boardM, "boardS": boardS,
                              "image_ids": ids[k], "slaveCam_wrt_masterCam": X[k]})
      groups.setdefault((master_cam, slave_cam), []).append((X[k], int(n_pairs[k])))
    max_density, max_group = 0, 0
    most, most_cam = -1, None
    self.picks = {}                  # (master, slave) -> index of the chosen candidate in camera_groups[master][slave]
    for master_cam in self.cam_names:
      temp_density, temp_group = 0, 0
      self.camera_poses[master_cam] = {master_cam: np.eye(4).tolist()}
      self.camera_groups[master_cam] = {}
      for slave_cam in self.cam_names:
        if slave_cam == master_cam:
          continue
        cands = groups.get((master_cam, slave_cam), [])
        if not cands:
          raise ValueError(f"HandEye.initialise_camera_poses: no hand-eye candidate for cameras ({master_cam}, {slave_cam}): no "
                           "pair of their boards shares 3 frames that determine the relative pose")
        cs_wrto_cm = [c for c, _ in cands]
        self.camera_groups[master_cam][slave_cam] = [g.tolist() for g in cs_wrto_cm]
        pick, density = vote([c[:3, 3] for c in cs_wrto_cm], [n for _, n in cands])
        self.camera_poses[master_cam][slave_cam] = cs_wrto_cm[pick].tolist()
        self.picks[(master_cam, slave_cam)] = pick
        temp_density += density
        temp_group += len(cs_wrto_cm)
      if temp_density > max_density and temp_group > max_group:
        max_density, max_group = temp_density, temp_group
        self.reference_camera = master_cam
      if temp_group > most:
        most, most_cam = temp_group, master_cam
    if self.reference_camera is None:
      self.reference_camera = most_cam
    self.camera_poses['Reference_camera'] = self.reference_camera
    if self.image_path is not None:
      with open(os.path.join(self.image_path, 'camera_groups.pkl'), 'wb') as f:
        pickle.dump(self.camera_groups, f)
      with open(os.path.join(self.image_path, 'initial_guess.json'), 'w') as fp:
        json.dump(self.camera_poses, fp)
    init0 = relative_to_cam(self.cam_names[0], self.camera_poses[self.reference_camera])
    # the calibration's camera poses are masterCam_wrt_slaveCam
    self.cam_init = {k: np.linalg.inv(init0[k]) for k in self.cam_names}
    return self.cam_init


class HandEyeCalibration(object):
  """optimization/hand_eye.py: a Calibration driven by the hand-eye motion model (motion.HandEye), kept together with the robot's
  poses `gripper_wrt_base` [F, 4, 4] and the frame poses `world_wrt_camera` [F, 4, 4] it was started from.  Immutable: the solver
  methods return a new object."""
  _state = ('gripper_wrt_base', 'world_wrt_camera', 'calib')

  def __init__(self, calib, gripper_wrt_base, world_wrt_camera):
    assert isinstance(calib.motion, HandEyeMotion), "HandEyeCalibration needs the hand-eye motion model"
    self.calib = calib
    self.gripper_wrt_base = gripper_wrt_base
    self.world_wrt_camera = world_wrt_camera

  @staticmethod
  def initialise(calib, gripper_wrt_base, solver=None):
    """optimization/hand_eye.py:22-36: start world_wrt_base / gripper_wrt_camera from the calibration's frame poses and the robot's
    poses over the valid frames (one device call); camera poses and cameras are held from here on."""
    frames = calib.motion.frame_poses
    world_wrt_camera = np.asarray(frames.poses, dtype=np.float64)
    valid = np.asarray(frames.valid).astype(bool)
    gripper_wrt_base = np.asarray(gripper_wrt_base, dtype=np.float64)
    base_wrt_gripper = tables.inverse_poses(gripper_wrt_base)
    base_wrt_world, gripper_wrt_camera, _ = hand_eye_robot_world(world_wrt_camera[valid], base_wrt_gripper[valid], solver)
    motion = HandEyeMotion(Table.create(poses=base_wrt_gripper, valid=valid), tables.inverse_poses(base_wrt_world),
                           gripper_wrt_camera, getattr(calib.motion, "names", None))
    held = calib.copy(motion=motion).enable(camera_poses=False, cameras=False)
    return HandEyeCalibration(held, gripper_wrt_base, world_wrt_camera)

  # ---- the model's parameters ----
  model = property(lambda self: self.calib.motion)
  valid = property(lambda self: self.calib.motion.valid)
  gripper_wrt_camera = property(lambda self: self.calib.motion.gripper_wrt_camera)
  base_wrt_world = property(lambda self: tables.inverse_poses(self.calib.motion.world_wrt_base))

  @cached_property
  def cameras_wrt_gripper(self):
    """{camera name: camera w.r.t. gripper}: the hand-eye transform with each camera in turn as the rig's master"""
    return {name: tables.inverse_poses(self.calib.with_master(name).motion.gripper_wrt_camera) for name in self.calib.cameras.names}

  # ---- solves ----
  def bundle_adjust(self, **kwargs):
    return self.copy(calib=self.calib.bundle_adjust(**kwargs))

  def adjust_outliers(self, **kwargs):
    return self.copy(calib=self.calib.adjust_outliers(**kwargs))

  def __getstate__(self):
    return subset(self.__dict__, self._state)

  def copy(self, **changes):
    return type(self)(**{**self.__getstate__(), **changes})
