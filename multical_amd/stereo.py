"""Stereo calibration of camera pairs with the cameras held (batched cv2.stereoCalibrate), on the MI355X.

One entry point of libmcba.so (csrc/mcba_stereo.h): every pair (l, r) of a detection table is one workgroup of ONE launch --
Levenberg-Marquardt over the relative pose T_rel (left-camera frame -> right-camera frame, the reference's matrix.join(R, T)) and
one board pose per common view, on the pixel residuals of the project's own projection in both cameras.  The reference gets these
numbers one cv2.stereoCalibrate call per pair (camera.py:261-286, tables.py:380-382); a rig of 8 cameras has 28 pairs.

The pair's own estimate beside camera_poses[r] @ inv(camera_poses[l]) of the joint bundle adjustment is the diagnostic behind
Calibration.pairwise_extrinsics: it says WHICH pair disagrees with the rig.

Out of scope: free intrinsics (fix_intrinsic=False: Calibration.bundle_adjust is the tool), rolling shutter (the model is cv2's static
one), match='all', robust weights and rectification (stereoRectify is host algebra on top of undistort_maps(R, P)).

Cameras are anything with `intrinsic` [3, 3] and `dist`.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import dp as _dp, entry as _entry, f64 as _f64, ip as _ip, u8 as _u8, up as _up   # noqa: F401 (_entry: see _lib.entry)
from .structs import struct
from .undistort import CameraSetInputs

OK, TOO_FEW, DEGENERATE, NOT_CONVERGED = _lib.STEREO_OK, _lib.STEREO_TOO_FEW, _lib.STEREO_DEGENERATE, _lib.STEREO_NOT_CONVERGED
STATUS_NAMES = {OK: "ok", TOO_FEW: "no common view", DEGENERATE: "degenerate views", NOT_CONVERGED: "not converged"}


def pad_boards(board_points, P):
  """(board_points [B, P, 3], board_valid [B, P]) of one [P_b, 3] array per board, padded at the end of the row"""
  padded, bv = np.zeros((len(board_points), P, 3)), np.zeros((len(board_points), P), dtype=np.uint8)
  for b, x in enumerate(board_points):
    x = np.asarray(x, dtype=np.float64)
    padded[b, :len(x)] = x
    bv[b, :len(x)] = 1
  return padded, bv


class StereoInputs(object):
  """The arrays of one mcba_stereo_problem, kept alive next to the ctypes struct that points into them."""

  def __init__(self, cameras, board_points, points, valid, view_poses, view_valid, pairs, board_valid=None, min_common=4, sigma=None,
               max_iterations=0):
    self.cams = CameraSetInputs(cameras)
    Cn = self.cams.n
    self.points = _f64(points)
    assert self.points.ndim == 5 and self.points.shape[0] == Cn and self.points.shape[4] == 2, "points are [C, F, B, P, 2]"
    _, F, B, P, _ = self.points.shape
    self.shape = (Cn, F, B, P)
    self.valid = _u8(valid, self.shape, "valid")
    if isinstance(board_points, (list, tuple)):
      board_points, bv = pad_boards(board_points, P)
      board_valid = bv if board_valid is None else board_valid
    self.board_points = _f64(board_points)
    assert self.board_points.shape == (B, P, 3), "board_points are [B, P, 3]"
    self.board_valid = None if board_valid is None else _u8(board_valid, (B, P), "board_valid")
    self.view_poses = _f64(view_poses)
    assert self.view_poses.shape == (Cn, F, B, 4, 4), "view_poses are [C, F, B, 4, 4]"
    self.view_valid = _u8(view_valid, (Cn, F, B), "view_valid")
    self.pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    self.n_pairs = len(self.pairs)
    self.min_common, self.max_iterations = int(min_common), int(max_iterations)
    self.sigma = 0.0 if sigma is None else float(sigma)

  def struct(self):
    p = _lib.StereoProblem()
    p.cams = self.cams.struct()
    _, p.F, p.B, p.P = self.shape
    p.board_points, p.board_valid = _dp(self.board_points), _up(self.board_valid)
    p.points, p.valid = _dp(self.points), _up(self.valid)
    p.view_poses, p.view_valid = _dp(self.view_poses), _up(self.view_valid)
    p.n_pairs, p.pairs = self.n_pairs, _ip(self.pairs)
    p.min_common, p.max_iterations, p.sigma_px = self.min_common, self.max_iterations, self.sigma
    return p

  def outputs(self):
    n, (_, F, B, _) = self.n_pairs, self.shape
    return struct(T=np.empty((n, 4, 4)), cov=np.empty((n, 6, 6)), sse=np.empty(n), n_views=np.empty(n, dtype=np.int32),
                  n_points=np.empty(n, dtype=np.int32), iterations=np.empty(n, dtype=np.int32), view_poses=np.empty((n, F, B, 4, 4)),
                  view_sse=np.empty((n, F, B, 2)), status=np.empty(n, dtype=np.uint8))


def skew(t):
  t = np.asarray(t, dtype=np.float64)
  z = np.zeros(t.shape[:-1])
  return np.stack([np.stack([z, -t[..., 2], t[..., 1]], -1), np.stack([t[..., 2], z, -t[..., 0]], -1),
                   np.stack([-t[..., 1], t[..., 0], z], -1)], -2)


def essential_matrices(T):
  """E = [t]x R of [..., 4, 4] relative poses (X_r = R X_l + t): x_r^T E x_l = 0 for normalised points"""
  T = np.asarray(T, dtype=np.float64)
  return skew(T[..., :3, 3]) @ T[..., :3, :3]


def fundamental_matrices(E, K_left, K_right):
  """F = K_r^-T E K_l^-1: p_r^T F p_l = 0 for distortion-free pixels"""
  return np.swapaxes(np.linalg.inv(K_right), -1, -2) @ E @ np.linalg.inv(K_left)


def calibrate_pairs(cameras, board_points, points, valid, view_poses, view_valid, pairs, board_valid=None, min_common=4, sigma=None,
                    max_iterations=0):
  """mcba_stereo_calibrate.  board_points [B, P, 3] (or one [P_b, 3] array per board), points [C, F, B, P, 2] pixels, valid
  [C, F, B, P], view_poses [C, F, B, 4, 4] start poses board -> camera with their mask view_valid [C, F, B], pairs [n, 2] (left, right).

  Returns struct(pairs, T [n, 4, 4] left-camera frame -> right-camera frame, cov [n, 6, 6] over (rx ry rz tx ty tz) of T -- global
  rotation vector, then translation -- with the view poses eliminated, sse [n], rms [n], n_views, n_points, iterations, view_poses
  [n, F, B, 4, 4] board -> left camera, view_sse [n, F, B, 2] (left | right), status [n], essential, fundamental [n, 3, 3]).

  rms = sqrt(sse / (2 n_points)): the RMS distance over the pair's 2 n_points image points.  This is believed to be the value
  cv2.stereoCalibrate returns; no cv2 binary was at hand to confirm it.  sigma: the standard deviation of a pixel coordinate behind
  `cov`; None: the pair's own sse / (4 n_points - 6 - 6 n_views).  Pairs without a result (status TOO_FEW: no view with min_common
  common corners; DEGENERATE) are the identity with NaN covariance and rms."""
  inp = StereoInputs(cameras, board_points, points, valid, view_poses, view_valid, pairs, board_valid=board_valid,
                     min_common=min_common, sigma=sigma, max_iterations=max_iterations)
  out = inp.outputs()
  p = inp.struct()
  _entry("stereo_calibrate")(C.byref(p), _dp(out.T), _dp(out.cov), _dp(out.sse), _ip(out.n_views), _ip(out.n_points),
                             _ip(out.iterations), _dp(out.view_poses), _dp(out.view_sse), _up(out.status))
  have = (out.status == OK) | (out.status == NOT_CONVERGED)
  rms = np.where(have, np.sqrt(out.sse / np.maximum(2 * out.n_points, 1)), np.nan)
  K = np.stack([np.asarray(c.intrinsic, dtype=np.float64) for c in cameras]) if len(cameras) else np.zeros((0, 3, 3))
  E = essential_matrices(out.T)
  Fm = fundamental_matrices(E, K[inp.pairs[:, 0]], K[inp.pairs[:, 1]]) if inp.n_pairs else np.zeros((0, 3, 3))
  return struct(pairs=inp.pairs, T=out.T, cov=out.cov, sse=out.sse, rms=rms, n_views=out.n_views, n_points=out.n_points,
                iterations=out.iterations, view_poses=out.view_poses, view_sse=out.view_sse, status=out.status, essential=E,
                fundamental=Fm)


COLLINEAR_TOL = 1e-6      # csrc/mcba_stereo_driver.h: COLLINEAR_TOL


def collinear_slots(board_points, common):
  """[m] of the slots common [m, P] (bool) over the board rows board_points [m, P, 3]: the common corners lie on one line -- no
  corner stands off the line from their centroid to the farthest of them by more than COLLINEAR_TOL of that distance
  (collinear_view of csrc/mcba_stereo_driver.h: the driver drops such a slot)."""
  common = np.asarray(common).astype(bool)
  X = np.asarray(board_points, dtype=np.float64)
  n = np.maximum(common.sum(axis=1), 1)
  d = (X - (X * common[..., None]).sum(axis=1)[:, None] / n[:, None, None]) * common[..., None]
  q = (d * d).sum(axis=-1)
  far = np.take_along_axis(d, np.argmax(q, axis=1)[:, None, None], axis=1)[:, 0]
  dmax = q.max(axis=1)
  off = d - ((d * far[:, None]).sum(axis=-1) / np.where(dmax > 0, dmax, 1.0)[:, None])[..., None] * far[:, None]
  return ~((off * off).sum(axis=-1) > COLLINEAR_TOL ** 2 * dmax[:, None]).any(axis=1)


def pair_views(valid, view_valid, i, j, min_common=4, board_points=None):
  """[F, B] the slots that are views of pair (i, j): start poses valid in both cameras, min_common common corners and -- with
  board_points [B, P, 3] -- not all of them on one line"""
  common = valid[i] & valid[j]
  use = (common.sum(axis=-1) >= min_common) & view_valid[i] & view_valid[j]
  if board_points is not None and use.any():
    f, b = np.nonzero(use)
    use[f, b] = ~collinear_slots(np.asarray(board_points)[b], common[f, b])
  return use


def common_view_pairs(valid, view_valid, min_common=4, board_points=None):
  """every (i, j), i < j, with a view: a slot whose start poses are valid in both cameras and that holds min_common common corners
  which -- where board_points [B, P, 3] is given, the driver's rule -- do not all lie on one line"""
  valid, view_valid = np.asarray(valid).astype(bool), np.asarray(view_valid).astype(bool)
  Cn = valid.shape[0]
  out = []
  for i in range(Cn):
    for j in range(i + 1, Cn):
      # (one view is enough: the slots are tested eight at a time until one of them is no line)
      use = pair_views(valid, view_valid, i, j, min_common)
      if board_points is not None and use.any():
        f, b = np.nonzero(use)
        common, found = valid[i] & valid[j], False
        for k in range(0, len(f), 8):
          found = found or bool((~collinear_slots(np.asarray(board_points)[b[k:k + 8]], common[f[k:k + 8], b[k:k + 8]])).any())
          if found:
            break
        if not found:
          continue
      elif not use.any():
        continue
      out.append((i, j))
  return np.asarray(out, dtype=np.int32).reshape(-1, 2)


def rotation_vectors(T):
  from scipy.spatial.transform import Rotation
  return Rotation.from_matrix(np.asarray(T, dtype=np.float64)[..., :3, :3]).as_rotvec()


def scaled_difference(T, T_other, cov):
  """How far the poses T [n, 4, 4] are from T_other in units of their own covariance cov [n, 6, 6] (calibrate_pairs' `cov`).  The
  covariance is over the GLOBAL rotation vector w and the translation t of T, so the differences are taken in those parameters:
  d_w = w(T) - w(T_other), with w(T_other) moved to the 2 pi branch next to w(T), and d_t = t(T) - t(T_other) -- NOT the rotation
  vector of R R_other^T, a left-tangent increment L(w) d_w that only agrees with d_w for small w.  Returns struct(d_rot, d_t [n, 3],
  rotation, translation [n] = sqrt(d^T C^-1 d) with C the block of that part; NaN where the block is not finite and positive
  definite)."""
  T, T_other, cov = np.asarray(T, dtype=np.float64), np.asarray(T_other, dtype=np.float64), np.asarray(cov, dtype=np.float64)
  n = len(T)
  if n == 0:
    return struct(d_rot=np.zeros((0, 3)), d_t=np.zeros((0, 3)), rotation=np.zeros(0), translation=np.zeros(0))
  w, w0 = rotation_vectors(T).reshape(n, 3), rotation_vectors(T_other).reshape(n, 3)
  angle = np.linalg.norm(w0, axis=1)
  axis = w0 / np.where(angle > 0, angle, 1.0)[:, None]
  branches = np.stack([axis * (angle + 2.0 * np.pi * k)[:, None] for k in (-1, 0, 1)], axis=1)         # the same rotation
  w0 = np.take_along_axis(branches, np.argmin(np.linalg.norm(branches - w[:, None], axis=-1), axis=1)[:, None, None], axis=1)[:, 0]
  d_rot, d_t = w - w0, T[:, :3, 3] - T_other[:, :3, 3]

  def scaled(d, C):
    out = np.full(n, np.nan)
    for k in range(n):
      if np.isfinite(C[k]).all() and np.isfinite(d[k]).all():
        try:
          out[k] = np.sqrt(max(float(d[k] @ np.linalg.solve(C[k], d[k])), 0.0))
        except np.linalg.LinAlgError:
          pass
    return out
  return struct(d_rot=d_rot, d_t=d_t, rotation=scaled(d_rot, cov[:, :3, :3]), translation=scaled(d_t, cov[:, 3:, 3:]))


def stereo_pairs(cameras, boards, point_table, pairs=None, pose_table=None, min_common=4, sigma=None, max_iterations=0):
  """The relative pose of camera pairs, every pair from its own common views, all pairs in one device call (see calibrate_pairs for
  what comes back).  boards: objects with `points` (or [P_b, 3] arrays); point_table: points [C, F, B, P, 2], valid; pose_table:
  poses [C, F, B, 4, 4], valid -- the start, None: tables.make_pose_table(..., exclude_bad_poses=False); pairs: [n, 2] (left,
  right), None: every i < j with a view (common_view_pairs, the driver's rule)."""
  from . import tables
  if pose_table is None:
    pose_table = tables.make_pose_table(point_table, boards, cameras, exclude_bad_poses=False)
  valid = np.asarray(point_table.valid).astype(bool)
  board_points = [np.asarray(getattr(b, "points", b), dtype=np.float64) for b in boards]
  if pairs is None:
    pairs = common_view_pairs(valid, pose_table.valid, min_common, pad_boards(board_points, valid.shape[3])[0])
  return calibrate_pairs(cameras, board_points, point_table.points, valid, pose_table.poses, pose_table.valid, pairs,
                         min_common=min_common, sigma=sigma, max_iterations=max_iterations)


def last_call_ms():
  """mcba_debug_stereo_calibrate_ms of this thread's last call: (dict(prepare, upload, kernel, download) in milliseconds -- the
  kernel by HIP events, the rest by host clock --, pairs launched)."""
  return _lib.call_ms("stereo_calibrate", ("prepare", "upload", "kernel", "download"))
