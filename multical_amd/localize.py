"""Using a calibration: where the rig was in frames that were not part of it (multi-camera PnP), on the MI355X.

One entry point of libmcba.so (csrc/mcba_localize.h): cameras, camera poses, boards and board poses are held, and every frame of a
detection table is one workgroup of ONE launch -- Levenberg-Marquardt over the frame's own rig pose (start and end under rolling
shutter) on the pixel residuals of the project's own projection.  The reference does this with a second run of its bundle adjustment
(`--fix_intrinsic --fix_camera_poses` on a held-out set, as its README advises); Calibration.with_localized_frames is that here.

Cameras are anything with `intrinsic` [3, 3], `dist` and (for rolling shutter) `image_size`.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import dp as _dp, entry as _entry, f64 as _f64, ip as _ip, u8 as _u8, up as _up   # noqa: F401 (_entry: see _lib.entry)
from .structs import struct
from .undistort import CameraSetInputs

OK, TOO_FEW, DEGENERATE, NOT_CONVERGED, BEHIND = (_lib.RIG_OK, _lib.RIG_TOO_FEW, _lib.RIG_DEGENERATE, _lib.RIG_NOT_CONVERGED,
                                                  _lib.RIG_BEHIND)
MAX_CAMERAS = _lib.RIG_MAX_CAMERAS


def covariance_matrices(tri, K):
  """[..., K (K + 1) / 2] upper triangles by rows -> [..., K, K]"""
  tri = np.asarray(tri)
  iu = np.triu_indices(K)
  out = np.zeros(tri.shape[:-1] + (K, K))
  out[..., iu[0], iu[1]] = tri
  out[..., iu[1], iu[0]] = tri
  return out


class RigPoseInputs(object):
  """The arrays of one mcba_rig_pose_problem, kept alive next to the ctypes struct that points into them."""

  def __init__(self, cameras, camera_poses, board_poses, board_points, points, valid, board_valid=None, init=None, init_end=None,
               rolling=False, sigma=None, max_iterations=20):
    self.cams = CameraSetInputs(cameras)
    Cn = self.cams.n
    self.points = _f64(points)
    assert self.points.ndim == 5 and self.points.shape[0] == Cn and self.points.shape[4] == 2, "points are [C, F, B, P, 2]"
    _, F, B, P, _ = self.points.shape
    self.shape = (Cn, F, B, P)
    self.valid = _u8(valid, self.shape, "valid")
    self.camera_poses, self.board_poses = _f64(camera_poses), _f64(board_poses)
    assert self.camera_poses.shape == (Cn, 4, 4) and self.board_poses.shape == (B, 4, 4), "poses are [C, 4, 4] and [B, 4, 4]"
    if isinstance(board_points, (list, tuple)):           # one [P_b, 3] array per board: padded at the end of the row
      padded, bv = np.zeros((B, P, 3)), np.zeros((B, P), dtype=np.uint8)
      for b, x in enumerate(board_points):
        x = np.asarray(x, dtype=np.float64)
        padded[b, :len(x)] = x
        bv[b, :len(x)] = 1
      board_points, board_valid = padded, bv if board_valid is None else board_valid
    self.board_points = _f64(board_points)
    assert self.board_points.shape == (B, P, 3), "board_points are [B, P, 3]"
    self.board_valid = None if board_valid is None else _u8(board_valid, (B, P), "board_valid")
    self.init = None if init is None else _f64(init)
    self.init_end = None if init_end is None else _f64(init_end)
    assert self.init is None or self.init.shape == (F, 4, 4), "init is [F, 4, 4]"
    assert self.init_end is None or (self.init is not None and self.init_end.shape == (F, 4, 4)), "init_end is [F, 4, 4], with init"
    self.rolling = bool(rolling)
    self.heights = _f64([c.image_size[1] for c in cameras]) if self.rolling else None
    self.sigma = 0.0 if sigma is None else float(sigma)
    self.max_iterations = int(max_iterations)
    self.K = 12 if self.rolling else 6

  def struct(self):
    p = _lib.RigPoseProblem()
    p.cams = self.cams.struct()
    _, p.F, p.B, p.P = self.shape
    p.camera_poses, p.board_poses, p.board_points = _dp(self.camera_poses), _dp(self.board_poses), _dp(self.board_points)
    p.board_valid, p.points, p.valid = _up(self.board_valid), _dp(self.points), _up(self.valid)
    p.init, p.init_end = _dp(self.init), _dp(self.init_end)
    p.rolling, p.image_heights = int(self.rolling), _dp(self.heights)
    p.sigma_px, p.max_iterations = self.sigma, self.max_iterations
    return p

  def outputs(self):
    Cn, F, B, P = self.shape
    return struct(poses=np.empty((F, 4, 4)), poses_end=np.empty((F, 4, 4)), cov=np.empty((F, self.K * (self.K + 1) // 2)),
                  sse=np.empty(F), n_obs=np.empty(F, dtype=np.int32), iters=np.empty(F, dtype=np.int32), error=np.empty(self.shape),
                  status=np.empty(F, dtype=np.uint8))


def localize_rig(cameras, camera_poses, board_poses, board_points, points, valid, init=None, rolling=False, sigma=None,
                 max_iterations=20, init_end=None, board_valid=None):
  """mcba_rig_poses.  camera_poses [C, 4, 4] rig -> camera, board_poses [B, 4, 4] board -> world, board_points [B, P, 3] (or one
  [P_b, 3] array per board), points [C, F, B, P, 2] pixels, valid [C, F, B, P].  init [F, 4, 4]: start poses (None: from the frame's
  own views); rolling: start and end pose per frame, scan time v / image height.  sigma: the standard deviation of a pixel coordinate
  behind `cov`; None: each frame's own sse / (2 n - k).  Returns struct(poses [F, 4, 4], poses_end (rolling, else None), cov
  [F, k, k] over (rx ry rz tx ty tz) of the start then the end, sse [F], n_obs [F], iters [F], error [C, F, B, P], status [F]); frames
  without a result are the identity with NaN covariance (status TOO_FEW or DEGENERATE)."""
  inp = RigPoseInputs(cameras, camera_poses, board_poses, board_points, points, valid, board_valid=board_valid, init=init,
                      init_end=init_end, rolling=rolling, sigma=sigma, max_iterations=max_iterations)
  out = inp.outputs()
  p = inp.struct()
  _entry("rig_poses")(C.byref(p), _dp(out.poses), _dp(out.poses_end), _dp(out.cov), _dp(out.sse), _ip(out.n_obs), _ip(out.iters),
                      _dp(out.error), _up(out.status))
  return struct(poses=out.poses, poses_end=out.poses_end if inp.rolling else None, cov=covariance_matrices(out.cov, inp.K), sse=out.sse,
                n_obs=out.n_obs, iters=out.iters, error=out.error, status=out.status)


def last_call_ms():
  """mcba_debug_rig_poses_ms of this thread's last call: (dict(upload, start_kernel, kernel, download, call) in milliseconds, frames
  launched)."""
  return _lib.call_ms("rig_poses", ("upload", "start_kernel", "kernel", "download", "call"))
