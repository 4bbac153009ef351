"""Using a calibration: the 3-D points behind what several cameras of the rig saw at once, on the MI355X.

One entry point of libmcba.so (csrc/mcba_triangulate.h): every (frame, point) of a table is one lane of ONE launch -- exact
undistortion, plane-intersection start, Levenberg-Marquardt on the pixel residuals of the project's own projection.  The reference
has no counterpart; its README asks users to judge a calibration on held-out data, and the distance between triangulated board
corners and the board geometry the rig predicts (Calibration.reconstruction_error) is that judgement in metres.

Cameras are anything with `intrinsic` [3, 3], `dist` and (for rolling shutter) `image_size`.  A view matrix is the top three rows
of camera_pose[c] @ rig_pose[f]: it takes a point of the rig's world frame into the camera frame.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import dp as _dp, entry as _entry, f64 as _f64, ip as _ip, u8 as _u8, up as _up   # noqa: F401 (_entry: see _lib.entry)
from .structs import struct
from .undistort import CameraSetInputs

OK, TOO_FEW, DEGENERATE, NOT_CONVERGED, BEHIND = (_lib.TRI_OK, _lib.TRI_TOO_FEW, _lib.TRI_DEGENERATE, _lib.TRI_NOT_CONVERGED,
                                                  _lib.TRI_BEHIND)
MAX_CAMERAS = _lib.TRI_MAX_CAMERAS


def _views(views, n_cameras, what):
  v = _f64(views)
  if v.ndim == 4 and v.shape[2:] == (4, 4):
    v = np.ascontiguousarray(v[:, :, :3, :])
  assert v.ndim == 4 and v.shape[0] == n_cameras and v.shape[2:] == (3, 4), f"{what} are [C, F, 3, 4] (or [C, F, 4, 4])"
  return v


def covariance_matrices(cov6):
  """[..., 6] upper triangles (xx xy xz yy yz zz) -> [..., 3, 3]"""
  return np.asarray(cov6)[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(np.shape(cov6)[:-1] + (3, 3))


def triangulate(cameras, views, points, valid, views_end=None, view_valid=None, sigma=None, max_iterations=20):
  """mcba_triangulate.  views [C, F, 3, 4] (views_end: the same at the end of a rolling-shutter frame), points [C, F, M, 2] pixels,
  valid [C, F, M], view_valid [C, F] or None.  sigma: the standard deviation of a pixel coordinate behind `cov`; None: each point's
  own sse / (2 n_views - 3).  Returns struct(points [F, M, 3], cov [F, M, 3, 3], sse [F, M], error [C, F, M], n_views [F, M],
  status [F, M]); points without a result are NaN (status TOO_FEW or DEGENERATE)."""
  inp = CameraSetInputs(cameras)
  views = _views(views, inp.n, "views")
  F = views.shape[1]
  points = _f64(points)
  assert points.ndim == 4 and points.shape[:2] == (inp.n, F) and points.shape[3] == 2, "points are [C, F, M, 2]"
  M = points.shape[2]
  valid = _u8(valid, (inp.n, F, M), "valid")
  heights = None
  if views_end is not None:
    views_end = _views(views_end, inp.n, "views_end")
    assert views_end.shape == views.shape
    heights = _f64([c.image_size[1] for c in cameras])
  view_valid = None if view_valid is None else _u8(view_valid, (inp.n, F), "view_valid")
  X, cov = np.empty((F, M, 3)), np.empty((F, M, 6))
  sse, err = np.empty((F, M)), np.empty((inp.n, F, M))
  n_views, status = np.empty((F, M), dtype=np.int32), np.empty((F, M), dtype=np.uint8)
  p = _lib.TriangulateProblem()
  p.cams = inp.struct()
  p.F, p.M = F, M
  p.views, p.views_end, p.image_heights = _dp(views), _dp(views_end), _dp(heights)
  p.view_valid, p.points, p.valid = _up(view_valid), _dp(points), _up(valid)
  p.sigma_px = 0.0 if sigma is None else float(sigma)
  p.max_iterations = int(max_iterations)
  _entry("triangulate")(C.byref(p), _dp(X), _dp(cov), _dp(sse), _dp(err), _ip(n_views), _up(status))
  return struct(points=X, cov=covariance_matrices(cov), sse=sse, error=err, n_views=n_views, status=status)


def rig_views(camera_poses, rig_poses):
  """[C, F, 3, 4]: top three rows of camera_pose[c] @ rig_pose[f]"""
  cam, rig = _f64(camera_poses), _f64(rig_poses)
  return np.ascontiguousarray((cam[:, None] @ rig[None, :])[:, :, :3, :])


def triangulate_rig(cameras, camera_poses, rig_poses, points, valid, rig_poses_end=None, view_valid=None, sigma=None,
                    max_iterations=20):
  """`triangulate` through the poses of a rig: camera_poses [C, 4, 4], rig_poses [F, 4, 4] (rig_poses_end: rolling shutter)."""
  end = None if rig_poses_end is None else rig_views(camera_poses, rig_poses_end)
  return triangulate(cameras, rig_views(camera_poses, rig_poses), points, valid, views_end=end, view_valid=view_valid, sigma=sigma,
                     max_iterations=max_iterations)


def last_call_ms():
  """mcba_debug_triangulate_ms of this thread's last call: (dict(upload, kernel, download, call) in milliseconds, points launched)."""
  return _lib.call_ms("triangulate", ("upload", "kernel", "download", "call"))
