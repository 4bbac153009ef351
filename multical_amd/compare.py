"""Comparing two calibrations of one rig: where does calibration 1 project what calibration 0 sees at a pixel?  

One entry point of libmcba.so (csrc/mcba_projdiff.h), the twin of multical_amd.uncertainty: that module predicts the covariance of a
projected point, this one measures the difference the covariance is supposed to bound.

  reference=None   intrinsics difference of each camera: pixel q is unprojected with calibration 0, moved by the IMPLIED TRANSFORM
                   (the rotation, or rigid motion at a finite distance, that best explains the two calibrations over the fit pixels
                   -- cx, cy trade against the camera's rotation, the focal length against distance) and projected with
                   calibration 1; diff = q' - q.  The transform is fitted on the device, once per camera, before the map.
  reference=a      transfer difference: camera a sees a point at pixel q at the given distance; diff is where camera b sees it under
                   calibration 1 minus where it does under calibration 0 (`landing`).  "Has camera b moved against camera a?"
                   Does not depend on the gauge, needs no fit; 0 for a itself.

This module marshals the jobs; undistort.CameraSetInputs, uncertainty.RigModel (the fix_aspect rule) and uncertainty.grid_of are
reused as they are.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import dp as _dp, entry as _entry, f64 as _f64, up as _up   # noqa: F401 (_entry: see _lib.entry)
from .structs import struct
from .uncertainty import RigModel, grid_of
from .undistort import CameraSetInputs

OK, NOT_CONVERGED, BEHIND, NO_FIT = _lib.PDIFF_OK, _lib.PDIFF_NOT_CONVERGED, _lib.PDIFF_BEHIND, _lib.PDIFF_NO_FIT
FIT_OK, FIT_TOO_FEW, FIT_NOT_CONVERGED, FIT_DEGENERATE = (_lib.PDIFF_FIT_OK, _lib.PDIFF_FIT_TOO_FEW, _lib.PDIFF_FIT_NOT_CONVERGED,
                                                          _lib.PDIFF_FIT_DEGENERATE)
NONE, ROTATION, RIGID = _lib.PDIFF_MODE_NONE, _lib.PDIFF_MODE_ROTATION, _lib.PDIFF_MODE_RIGID
MAX_FIT = _lib.PDIFF_MAX_FIT
FIT_MODES = dict(none=NONE, rotation=ROTATION, rigid=RIGID)


def fit_mode(fit, distance):
  """MCBA_PDIFF_MODE_* of `fit`: a mode, its name, or "auto" = a rotation at infinity, a rigid motion at a finite distance"""
  if isinstance(fit, str):
    if fit == "auto":
      return ROTATION if np.isinf(distance) else RIGID
    if fit not in FIT_MODES:
      raise ValueError(f"projection_diff: fit is 'auto' or one of {sorted(FIT_MODES)}, not {fit!r}")
    return FIT_MODES[fit]
  return int(fit)


class Job(object):
  """One job of the call: camera b, reference a (None: the camera itself), distance, fit mode, the fit pixels (fit_grid (gw, gh, u0,
  v0, du, dv) or fit_pixels [m, 2]; ignored by a job that does not fit), the focus disc (u, v, radius) or None, and its queries: grid
  (gw, gh, u0, v0, du, dv) or pixels [n, 2]."""

  def __init__(self, camera, reference=None, distance=np.inf, fit=NONE, fit_grid=None, fit_pixels=None, focus=None, grid=None,
               pixels=None):
    self.camera, self.reference = int(camera), None if reference is None else int(reference)
    self.rho = 0.0 if np.isinf(distance) else 1.0 / float(distance)
    self.fit = fit_mode(fit, distance)
    self.fit_grid = fit_grid
    self.fit_pixels = None if fit_pixels is None else np.ascontiguousarray(_f64(fit_pixels).reshape(-1, 2))
    self.focus = (0.0, 0.0, 0.0) if focus is None else tuple(float(v) for v in focus)
    assert (grid is None) != (pixels is None), "a job has a grid or a list of pixels"
    self.grid = grid
    self.pixels = None if pixels is None else np.ascontiguousarray(_f64(pixels).reshape(-1, 2))

  @property
  def n(self):
    return self.grid[0] * self.grid[1] if self.grid is not None else len(self.pixels)

  @staticmethod
  def _grid_array(grid):
    gw, gh, u0, v0, du, dv = grid
    u = u0 + np.arange(gw, dtype=np.float64) * du
    v = v0 + np.arange(gh, dtype=np.float64) * dv
    return np.stack(np.broadcast_arrays(u[None, :], v[:, None]), axis=-1).reshape(-1, 2)

  def pixel_array(self):
    """[n, 2] the pixels of the job as the device generates them (a product and a sum, each rounded once)"""
    return self.pixels if self.grid is None else self._grid_array(self.grid)

  def fit_pixel_array(self):
    """[m, 2] the fit pixels of the job (before the focus disc), or None for a job without"""
    if self.fit_pixels is not None:
      return self.fit_pixels
    return None if self.fit_grid is None else self._grid_array(self.fit_grid)


def run_jobs(rig0, rig1, jobs):
  """mcba_projection_diff over the jobs: struct(transform [J, 6], fit_info [J, 5], diff [n_total, 2], magnitude [n_total], landing
  [n_total, 2], status [n_total]), job after job.  rig0, rig1: uncertainty.RigModel of the two calibrations."""
  inp0, inp1 = CameraSetInputs(rig0.cameras), CameraSetInputs(rig1.cameras)
  recs = (_lib.ProjDiffJob * max(len(jobs), 1))()
  for rec, job in zip(recs, jobs):
    rec.camera, rec.reference = job.camera, -1 if job.reference is None else job.reference
    rec.inv_distance, rec.fit = job.rho, job.fit
    if job.fit_pixels is not None:
      rec.fit_grid_w, rec.fit_grid_h, rec.fit_n, rec.fit_uv = 0, 0, len(job.fit_pixels), _dp(job.fit_pixels)
    elif job.fit_grid is not None:
      rec.fit_grid_w, rec.fit_grid_h, rec.fit_u0, rec.fit_v0, rec.fit_du, rec.fit_dv = job.fit_grid
    rec.focus_u, rec.focus_v, rec.focus_radius = job.focus
    if job.grid is not None:
      rec.grid_w, rec.grid_h, rec.u0, rec.v0, rec.du, rec.dv = job.grid
    else:
      rec.grid_w, rec.grid_h, rec.n, rec.uv = 0, 0, len(job.pixels), _dp(job.pixels)
  n, J = sum(job.n for job in jobs), len(jobs)
  out = struct(transform=np.empty((J, 6)), fit_info=np.empty((J, 5)), diff=np.empty((n, 2)), magnitude=np.empty(n),
               landing=np.empty((n, 2)), status=np.empty(n, dtype=np.uint8))
  _entry("projection_diff")(C.byref(inp0.struct()), _dp(rig0.poses), C.byref(inp1.struct()), _dp(rig1.poses), J, recs,
                            _dp(out.transform), _dp(out.fit_info), _dp(out.diff), _dp(out.magnitude), _dp(out.landing), _up(out.status))
  return out


def fit_struct(fit_info):
  """[J, 5] -> struct(n_fit, iterations, rms_before, rms_after, status)"""
  f = np.asarray(fit_info)
  return struct(n_fit=f[:, 0].astype(np.int64), iterations=f[:, 1].astype(np.int64), rms_before=f[:, 2].copy(), rms_after=f[:, 3].copy(),
                status=f[:, 4].astype(np.uint8))


def projection_diff(cameras0, poses0, cameras1, poses1, query_cameras=None, reference=None, distance=np.inf, grid=(16, 12), pixels=None,
                    fit="auto", fit_grid=(60, 40), focus=None):
  """The functional entry: no Calibration needed.  cameras0 / cameras1: the same number of cameras with `intrinsic`, `dist`,
  `image_size` (and `fix_aspect`) -- the families may differ, the image sizes are taken from cameras0; poses0 / poses1 [C, 4, 4] rig ->
  camera.  One device call for all query_cameras (default: all).  reference=None: the intrinsics difference of each camera behind
  its implied transform (fit: "auto" = "rotation" at infinity and "rigid" at a finite distance, or "none"; fit_grid: the fit pixels,
  a grid of their own of at most 65 536 pixels; focus = (u, v, radius in pixels): only fit pixels inside the disc take part).
  reference=a: the transfer difference against camera a (no fit).  Returns struct(diff [C', gh, gw, 2], magnitude [C', gh, gw],
  landing [C', gh, gw, 2] (transfer: where the point lands under calibration 0; NaN otherwise), pixels [C', gh, gw, 2], status
  (OK / NOT_CONVERGED / BEHIND / NO_FIT; NaN where not OK), transform [C', 6] rotation vector | translation, fit = struct(n_fit,
  iterations, rms_before, rms_after, status [C'])); with pixels [n, 2] and one camera the per-pixel arrays are [n, ..]."""
  rig0, rig1 = RigModel(cameras0, poses0), RigModel(cameras1, poses1)
  assert len(rig0.cameras) == len(rig1.cameras), "the two calibrations have the same cameras"
  query = list(range(len(rig0.cameras))) if query_cameras is None else [int(c) for c in np.atleast_1d(query_cameras)]
  if pixels is not None:
    assert len(query) == 1, "a list of pixels belongs to one camera"
  mode = NONE if reference is not None else fit_mode(fit, distance)
  if mode == RIGID and np.isinf(distance):
    raise ValueError("projection_diff: a rigid fit needs a finite distance")
  jobs = []
  for b in query:
    size = cameras0[b].image_size
    where = dict(pixels=pixels) if pixels is not None else dict(grid=grid_of(size, grid))
    jobs.append(Job(b, reference, distance, mode, fit_grid=grid_of(size, fit_grid) if mode != NONE else None, focus=focus, **where))
  r = run_jobs(rig0, rig1, jobs)
  px = np.concatenate([j.pixel_array() for j in jobs]) if jobs else np.zeros((0, 2))
  common = dict(transform=r.transform, fit=fit_struct(r.fit_info))
  if pixels is not None:
    return struct(diff=r.diff, magnitude=r.magnitude, landing=r.landing, pixels=px, status=r.status, **common)
  shape = (len(query), int(grid[1]), int(grid[0]))
  return struct(diff=r.diff.reshape(shape + (2,)), magnitude=r.magnitude.reshape(shape), landing=r.landing.reshape(shape + (2,)),
                pixels=px.reshape(shape + (2,)), status=r.status.reshape(shape), **common)


def significance(diff, cov0, cov1):
  """d = sqrt(diff^T (C0 + C1)^-1 diff) per pixel: diff [..., 2], cov0 / cov1 [..., 2, 2]; NaN where the sum is not positive
  definite or anything is NaN.  Calibrated (chi with two degrees of freedom) only when the two data sets are independent."""
  S = np.asarray(cov0) + np.asarray(cov1)
  a, b, c = S[..., 0, 0], 0.5 * (S[..., 0, 1] + S[..., 1, 0]), S[..., 1, 1]
  x, y = np.asarray(diff)[..., 0], np.asarray(diff)[..., 1]
  det = a * c - b * b
  with np.errstate(invalid="ignore", divide="ignore"):
    q = (c * x * x - 2.0 * b * x * y + a * y * y) / det
    return np.where((det > 0) & (a > 0), np.sqrt(np.maximum(q, 0.0)), np.nan)


def last_call_ms():
  """mcba_debug_projection_diff_ms of this thread's last call: (dict(upload, fit, map, download, call) in ms, queries launched)."""
  return _lib.call_ms("projection_diff", ("upload", "fit", "map", "download", "call"))
