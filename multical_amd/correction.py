"""Applying the residual field: corrected observations, points, maps and images, on the MI355X.  

`Calibration.residual_field` fits, per camera, a smooth B-spline field e(u, v) to r = projected - observed as a function of the
OBSERVED pixel.  Here that field is a warp of the image plane (csrc/mcba_warp.h):

  forward, raw -> corrected     w(p) = p + e(p): the corrected observation is what the parametric model predicts
  inverse, corrected -> raw     p + e(p) = q by Newton (FP64, analytic Jacobian): where the sensor really records a point that the
                                parametric model puts at q
  corrected camera              project_corrected(X) = w^-1(pi(X)),  undistort_corrected(p) = pi^-1(w(p))

Outside the image the field is that of the pixel clamped to it.  A field whose fold bound (FieldCorrection.fold_bound) reaches 0.2
could fold the image and is refused by every entry point.  The pair (parameters, field) is the model: parameters of two
calibrations with different corrections are not comparable on their own.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import dp as _dp, entry as _entry, f64 as _f64, fp as _fp, ip as _ip, up as _up   # noqa: F401 (_entry: see _lib.entry)

WARP_OK, WARP_NOT_CONVERGED = _lib.UNDISTORT_OK, _lib.UNDISTORT_NOT_CONVERGED
FOLD_LIMIT = 0.2
WARP_THREADS, WARP_POINTS_MAX_BLOCKS = 256, 2048      # csrc/mcba_warp_kernels.h: beyond their product a lane of k_warp_points strides


class FieldCorrection(object):
  """The fitted fields of a rig: coefficients [C, (nx + 3)(ny + 3), 2] (`residual_field().coefficients`), image_sizes [C] (W, H),
  the grid nx x ny."""

  def __init__(self, coefficients, image_sizes, nx, ny):
    self.nx, self.ny = int(nx), int(ny)
    self.coefficients = np.array(coefficients, dtype=np.float64, order="C")
    self.image_sizes = [tuple(int(v) for v in s) for s in image_sizes]
    K = (self.nx + 3) * (self.ny + 3)
    if self.coefficients.ndim != 3 or self.coefficients.shape != (len(self.image_sizes), K, 2):
      raise ValueError(f"coefficients are {self.coefficients.shape}, not [{len(self.image_sizes)}, {K}, 2]")
    self._sizes = np.ascontiguousarray(np.array(self.image_sizes, dtype=np.int32).reshape(-1, 2))

  @property
  def n(self):
    return len(self.image_sizes)

  def struct(self):
    """the mcba_field_set that points into this object's arrays (keep the object alive next to it)"""
    s = _lib.FieldSet()
    s.C, s.image_size, s.nx, s.ny, s.coef = self.n, _ip(self._sizes), self.nx, self.ny, _dp(self.coefficients)
    return s

  def fold_bound(self):
    """[C] L = max over the components of max |D_x coef| nx / W + max |D_y coef| ny / H: a bound of the infinity norm of De"""
    c = self.coefficients.reshape(self.n, self.ny + 3, self.nx + 3, 2)
    dx, dy = np.abs(np.diff(c, axis=2)).max(axis=(1, 2)), np.abs(np.diff(c, axis=1)).max(axis=(1, 2))     # [C, 2]
    sizes = np.array(self.image_sizes, dtype=np.float64)
    return np.max(dx * (self.nx / sizes[:, :1]) + dy * (self.ny / sizes[:, 1:]), axis=1)

  def _warp(self, pixels, camera_of_point, inverse):
    uv = _f64(pixels).reshape(-1, 2)
    of = None if camera_of_point is None else np.ascontiguousarray(np.asarray(camera_of_point, dtype=np.int32).reshape(-1))
    assert of is None or of.shape == (len(uv),), "one camera per point"
    out, status = np.empty((len(uv), 2)), np.empty(len(uv), dtype=np.uint8)
    s = self.struct()
    _entry("warp_points")(C.byref(s), len(uv), _ip(of), 1 if inverse else 0, _dp(uv), _dp(out), _up(status))
    return out, status

  def correct(self, pixels, camera_of_point=None):
    """mcba_warp_points, raw -> corrected: (w(p) [n, 2], status [n]); camera_of_point [n] (None: camera 0).  A non-finite pixel:
    NaN, WARP_NOT_CONVERGED."""
    return self._warp(pixels, camera_of_point, False)

  def uncorrect(self, pixels, camera_of_point=None):
    """mcba_warp_points, corrected -> raw: (w^-1(q) [n, 2], status [n])"""
    return self._warp(pixels, camera_of_point, True)

  def correct_table(self, point_table):
    """the [C, F, B, P] observation table with `points` warped raw -> corrected in one call and `valid` kept"""
    pts = _f64(point_table.points)
    assert pts.ndim == 5 and pts.shape[0] == self.n and pts.shape[-1] == 2, f"a table of {self.n} cameras"
    of = np.repeat(np.arange(self.n, dtype=np.int32), int(np.prod(pts.shape[1:4])))
    flat = pts.reshape(-1, 2)
    # (slots without a detection may hold anything: they are warped as zeros and keep what they held)
    ok = np.isfinite(flat).all(axis=1)
    if ok.all():
      out, _ = self.correct(flat, of)
    else:
      out, _ = self.correct(np.where(ok[:, None], flat, 0.0), of)
      out = np.where(ok[:, None], out, flat)
    return point_table._extend(points=out.reshape(pts.shape))

  def to_dict(self):
    return dict(nx=self.nx, ny=self.ny, image_sizes=[list(s) for s in self.image_sizes], coefficients=self.coefficients.tolist())

  @staticmethod
  def from_dict(d):
    return FieldCorrection(np.array(d["coefficients"], dtype=np.float64), d["image_sizes"], d["nx"], d["ny"])

  def field_on_grid(self, grid=(16, 12)):
    """[C, gh, gw, 2] e on the centres of `grid` of every camera (w(p) - p of mcba_warp_points)"""
    from .uncertainty import grid_of
    out = []
    for c, size in enumerate(self.image_sizes):
      gw, gh, u0, v0, du, dv = grid_of(size, grid)
      uu, vv = np.meshgrid(u0 + du * np.arange(gw), v0 + dv * np.arange(gh))
      q = np.stack([uu, vv], axis=-1).reshape(-1, 2)
      out.append((self.correct(q, np.full(len(q), c, dtype=np.int32))[0] - q).reshape(gh, gw, 2))
    return np.stack(out)


# ---- the corrected forms of the undistort module's calls (multical_amd.undistort passes its `correction` argument here) ---------
def project_points(cameras, points, camera_of_point, correction):
  """project_corrected: mcba_project_points, then the inverse warp: (pixels [n, 2], status [n])"""
  from . import undistort
  return correction.uncorrect(undistort.project_points(cameras, points, camera_of_point), camera_of_point)


def undistort_points(cameras, pixels, camera_of_point, R, P, correction):
  """undistort_corrected: the forward warp, then mcba_undistort_points: (out [n, 2], status [n]); a non-finite pixel is
  NOT_CONVERGED"""
  from . import undistort
  corrected, warped = correction.correct(pixels, camera_of_point)
  out, status = undistort.undistort_points(cameras, corrected, camera_of_point, R, P)
  return out, np.maximum(status, warped)


def undistort_maps(inp, image_size, correction):
  """mcba_undistort_maps_corrected; inp: undistort.CameraSetInputs"""
  w, h = int(image_size[0]), int(image_size[1])
  maps = np.empty((inp.n, h, w, 2), dtype=np.float32)
  s, f = inp.struct(), correction.struct()
  _entry("undistort_maps_corrected")(C.byref(s), C.byref(f), _dp(inp.R), _dp(inp.P), w, h, _fp(maps))
  return maps


def undistort_images(inp, batch, of, hd, wd, border, correction):
  """mcba_undistort_images_corrected; inp: undistort.CameraSetInputs, batch: undistort.ImageBatch"""
  out = batch.output(hd, wd)
  s, f = inp.struct(), correction.struct()
  _entry("undistort_images_corrected")(C.byref(s), C.byref(f), _dp(inp.R), _dp(inp.P), batch.data.ctypes.data_as(C.c_void_p), batch.n,
                                       batch.h, batch.w, batch.channels, batch.dtype, _ip(of), hd, wd, float(border),
                                       out.ctypes.data_as(C.c_void_p))
  return batch.shaped(out)


def report_lines(correction, names, before, after, stage=""):
  """one line per camera: the fold bound, the largest |e| on the default grid, the rms before and after the correction"""
  L, mag = correction.fold_bound(), np.linalg.norm(correction.field_on_grid(), axis=-1)
  return [f"{stage} {name}: residual correction fold bound={L[c]:.4f} max |e|={float(mag[c].max()):.3f} px "
          f"rms before={before[c]:.3f} after={after[c]:.3f}" for c, name in enumerate(names)]


def last_call_ms():
  """mcba_debug_warp_ms of this thread's last call: (dict(upload, kernel, download, call) in milliseconds, points or pixels written)."""
  return _lib.call_ms("warp", ("upload", "kernel", "download", "call"))
