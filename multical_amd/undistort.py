"""Using a calibration: project, undistort points, undistortion maps and the bicubic remap, on the MI355X.

The reference's cameras carry `project`, `undistort_points` and `undistort_map` (multical/camera.py:113-128,
multical/camera_fisheye.py:102-117: cv2.projectPoints, cv2.undistortPoints, cv2.initUndistortRectifyMap) and
`camera.undistort_images` pushes every image of every camera through cv2.remap(INTER_CUBIC) in a thread pool (camera.py:244-258).
Here they are five entry points of libmcba.so (csrc/mcba_undistort.h); `undistort_images` is ONE launch for all images of a size,
the map coordinate computed in registers where the interpolation needs it.

Cameras are anything with `intrinsic` [3, 3] and `dist` (multical_amd.camera.Camera, CameraFisheye, the reference's own classes).
Images are uint8 or float32 arrays [H, W] or [H, W, 3]; a batch is [N, H, W(, 3)].
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import dp as _dp, entry as _entry, f64 as _f64, fp as _fp, ip as _ip, up as _up   # noqa: F401 (_entry: see _lib.entry)
from .tables import _is_fisheye

UNDISTORT_OK, UNDISTORT_NOT_CONVERGED = _lib.UNDISTORT_OK, _lib.UNDISTORT_NOT_CONVERGED
_DTYPES = {np.dtype(np.uint8): _lib.PIXEL_U8, np.dtype(np.float32): _lib.PIXEL_F32}


class CameraSetInputs(object):
  """The arrays of one mcba_camera_set, kept alive next to the ctypes struct that points into them; R, P: one [3, 3] per camera
  (or one for all), None = absent."""

  def __init__(self, cameras, R=None, P=None):
    cameras = list(cameras)
    assert len(cameras) > 0, "no cameras"
    nds = [int(np.asarray(c.dist).size) for c in cameras]
    self.n = len(cameras)
    self.n_dist = max(nds + [4])
    self.cameras = np.zeros((self.n, 5 + self.n_dist))
    for i, c in enumerate(cameras):
      K = np.asarray(c.intrinsic, dtype=np.float64)
      self.cameras[i, :5] = [K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 1]]
      self.cameras[i, 5:5 + nds[i]] = np.asarray(c.dist, dtype=np.float64).ravel()
    self.camera_n_dist = np.ascontiguousarray(np.array(nds, dtype=np.int32))
    self.is_fisheye = np.ascontiguousarray(np.array([_is_fisheye(c) for c in cameras], dtype=np.uint8))
    self.R, self.P = self._per_camera(R), self._per_camera(P)

  def _per_camera(self, M):
    if M is None:
      return None
    M = _f64(M)
    M = np.ascontiguousarray(np.broadcast_to(M, (self.n, 3, 3))) if M.ndim == 2 else M
    assert M.shape == (self.n, 3, 3), "one 3 x 3 matrix per camera"
    return M

  def struct(self):
    s = _lib.CameraSet()
    s.C, s.cameras, s.n_dist = self.n, _dp(self.cameras), self.n_dist
    s.camera_n_dist = _ip(self.camera_n_dist)
    s.is_fisheye = _up(self.is_fisheye)
    return s

  def index(self, of, n):
    """[n] int32 camera of every item; None = camera 0"""
    if of is None:
      return None
    of = np.ascontiguousarray(np.asarray(of, dtype=np.int32).reshape(-1))
    assert of.shape == (n,)
    return of


class ImageBatch(object):
  """Images of one size as the [N, H, W, channels] block the library reads, and the shape their results go back to."""

  def __init__(self, images):
    a = np.asarray(images)
    if a.dtype not in _DTYPES:
      raise TypeError(f"images must be uint8 or float32, not {a.dtype}")
    if a.ndim == 3:
      a = a[..., None]
    if a.ndim != 4:
      raise ValueError(f"images must be [N, H, W] or [N, H, W, channels], not {np.asarray(images).shape}")
    self.grey = np.asarray(images).ndim == 3
    self.data = np.ascontiguousarray(a)
    self.n, self.h, self.w, self.channels = self.data.shape
    self.dtype = _DTYPES[self.data.dtype]

  def output(self, h, w):
    return np.empty((self.n, h, w, self.channels), dtype=self.data.dtype)

  def shaped(self, out):
    return out[..., 0] if self.grey else out


def project_points(cameras, points, camera_of_point=None, correction=None):
  """mcba_project_points: pixels [n, 2] of camera-frame points [n, 3]; camera_of_point [n] indexes `cameras` (None: camera 0).
  correction (a correction.FieldCorrection): the corrected camera, w^-1 of the projection -- (pixels, status) of two device calls."""
  if correction is not None:
    from . import correction as _correction
    return _correction.project_points(cameras, points, camera_of_point, correction)
  inp = CameraSetInputs(cameras)
  X = _f64(points).reshape(-1, 3)
  of = inp.index(camera_of_point, len(X))
  uv = np.empty((len(X), 2))
  s = inp.struct()
  _entry("project_points")(C.byref(s), len(X), _ip(of), _dp(X), _dp(uv))
  return uv


def undistort_points(cameras, pixels, camera_of_point=None, R=None, P=None, correction=None):
  """mcba_undistort_points: (out [n, 2], status [n]).  out = P [X/W, Y/W, 1] with [X Y W] = R [x y 1] of the undistorted normalised
  point; P = None: the normalised point.  A pixel the model cannot have produced: NaN, status UNDISTORT_NOT_CONVERGED.
  correction: the corrected camera, the forward warp of the pixels first (two device calls)."""
  if correction is not None:
    from . import correction as _correction
    return _correction.undistort_points(cameras, pixels, camera_of_point, R, P, correction)
  inp = CameraSetInputs(cameras, R, P)
  uv = _f64(pixels).reshape(-1, 2)
  of = inp.index(camera_of_point, len(uv))
  out, status = np.empty((len(uv), 2)), np.empty(len(uv), dtype=np.uint8)
  s = inp.struct()
  _entry("undistort_points")(C.byref(s), len(uv), _ip(of), _dp(uv), _dp(inp.R), _dp(inp.P), _dp(out),
                             _up(status))
  return out, status


def undistort_maps(cameras, image_size, R=None, P=None, correction=None):
  """mcba_undistort_maps: [C, H, W, 2] float32, the source coordinate (x, y) of every pixel of the undistorted image of
  image_size = (width, height); P = None: each camera's own matrix (cv2.initUndistortRectifyMap(K, dist, R, P, size, CV_32FC2)).
  correction: mcba_undistort_maps_corrected, the maps of the corrected cameras."""
  inp = CameraSetInputs(cameras, R, P)
  if correction is not None:
    from . import correction as _correction
    return _correction.undistort_maps(inp, image_size, correction)
  w, h = int(image_size[0]), int(image_size[1])
  maps = np.empty((inp.n, h, w, 2), dtype=np.float32)
  s = inp.struct()
  _entry("undistort_maps")(C.byref(s), _dp(inp.R), _dp(inp.P), w, h, _fp(maps))
  return maps


def remap(images, maps, map_of_image=None, border=0.0):
  """mcba_remap: cv2.remap(image, map, None, INTER_CUBIC) with a constant border for a batch: images [N, Hs, Ws(, 3)], maps
  [M, Hd, Wd, 2] float32 (or one [Hd, Wd, 2]); image i goes through map map_of_image[i] (None: map 0).  Returns [N, Hd, Wd(, 3)]."""
  batch = ImageBatch(images)
  maps = np.ascontiguousarray(np.asarray(maps, dtype=np.float32))
  maps = maps[None] if maps.ndim == 3 else maps
  assert maps.ndim == 4 and maps.shape[3] == 2, "maps are [M, H, W, 2]"
  of = np.zeros(batch.n, dtype=np.int32) if map_of_image is None else np.ascontiguousarray(np.asarray(map_of_image, dtype=np.int32))
  assert of.shape == (batch.n,)
  M, hd, wd = maps.shape[:3]
  out = batch.output(hd, wd)
  _entry("remap")(batch.data.ctypes.data_as(C.c_void_p), batch.n, batch.h, batch.w, batch.channels, batch.dtype,
                  _fp(maps), M, hd, wd, _ip(of), float(border), out.ctypes.data_as(C.c_void_p))
  return batch.shaped(out)


def undistort_images(cameras, images, camera_of_image=None, image_size=None, R=None, P=None, border=0.0, correction=None):
  """mcba_undistort_images: remap(images, undistort_maps(cameras, image_size, R, P), camera_of_image) in one launch and without
  the maps; image_size = (width, height) of the result, None: that of the images.  correction: mcba_undistort_images_corrected,
  the remap through the corrected maps, which stay on the device."""
  batch = ImageBatch(images)
  inp = CameraSetInputs(cameras, R, P)
  of = np.zeros(batch.n, dtype=np.int32) if camera_of_image is None else inp.index(camera_of_image, batch.n)
  wd, hd = (batch.w, batch.h) if image_size is None else (int(image_size[0]), int(image_size[1]))
  if correction is not None:
    from . import correction as _correction
    return _correction.undistort_images(inp, batch, of, hd, wd, border, correction)
  out = batch.output(hd, wd)
  s = inp.struct()
  _entry("undistort_images")(C.byref(s), _dp(inp.R), _dp(inp.P), batch.data.ctypes.data_as(C.c_void_p), batch.n, batch.h, batch.w,
                             batch.channels, batch.dtype, _ip(of), hd, wd, float(border), out.ctypes.data_as(C.c_void_p))
  return batch.shaped(out)


def last_call_ms():
  """mcba_debug_undistort_ms of this thread's last call: (dict(upload, kernel, download, call) in milliseconds, pixels written)."""
  return _lib.call_ms("undistort", ("upload", "kernel", "download", "call"))
