"""Sub-pixel refinement of detected corners on the MI355X: the step between an image and the detection table.

The reference refines the corners of every image in Python (board/common.py:50-54: cv2.cornerSubPix, called by AprilGrid.detect,
board/aprilgrid.py:194).  Here the corners of all images of one size are ONE call of libmcba.so (mcba_refine_corners,
csrc/mcba_subpix.h): one wavefront per corner, FP64, with a status, the iterations used and a corner quality per corner.

Images are grey uint8 or float32 arrays: one [H, W] or a batch [N, H, W].  Pixel centres are at integer coordinates."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import dp as _dp, entry as _entry, f64 as _f64, ip as _ip, up as _up   # noqa: F401 (_entry: see _lib.entry)

OK, MAX_ITER, SINGULAR, LEFT_IMAGE, REVERTED, INVALID = (_lib.SUBPIX_OK, _lib.SUBPIX_MAX_ITER, _lib.SUBPIX_SINGULAR,
                                                         _lib.SUBPIX_LEFT_IMAGE, _lib.SUBPIX_REVERTED, _lib.SUBPIX_INVALID)
STATUS_NAMES = dict(ok=OK, max_iter=MAX_ITER, singular=SINGULAR, left_image=LEFT_IMAGE, reverted=REVERTED, invalid=INVALID)
_DTYPES = {np.dtype(np.uint8): _lib.PIXEL_U8, np.dtype(np.float32): _lib.PIXEL_F32}
# the reference's criteria (board/common.py:51)
REFERENCE_MAX_ITER, REFERENCE_EPS = 30, 1e-4


def _pair(value, what):
  """(x, y) of an int or a pair"""
  if np.ndim(value) == 0:
    return int(value), int(value)
  x, y = value
  assert int(x) == x and int(y) == y, f"{what} must be whole numbers"
  return int(x), int(y)


def _grey_batch(images):
  a = np.asarray(images)
  if a.dtype not in _DTYPES:
    raise TypeError(f"images must be uint8 or float32, not {a.dtype}")
  if a.ndim == 2:
    a = a[None]
  if a.ndim != 3:
    raise ValueError(f"images must be grey, [H, W] or [N, H, W], not {np.asarray(images).shape}: a channel count other than 1 is not served")
  return np.ascontiguousarray(a)


def refine_corners(images, corners, image_of_corner=None, window=5, zero_zone=-1, max_iter=REFERENCE_MAX_ITER, eps=REFERENCE_EPS):
  """mcba_refine_corners: (refined [n, 2] float64, status [n] uint8, iterations [n] int32, quality [n]) of corners [n, 2] (x, y) in
  images [N, H, W] (or one [H, W]); image_of_corner [n] indexes the images (None: image 0).  window, zero_zone: half sizes as in
  cv2.cornerSubPix, an int or (x, y).  quality: the mean squared gradient along the weakest direction of the last window, in grey
  levels squared -- what to threshold to drop blurred or flat corners."""
  batch = _grey_batch(images)
  xy = _f64(corners).reshape(-1, 2)
  n = len(xy)
  of = None
  if image_of_corner is not None:
    of = np.ascontiguousarray(np.asarray(image_of_corner, dtype=np.int32).reshape(-1))
    assert of.shape == (n,), "one image index per corner"
  wx, wy = _pair(window, "window")
  zx, zy = _pair(zero_zone, "zero_zone")
  refined, status = np.empty((n, 2)), np.empty(n, dtype=np.uint8)
  iterations, quality = np.empty(n, dtype=np.int32), np.empty(n)
  N, H, W = batch.shape
  _entry("refine_corners")(batch.ctypes.data_as(C.c_void_p), N, H, W, _DTYPES[batch.dtype], n, _dp(xy), _ip(of), wx, wy, zx, zy,
                           int(max_iter), float(eps), _dp(refined), _up(status), _ip(iterations), _dp(quality))
  return refined, status, iterations, quality


def subpix_corners(image, detections, window):
  """board.subpix_corners (board/common.py:50-54) with its signature and criteria: detections with `corners` refined in a square
  window, the dtype of the corners kept."""
  corners = np.asarray(detections.corners)
  refined = refine_corners(image, corners.reshape(-1, 2), window=window, zero_zone=-1)[0]
  return detections._extend(corners=refined.astype(corners.dtype if corners.dtype.kind == "f" else np.float64).reshape(-1, 2))


def last_call_ms():
  """mcba_debug_subpix_ms of this thread's last call: (dict(upload, kernel, download, call) in milliseconds, corners)."""
  return _lib.call_ms("subpix", ("upload", "kernel", "download", "call"))
