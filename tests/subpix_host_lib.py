"""TEST INFRASTRUCTURE: ctypes wrapper of tests/subpix_host (g++ build of multical_amd/csrc/mcba_subpix.h, the mathematics of
mcba_refine_corners) + the status cases the host and the device tests share."""
import numpy as np

import host_build
import subpix_reference as ref
from multical_amd import subpix

from multical_amd import _lib

_SIGNATURE = {name: argtypes for name, _, argtypes in _lib.SYMBOLS}["mcba_refine_corners"]
_host = host_build.HostLib("subpix_host", "sph", ["refine_corners"], extra={"refine_corners_wave_order": _SIGNATURE}, module=subpix)
lib, build, entry, host_backend, on_host = _host.lib, _host.build, _host.entry, _host.host_backend, _host.on_host


def refine_on_host(*args, **kwargs):
  """subpix.refine_corners served by the host build, the sums in row order"""
  return on_host(subpix.refine_corners, *args, **kwargs)


def refine_in_wave_order(*args, **kwargs):
  """subpix.refine_corners served by the host build with the sums in the order of the device (64 lane partials, xor butterfly)"""
  saved = subpix._entry
  subpix._entry = lambda name: entry(name + "_wave_order")
  try:
    return subpix.refine_corners(*args, **kwargs)
  finally:
    subpix._entry = saved


def border_corners(shape, w):
  """starts within the window of each border and of each image corner"""
  H, W = shape
  xs, ys = [0.0, 0.4 * w, W / 2 + 0.3, W - 1 - 0.6 * w, W - 0.01], [0.0, 0.7 * w, H / 2 - 0.2, H - 1 - 0.3 * w, H - 0.01]
  return np.array([(x, y) for y in ys for x in xs if not (x == xs[2] and y == ys[2])])


def status_cases():
  """[(name, images, corners, image_of, kwargs)]: inputs whose statuses the restatement decides -- starts within the window of every border and image corner
  of a texture (three iterations: the replicate border enters every sample) and of image A, a constant
  image, invalid starts, a start 1.5 windows from the only corner of image B, one iteration"""
  A, tA = ref.image_a()
  B, tB = ref.image_b()
  T = ref.texture()
  flat = np.full(ref.SHAPE, 77, dtype=np.uint8)
  H, W = ref.SHAPE
  invalid = np.array([(np.nan, 5.0), (5.0, np.inf), (-0.5, 5.0), (5.0, -1e-9), (float(W), 5.0), (5.0, float(H)), (-np.inf, np.nan)])
  away = tB[:4] + 1.5 * 5 * np.array([(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.7, -0.7)])
  return [
    ("border-w3", T, border_corners(ref.SHAPE, 3), dict(window=3, max_iter=3, eps=0.0)),
    ("border-w8", T, border_corners(ref.SHAPE, 8), dict(window=8, max_iter=3, eps=0.0)),
    ("border-w15x2", T, border_corners(ref.SHAPE, 15), dict(window=(15, 2), max_iter=3, eps=0.0)),
    ("border-checker", A, border_corners(ref.SHAPE, 8), dict(window=8)),
    ("constant", flat, np.array([(10.3, 20.6), (0.0, 0.0), (100.5, 90.5)]), dict(window=4)),
    ("invalid", A, invalid, dict(window=3)),
    ("away", B, away, dict(window=5)),
    ("one-iteration", A, ref.starts(tA, 1.0), dict(window=3, max_iter=1)),
  ]
