"""TEST INFRASTRUCTURE: ctypes wrapper of tests/residual_field (g++ build of multical_amd/csrc/mcba_residual_field.h, the mathematics
of mcba_residual_gram) + what the residual-field tests share: the observation tables of the golden fixtures with their stored
residuals, and the entry-wise error bound of a Gram matrix."""
import ctypes as C
import functools

import numpy as np

import host_build
from multical_amd._lib import c_double_p, c_int32_p, c_uint8_p, dp, ip, up
from multical_amd.structs import struct
from util import load_golden

c_int64_p = C.POINTER(C.c_int64)
_host = host_build.HostLib("residual_field", "rfh", extra={
  "cell": [C.c_double, C.c_double, C.c_int32, c_int32_p, c_double_p],
  "weights": [C.c_int64, c_double_p, c_double_p],
  "rows": [C.c_int64, c_double_p, C.c_double, C.c_double, C.c_int32, C.c_int32, c_int32_p, c_double_p, c_uint8_p],
  "residual_gram": [C.c_int32] * 4 + [c_double_p, c_double_p, c_uint8_p, c_uint8_p, c_int32_p] + [C.c_int32] * 4 +
                   [c_double_p, c_double_p, c_int64_p, c_int64_p, C.c_int32, C.c_int32, c_int32_p],
})
lib, build, entry = _host.lib, _host.build, _host.entry

FIXTURES = ("tiny", "tiny_rolling", "tiny_fisheye", "tiny_handeye")
GRIDS = {(1, 1): 18, (3, 2): 32, (4, 2): 37, (5, 3): 50, (5, 4): 58, (7, 3): 62}   # (nx, ny) -> NC


def cell(u, W, n):
  i, t = C.c_int32(), C.c_double()
  entry("cell")(float(u), float(W), int(n), C.byref(i), C.byref(t))
  return i.value, t.value


def weights(t):
  t = np.ascontiguousarray(np.asarray(t, dtype=np.float64).ravel())
  w = np.empty((t.size, 4))
  entry("weights")(t.size, dp(t), dp(w))
  return w


def rows(pixels, image_size, nx, ny):
  """(col [n, 16], w [n, 16], inside [n]) of pixels [n, 2] in one image"""
  px = np.ascontiguousarray(np.asarray(pixels, dtype=np.float64).reshape(-1, 2))
  col, w, inside = np.empty((px.shape[0], 16), dtype=np.int32), np.empty((px.shape[0], 16)), np.empty(px.shape[0], dtype=np.uint8)
  entry("rows")(px.shape[0], dp(px), float(image_size[0]), float(image_size[1]), int(nx), int(ny), ip(col), dp(w), up(inside))
  return col, w, inside.astype(bool)


def gram(projected, observed, valid, inlier, image_sizes, nx=5, ny=4, n_folds=5, inliers_only=True, coverage=(16, 12)):
  """host_residual_gram over [C,F,B,P] tables: struct(gram, absgram [C, n_folds, NC, NC], count [C, n_folds], outside [C], coverage
  [C, 2, h, w] or None)"""
  proj, obs = (np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in (projected, observed))
  va, inl = (np.ascontiguousarray(np.asarray(a).astype(np.uint8)) for a in (valid, inlier))
  n_cam, F, B, P = va.shape
  assert proj.shape == obs.shape == (n_cam, F, B, P, 2) and inl.shape == va.shape
  size = np.ascontiguousarray(np.asarray(image_sizes, dtype=np.int32).reshape(n_cam, 2))
  nc = (nx + 3) * (ny + 3) + 2
  G, A = np.empty((n_cam, n_folds, nc, nc)), np.empty((n_cam, n_folds, nc, nc))
  count, outside = np.empty((n_cam, n_folds), dtype=np.int64), np.empty(n_cam, dtype=np.int64)
  cw, ch = (0, 0) if coverage is None else coverage
  cov = None if coverage is None else np.empty((n_cam, 2, ch, cw), dtype=np.int32)
  entry("residual_gram")(n_cam, F, B, P, dp(proj), dp(obs), up(va), up(inl), ip(size), nx, ny, n_folds, 1 if inliers_only else 0,
                         dp(G), dp(A), count.ctypes.data_as(c_int64_p), outside.ctypes.data_as(c_int64_p), cw, ch, ip(cov))
  return struct(gram=G, absgram=A, count=count, outside=outside, coverage=cov)


def bound(absgram, count):
  """entry-wise |G - G'| <= 4 n 2^-53 A: the standard bound of two summations of the same n products per entry (each within
  n u sum |products|, u = 2^-53, and as much again for the products themselves and second-order terms), per (camera, fold)"""
  return 4.0 * np.asarray(count, dtype=np.float64)[..., None, None] * 2.0 ** -53 * absgram


def worst_ratio(G, ref):
  """max over the entries of |G - ref.gram| / bound (0 where both are exactly equal)"""
  diff, lim = np.abs(G - ref.gram), bound(ref.absgram, ref.count)
  with np.errstate(divide="ignore", invalid="ignore"):
    ratio = np.where(diff == 0.0, 0.0, diff / lim)
  return float(ratio.max()) if ratio.size else 0.0


def image_sizes(rig):
  return [tuple(int(v) for v in cam.image_size) for cam in rig.init.cameras]


@functools.lru_cache(maxsize=None)
def tables(name):
  """struct(projected, observed [C,F,B,P,2], valid, inlier [C,F,B,P], sizes) of a golden fixture at its stored x0: the projected
  points are the observed ones plus the fixture's stored residuals r0 (inliers0 in the reference's order); valid slots that are not
  inliers carry a zero residual"""
  g, rig = load_golden(name)
  obs, valid, inlier = g["points"].astype(np.float64), g["valid"].astype(bool), g["inliers0"].astype(bool)
  assert g["r0"].size == 2 * inlier.sum() and not (inlier & ~valid).any()
  proj = obs.copy()
  proj[inlier] += g["r0"].reshape(-1, 2)
  for a in (proj, obs, valid, inlier):
    a.setflags(write=False)
  return struct(projected=proj, observed=obs, valid=valid, inlier=inlier, sizes=image_sizes(rig))
