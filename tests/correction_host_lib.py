"""TEST INFRASTRUCTURE: ctypes wrapper of tests/correction_host (g++ build of multical_amd/csrc/mcba_warp.h, the mathematics of the
corrected entry points) + the fields and rigs the correction tests share."""
import copy
import ctypes as C
import functools

import numpy as np

import host_build
from multical_amd import correction, synthetic
from multical_amd._lib import c_double_p, dp
from multical_amd.correction import FieldCorrection

NAMES = ["warp_points", "undistort_maps_corrected", "undistort_images_corrected"]
_host = host_build.HostLib("correction_host", "ch", NAMES, extra={
  "field_value_jacobian": [C.c_int64, c_double_p, c_double_p, C.c_double, C.c_double, C.c_int32, C.c_int32, c_double_p, c_double_p,
                           c_double_p],
  "fold_bound": [c_double_p, C.c_double, C.c_double, C.c_int32, C.c_int32, c_double_p],
}, module=correction)
lib, build, entry, host_backend, on_host = _host.lib, _host.build, _host.entry, _host.host_backend, _host.on_host

GRIDS = [(1, 1), (2, 3), (5, 4), (7, 3)]
IMAGE_SIZE = (200, 150)
U = 2.0 ** -53


def field_value_jacobian(coef, pixels, image_size, nx, ny):
  """(e [n, 2] of field_value_jacobian, De [n, 2, 2], e [n, 2] of field_value) of finite pixels [n, 2] in one camera's field"""
  px = np.ascontiguousarray(np.asarray(pixels, dtype=np.float64).reshape(-1, 2))
  coef = np.ascontiguousarray(np.asarray(coef, dtype=np.float64))
  e, J, e_only = np.empty((len(px), 2)), np.empty((len(px), 4)), np.empty((len(px), 2))
  entry("field_value_jacobian")(len(px), dp(px), dp(coef), float(image_size[0]), float(image_size[1]), int(nx), int(ny), dp(e), dp(J),
                                dp(e_only))
  return e, J.reshape(-1, 2, 2), e_only


def fold_bound(coef, image_size, nx, ny):
  coef, L = np.ascontiguousarray(np.asarray(coef, dtype=np.float64)), C.c_double()
  entry("fold_bound")(dp(coef), float(image_size[0]), float(image_size[1]), int(nx), int(ny), C.byref(L))
  return L.value


def random_field(seed, sizes, nx, ny, sigma=1.0):
  """FieldCorrection with N(0, sigma px) control values for cameras of those image sizes"""
  rng = np.random.default_rng(seed)
  return FieldCorrection(sigma * rng.normal(size=(len(sizes), (nx + 3) * (ny + 3), 2)), sizes, nx, ny)


def scaled(field, factor):
  return FieldCorrection(field.coefficients * factor, field.image_sizes, field.nx, field.ny)


def zero_field(sizes, nx=5, ny=4):
  return FieldCorrection(np.zeros((len(sizes), (nx + 3) * (ny + 3), 2)), sizes, nx, ny)


def edge_pixels(image_size, nx, ny):
  """pixels on every cell boundary u = k W / nx, v = k H / ny and on all four edges"""
  W, H = image_size
  us, vs = np.arange(nx + 1) * W / nx, np.arange(ny + 1) * H / ny
  on_u = [(u, v) for u in us for v in (0.0, 0.37 * H, float(H))]
  on_v = [(u, v) for v in vs for u in (0.0, 0.61 * W, float(W))]
  edges = [(u, v) for u in np.linspace(0.0, W, 9) for v in (0.0, float(H))] + [(u, v) for v in np.linspace(0.0, H, 9) for u in (0.0, float(W))]
  return np.array(on_u + on_v + edges, dtype=np.float64)


def point_cases(sizes, nx, ny, n, seed):
  """(pixels [n, 2], camera_of [n]): cameras interleaved per point; cell boundaries and edges, pixels outside by 0.5 and 20, NaN and
  +-inf first, random pixels in and around the image after them -- cut or filled to n points"""
  rng = np.random.default_rng(seed)
  of = (np.arange(n) % len(sizes)).astype(np.int32)
  W, H = np.array(sizes, dtype=np.float64)[of].T
  px = np.stack([rng.uniform(-20.0, W + 20.0), rng.uniform(-20.0, H + 20.0)], axis=1)
  special = []
  for c, size in enumerate(sizes):
    w, h = float(size[0]), float(size[1])
    pts = list(edge_pixels(size, nx, ny)) + [(-0.5, 3.0), (w + 0.5, 3.0), (3.0, -0.5), (3.0, h + 0.5), (-20.0, -20.0), (w + 20.0, h + 20.0),
                                              (np.nan, 1.0), (1.0, np.nan), (np.inf, 1.0), (1.0, -np.inf), (-np.inf, np.inf)]
    special += [(c, p) for p in pts]
  slots = {c: list(np.flatnonzero(of == c)) for c in range(len(sizes))}
  for c, p in special:
    if slots[c]:
      px[slots[c].pop(0)] = p
  return px, of


# frames and seed: both cameras see boards in every sixteenth of the image.  The fit of the exact case runs with sigma2 = 1e-12 and, as
# the planted-exact test of the residual field does, prior_px = tau0 = 1e9: the penalty is then 1e-30 of B^T B and really vanishes (at
# the default priors 1e-12 L^T L still moves the weakest direction of B^T B, cond 1e9, by 1e-4 px).
PLANTED = dict(config="tiny", frames=48, seed=5, noise=0.2, nx=1, ny=1, amplitude=0.5)
EXACT_FIT = dict(sigma2=1e-12, prior_px=1e9, tau0=1e9)


@functools.lru_cache(maxsize=None)
def planted_exact():
  """The exact planted case: struct of the noise-free detections of a static rig with truth (`exact` [C,F,B,P,2], valid), a planted
  in-span field of 0.5 px control values (`field`, fold bound below 0.2) and the raw observations `raw` = w^-1(exact) through the
  host build: at the truth parameters the residual projected - observed is exactly e(raw)."""
  from multical_amd.structs import struct
  p = PLANTED
  rig = synthetic.make_rig(p["config"], frames=p["frames"], seed=p["seed"], noise=0.0, outlier_frac=0.0)
  sizes = [tuple(int(v) for v in cam.image_size) for cam in rig.init.cameras]
  field = random_field(3, sizes, p["nx"], p["ny"], p["amplitude"])
  assert field.fold_bound().max() < 0.2
  C_, F, B, P = rig.valid.shape
  of = np.repeat(np.arange(C_, dtype=np.int32), F * B * P)
  flat = np.where(rig.valid.reshape(-1, 1), rig.points.reshape(-1, 2), 0.0)
  raw, status = on_host(field.uncorrect, flat, of)
  assert (status == 0).all()
  raw = np.where(rig.valid[..., None], raw.reshape(rig.points.shape), rig.points)
  for a in (raw, rig.points, rig.valid):
    a.setflags(write=False)
  return struct(rig=rig, sizes=sizes, field=field, exact=rig.points, valid=rig.valid, raw=raw)


def rig_with_points(rig, points):
  """a copy of a synthetic rig with another observation table"""
  out = copy.copy(rig)
  out.points = np.array(points, dtype=np.float64)
  return out
