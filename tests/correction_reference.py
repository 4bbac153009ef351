"""TEST INFRASTRUCTURE: an independent numpy / scipy restatement of the warp of csrc/mcba_warp.h.

The field is evaluated through scipy.interpolate.BSpline on the extended uniform knot vector (knots k W / nx, k = -3 .. nx + 3: the
nx + 3 cubic B-splines whose supports meet [0, W]), not through the closed-form weights of the product.  The inverse warp is
scipy.optimize.root on p + e(p) = q for point lists, and the fixed-point iteration p <- q - e(p) (a contraction for a fold bound
below 0.2: 26 sweeps shrink any start by 0.2^26 < 1e-18) for whole maps, where a root finder per pixel would take minutes: neither is the product's
Newton iteration.
"""
import numpy as np
from scipy.interpolate import BSpline
from scipy.optimize import root

import undistort_reference


def basis_1d(x, extent, n, derivative=0):
  """[len(x), n + 3] the cubic B-splines (or their derivative) of the extended uniform knots at x in [0, extent]"""
  t = np.arange(-3, n + 4, dtype=np.float64) * (float(extent) / n)
  spl = BSpline(t, np.eye(n + 3), 3, extrapolate=True)
  if derivative:
    spl = spl.derivative(derivative)
  return spl(np.asarray(x, dtype=np.float64))


def field(coef, pixels, image_size, nx, ny):
  """(e [n, 2], De [n, 2, 2]) at pixels [n, 2]: outside the closed image rectangle the field of the clamped pixel, with zero derivative
  in the clamped direction"""
  px = np.asarray(pixels, dtype=np.float64).reshape(-1, 2)
  (W, H), c = image_size, np.asarray(coef, dtype=np.float64).reshape(ny + 3, nx + 3, 2)
  u, v = np.clip(px[:, 0], 0.0, W), np.clip(px[:, 1], 0.0, H)
  bx, by, dbx, dby = basis_1d(u, W, nx), basis_1d(v, H, ny), basis_1d(u, W, nx, 1), basis_1d(v, H, ny, 1)
  dbx = dbx * ((px[:, 0] >= 0.0) & (px[:, 0] <= W))[:, None]
  dby = dby * ((px[:, 1] >= 0.0) & (px[:, 1] <= H))[:, None]
  e = np.einsum("na,nb,abi->ni", by, bx, c)
  J = np.stack([np.einsum("na,nb,abi->ni", by, dbx, c), np.einsum("na,nb,abi->ni", dby, bx, c)], axis=-1)    # [n, component, d/du | d/dv]
  return e, J


def warp_forward(coef, pixels, image_size, nx, ny):
  px = np.asarray(pixels, dtype=np.float64).reshape(-1, 2)
  return px + field(coef, px, image_size, nx, ny)[0]


def warp_inverse_root(coef, pixels, image_size, nx, ny):
  """w^-1 of finite pixels [n, 2], one scipy.optimize.root each"""
  out = np.empty((len(pixels), 2))
  for i, q in enumerate(np.asarray(pixels, dtype=np.float64)):
    # (xtol is relative to |p|: 1e-12 of a few hundred pixels; what is asserted is the equation itself)
    sol = root(lambda p: p + field(coef, p[None], image_size, nx, ny)[0][0] - q, q, method="hybr", tol=1e-12)
    assert np.abs(sol.fun).max() <= 1e-10, (sol.message, sol.fun)
    out[i] = sol.x
  return out


def warp_inverse_sweeps(coef, pixels, image_size, nx, ny, sweeps=26):
  """w^-1 of pixels [n, 2] by p <- q - e(p); NaN rows stay NaN"""
  q = np.asarray(pixels, dtype=np.float64).reshape(-1, 2)
  ok = np.isfinite(q).all(axis=1)
  p = np.full_like(q, np.nan)
  cur = q[ok].copy()
  for _ in range(sweeps):
    cur = q[ok] - field(coef, cur, image_size, nx, ny)[0]
  p[ok] = cur
  return p


def corrected_map(camera, image_size, coef, field_size, nx, ny, R=None, P=None):
  """[H, W, 2] float32: w^-1 of the FP64 coordinates undistort_reference.undistort_map rounds, NaN where the pixel looks behind the
  camera"""
  w, h = image_size
  P = np.asarray(camera.intrinsic if P is None else P, dtype=np.float64)
  iR = np.linalg.inv(P @ (np.eye(3) if R is None else np.asarray(R, dtype=np.float64)))
  u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
  rays = np.stack([u, v, np.ones_like(u)], axis=-1).reshape(-1, 3) @ iR.T
  uv = undistort_reference.project(camera, rays)
  uv[~(rays[:, 2] > 0) | ~np.isfinite(uv).all(axis=1)] = np.nan
  return warp_inverse_sweeps(coef, uv, field_size, nx, ny).astype(np.float32).reshape(h, w, 2)
