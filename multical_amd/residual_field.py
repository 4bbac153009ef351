"""Residual fields: is what bundle_adjust leaves behind noise, or a smooth function of the pixel?  

Per camera a tensor-product uniform cubic B-spline field e(u, v) in R^2 over the image is fitted to the residuals r = projected -
observed as a function of the OBSERVED pixel.  The device makes one pass over the observation table (mcba_residual_gram,
csrc/mcba_residual_field_kernels.h) and returns, per (camera, fold = frame mod n_folds), the Gram matrix of the rows [b(u, v) | r_x |
r_y]: B^T B, B^T r and r^T r in one symmetric NC x NC block, NC = (nx + 3)(ny + 3) + 2 <= 64.  Everything below is numpy on those
blocks, matrices of at most 62 x 62:

  coefficients     c = (B^T B + Pen)^-1 B^T r per component, by Cholesky
  penalty          Pen = (sigma2 / tau^2) L^T L + (sigma2 / tau0^2) I, L = second differences of the control grid along x and y
  rms              all of the residual at the observations, sqrt(r^T r / n) (the RMS `report` prints)
  systematic_rms   the fitted field at the observations, sqrt(c^T B^T B c / n)
  explained        1 - SSE(c) / SSE(0),  SSE(c) = r^T r - 2 c^T B^T r + c^T B^T B c  (in-sample: never negative for Pen -> 0)
  cv_gain          1 - sum_k SSE_k(c_-k) / sum_k SSE_k(0): c_-k fitted WITHOUT fold k (from G - G_k), SSE_k from G_k alone -- the share of
                   the held-out frames' squared error the field predicts; about 0 or negative when the residual is noise
  z                (T - nu) / sqrt(2 nu),  T = sum over components of (B^T r)^T (B^T B + Pen)^-1 (B^T r) / sigma2,
                   nu = 2 tr(B^T B (B^T B + Pen)^-1): how far the fitted energy is above what noise of variance sigma2 puts there

MODELLING CHOICES (not derived from the data): tau = prior_px (default 1 px) is the second difference of neighbouring control
values one thinks plausible; tau0 = 100 px only makes the system positive definite where a camera never saw a board; sigma2 is the
caller's, or the estimate |r|^2 / (m - p_free) that Calibration.covariance uses.
"""
import numpy as np
import scipy.linalg

from . import _lib
from .structs import struct
from .uncertainty import grid_of

DEFAULT_GRID = (16, 12)
TAU0 = 100.0
# REPORTING CONVENTIONS of report_residual_field (not tests of a hypothesis): a camera is flagged when the field predicts more than a
# tenth of the held-out squared error AND its energy is more than five standard deviations above the noise level
WARN_CV_GAIN, WARN_Z = 0.1, 5.0


def n_control(nx, ny):
  return (nx + 3) * (ny + 3)


def cubic_weights(t):
  """[..., 4] cubic B-spline weights of the fraction t (the formulas of csrc/mcba_residual_field.h)"""
  t = np.asarray(t, dtype=np.float64)
  m = 1.0 - t
  return np.stack([m * m * m, (3.0 * t - 6.0) * t * t + 4.0, ((-3.0 * t + 3.0) * t + 3.0) * t + 1.0, t * t * t], axis=-1) / 6.0


def cell(u, extent, n):
  """(interval [...], fraction [...]) of coordinate u of an image of that extent cut into n intervals (the far edge: last, 1)"""
  s = np.asarray(u, dtype=np.float64) * n / float(extent)
  i = np.clip(np.floor(s), 0, n - 1)
  return i.astype(np.int64), s - i


def basis(pixels, image_size, nx, ny):
  """dense rows b(u, v) [n, K] of pixels [n, 2] (NaN rows for pixels outside the image)"""
  px = np.asarray(pixels, dtype=np.float64).reshape(-1, 2)
  (W, H), K = image_size, n_control(nx, ny)
  inside = (px[:, 0] >= 0) & (px[:, 0] <= W) & (px[:, 1] >= 0) & (px[:, 1] <= H)
  q = np.where(inside[:, None], px, 0.0)
  (ix, tx), (iy, ty) = cell(q[:, 0], W, nx), cell(q[:, 1], H, ny)
  wx, wy = cubic_weights(tx), cubic_weights(ty)
  out = np.zeros((px.shape[0], K))
  rows = np.arange(px.shape[0])
  for a in range(4):
    for b in range(4):
      out[rows, (iy + a) * (nx + 3) + ix + b] = wy[:, a] * wx[:, b]
  out[~inside] = np.nan
  return out


def second_differences(nx, ny):
  """L [m, K]: second differences of the control grid along x, then along y"""
  gx, gy = nx + 3, ny + 3
  idx = np.arange(gx * gy).reshape(gy, gx)
  rows = []
  for a, b, c in [(idx[:, :-2], idx[:, 1:-1], idx[:, 2:]), (idx[:-2], idx[1:-1], idx[2:])]:
    for i, j, k in zip(a.ravel(), b.ravel(), c.ravel()):
      row = np.zeros(gx * gy)
      row[i], row[j], row[k] = 1.0, -2.0, 1.0
      rows.append(row)
  return np.array(rows)


def penalty(nx, ny, sigma2, prior_px=1.0, tau0=TAU0):
  L = second_differences(nx, ny)
  return (sigma2 / prior_px ** 2) * (L.T @ L) + (sigma2 / tau0 ** 2) * np.eye(n_control(nx, ny))


def sse(G, c):
  """SSE(c) of both components from one Gram block G [NC, NC] and coefficients c [K, 2]"""
  K = G.shape[0] - 2
  BtB, Btr = G[:K, :K], G[:K, K:]
  return float(G[K, K] + G[K + 1, K + 1] - 2.0 * np.sum(c * Btr) + np.sum(c * (BtB @ c)))


def solve(G, pen):
  """(c [K, 2], Cholesky factor of B^T B + Pen) of a Gram block"""
  K = G.shape[0] - 2
  factor = scipy.linalg.cho_factor(G[:K, :K] + pen, lower=True)
  return scipy.linalg.cho_solve(factor, G[:K, K:]), factor


def fit_camera(gram, count, nx, ny, sigma2, prior_px=1.0, tau0=TAU0):
  """The algebra of one camera: gram [n_folds, NC, NC], count [n_folds] -> struct(coefficients [K, 2], factor, n, rms,
  systematic_rms, sse, sse0, explained, cv_gain (NaN with one fold), T, nu, z)"""
  gram = np.asarray(gram, dtype=np.float64)
  K = n_control(nx, ny)
  assert gram.ndim == 3 and gram.shape[1:] == (K + 2, K + 2), f"gram is {gram.shape}, not [n_folds, {K + 2}, {K + 2}]"
  pen = penalty(nx, ny, sigma2, prior_px, tau0)
  G = gram.sum(axis=0)
  n = int(np.sum(count))
  c, factor = solve(G, pen)
  BtB, Btr = G[:K, :K], G[:K, K:]
  sse0, sse_c = float(G[K, K] + G[K + 1, K + 1]), sse(G, c)
  nan = float("nan")
  cv_gain = nan
  if gram.shape[0] > 1 and sse0 > 0.0:
    held = sum(sse(Gk, solve(G - Gk, pen)[0]) for Gk in gram)
    cv_gain = 1.0 - held / sse0
  T = float(np.sum(Btr * c)) / sigma2
  nu = 2.0 * float(np.trace(scipy.linalg.cho_solve(factor, BtB)))
  return struct(coefficients=c, factor=factor, n=n, rms=np.sqrt(sse0 / n) if n else nan,
                systematic_rms=np.sqrt(max(float(np.sum(c * (BtB @ c))), 0.0) / n) if n else nan, sse=sse_c, sse0=sse0,
                explained=1.0 - sse_c / sse0 if sse0 > 0.0 else nan, cv_gain=cv_gain, T=T, nu=nu,
                z=(T - nu) / np.sqrt(2.0 * nu) if nu > 0.0 else nan)


def evaluate(fit, pixels, image_size, nx, ny, sigma2):
  """(field [n, 2], posterior standard deviation [n]) of a camera's fit at pixels [n, 2]; NaN outside the image"""
  b = basis(pixels, image_size, nx, ny)
  ok = ~np.isnan(b[:, 0])
  field, std = np.full((b.shape[0], 2), np.nan), np.full(b.shape[0], np.nan)
  field[ok] = b[ok] @ fit.coefficients
  std[ok] = np.sqrt(sigma2 * np.einsum("ij,ji->i", b[ok], scipy.linalg.cho_solve(fit.factor, b[ok].T)))
  return field, std


def analyse(gram, count, outside, coverage, image_sizes, nx, ny, sigma2, prior_px=1.0, tau0=TAU0, grid=DEFAULT_GRID, pixels=None):
  """The results of `Calibration.residual_field` from the blocks of mcba_residual_gram (gram [C, n_folds, NC, NC], count [C, n_folds],
  outside [C], coverage [C, 2, h, w] or None).  grid=(gw, gh): the field at the centres u_i = (i + 0.5) W / gw - 0.5 of every
  camera, [C, gh, gw, ...]; pixels [n, 2]: at that list instead, [C, n, ...]."""
  sigma2 = float(sigma2)
  assert sigma2 > 0.0 and prior_px > 0.0 and tau0 > 0.0, "residual_field: sigma2, prior_px and tau0 are positive"
  fits, fields, stds, pix = [], [], [], []
  for c, size in enumerate(image_sizes):
    fit = fit_camera(gram[c], count[c], nx, ny, sigma2, prior_px, tau0)
    if pixels is None:
      gw, gh, u0, v0, du, dv = grid_of(size, grid)
      uu, vv = np.meshgrid(u0 + du * np.arange(gw), v0 + dv * np.arange(gh))
      q = np.stack([uu, vv], axis=-1)
    else:
      q = np.asarray(pixels, dtype=np.float64).reshape(-1, 2)
    field, std = evaluate(fit, q.reshape(-1, 2), size, nx, ny, sigma2)
    fits.append(fit)
    fields.append(field.reshape(q.shape))
    stds.append(std.reshape(q.shape[:-1]))
    pix.append(q)
  col = lambda name: np.array([getattr(f, name) for f in fits])
  return struct(coefficients=np.stack([f.coefficients for f in fits]), field=np.stack(fields), field_std=np.stack(stds),
                pixels=np.stack(pix), n=col("n"), rms=col("rms"), systematic_rms=col("systematic_rms"), explained=col("explained"),
                cv_gain=col("cv_gain"), T=col("T"), nu=col("nu"), z=col("z"), sse=col("sse"), sse0=col("sse0"),
                count=np.asarray(count), outside=np.asarray(outside), coverage=coverage, sigma2=sigma2, nx=nx, ny=ny,
                prior_px=float(prior_px), tau0=float(tau0))


def report_lines(result, names, stage=""):
  """one (line, warn) per camera: n, rms, systematic_rms, cv_gain, z, the largest |field| of the map and where it is"""
  out = []
  for c, name in enumerate(names):
    mag = np.linalg.norm(result.field[c], axis=-1)
    if result.n[c] == 0 or not np.isfinite(mag).any():
      out.append((f"{stage} {name}: residual field not defined (no observation entered)", False))
      continue
    worst = np.unravel_index(np.nanargmax(mag), mag.shape)
    at = result.pixels[c][worst]
    warn = bool(result.cv_gain[c] > WARN_CV_GAIN and result.z[c] > WARN_Z)
    out.append((f"{stage} {name}: residual field n={int(result.n[c])} rms={result.rms[c]:.3f} systematic_rms={result.systematic_rms[c]:.3f} "
                f"cv_gain={result.cv_gain[c]:.3f} z={result.z[c]:.1f} max |field|={float(mag[worst]):.3f} px at ({at[0]:.0f}, {at[1]:.0f})"
                + (" -- the residuals of this camera are not noise: its model leaves a smooth error field" if warn else ""), warn))
  return out


def last_call_ms():
  """mcba_debug_residual_gram_ms of this thread's last call: (dict(project, gram, fold, call) in milliseconds, rows that entered)."""
  return _lib.call_ms("residual_gram", ("project", "gram", "fold", "call"))
