"""TEST INFRASTRUCTURE: an independent numpy / scipy restatement of projection, undistortion, undistortion maps and the bicubic
remap -- it does not read csrc/mcba_undistort.h.

  forward     the restated cv2.projectPoints / cv2.fisheye.projectPoints of oracle/shims/cv2 (float64);
  inverse     scipy.optimize.least_squares on that forward function, one pixel at a time;
  maps        float32(forward(iR [u v 1])), iR = inv(P R) by numpy;
  remap       OpenCV's bicubic kernel (A = -0.75) and a constant border, evaluated in float64 from the float32 coordinates.
"""
import numpy as np
from scipy.optimize import least_squares

from oracle.shims import cv2 as cv2_restated


def is_fisheye(camera):
  return type(camera).__name__ == "CameraFisheye"


def project(camera, X):
  """pixels [n, 2] of camera-frame points [n, 3]"""
  X = np.asarray(X, dtype=np.float64).reshape(-1, 1, 3)
  f = cv2_restated.fisheye.projectPoints if is_fisheye(camera) else cv2_restated.projectPoints
  with np.errstate(all="ignore"):
    uv, _ = f(X, np.zeros(3), np.zeros(3), camera.intrinsic, camera.dist)
  return np.asarray(uv).reshape(-1, 2)


def undistort_normalised(camera, uv):
  """normalised points [n, 2] whose projection is uv [n, 2]: least squares on the forward function, tolerances at rounding"""
  K = np.asarray(camera.intrinsic, dtype=np.float64)
  out = np.zeros((len(uv), 2))
  for i, p in enumerate(np.asarray(uv, dtype=np.float64)):
    start = np.array([(p[0] - K[0, 2]) / K[0, 0], (p[1] - K[1, 2]) / K[1, 1]])
    res = least_squares(lambda q: project(camera, [[q[0], q[1], 1.0]])[0] - p, start, xtol=1e-15, ftol=1e-15, gtol=1e-15)
    out[i] = res.x
  return out


def undistort_points(camera, uv, R=None, P=None):
  xy = undistort_normalised(camera, uv)
  h = np.concatenate([xy, np.ones((len(xy), 1))], axis=1)
  if R is not None:
    h = h @ np.asarray(R).T
    h = h / h[:, 2:]
  if P is not None:
    h = h @ np.asarray(P).T
    h = h / h[:, 2:]
  return h[:, :2]


def undistort_map(camera, image_size, R=None, P=None):
  """[H, W, 2] float32; NaN where the pixel looks behind the camera"""
  w, h = image_size
  P = np.asarray(camera.intrinsic if P is None else P, dtype=np.float64)
  iR = np.linalg.inv(P @ (np.eye(3) if R is None else np.asarray(R, dtype=np.float64)))
  u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
  rays = np.stack([u, v, np.ones_like(u)], axis=-1).reshape(-1, 3) @ iR.T
  uv = project(camera, rays)
  uv[~(rays[:, 2] > 0) | ~np.isfinite(uv).all(axis=1)] = np.nan
  return uv.astype(np.float32).reshape(h, w, 2)


def cubic_weights(t):
  """[..., 4] weights of the taps floor - 1 .. floor + 2 (OpenCV's interpolateCubic), float64"""
  A = -0.75
  t = np.asarray(t, dtype=np.float64)
  w0 = ((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A
  w1 = ((A + 2) * t - (A + 3)) * t * t + 1
  s = 1 - t
  w2 = ((A + 2) * s - (A + 3)) * s * s + 1
  return np.stack([w0, w1, w2, 1 - w0 - w1 - w2], axis=-1)


def remap(image, coords, border=0.0):
  """float64 bicubic sample of image [Hs, Ws(, CH)] at the float32 coordinates coords [Hd, Wd, 2]; no rounding, no saturation.
  A coordinate that is not finite, or whose taps all lie outside, gives the border value."""
  img = np.asarray(image, dtype=np.float64)
  img = img[..., None] if img.ndim == 2 else img
  hs, ws, ch = img.shape
  c = np.asarray(coords, dtype=np.float32).astype(np.float64)
  mx, my = c[..., 0], c[..., 1]
  with np.errstate(invalid="ignore"):
    dead = ~(np.isfinite(mx) & np.isfinite(my) & (mx >= -2) & (mx < ws + 1) & (my >= -2) & (my < hs + 1))
  mx, my = np.where(dead, 0.0, mx), np.where(dead, 0.0, my)
  fx, fy = np.floor(mx), np.floor(my)
  # the fractional part as the float32 difference the kernel forms (exact: both operands are float32 and close)
  wx, wy = cubic_weights((mx - fx).astype(np.float32)), cubic_weights((my - fy).astype(np.float32))
  ix, iy = fx.astype(np.int64) - 1, fy.astype(np.int64) - 1
  padded = np.full((hs + 8, ws + 8, ch), float(border))
  padded[4:4 + hs, 4:4 + ws] = img
  out = np.zeros(c.shape[:-1] + (ch,))
  for j in range(4):
    for i in range(4):
      out += (wy[..., j] * wx[..., i])[..., None] * padded[iy + j + 4, ix + i + 4]
  out[dead] = float(border)
  return out[..., 0] if np.asarray(image).ndim == 2 else out
