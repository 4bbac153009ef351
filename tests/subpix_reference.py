"""TEST INFRASTRUCTURE: an independent numpy restatement of the corner refinement (csrc/mcba_subpix.h; it shares no code with the
header: scipy's map_coordinates samples, plain numpy sums) and the planted images of the sub-pixel tests."""
import functools

import numpy as np
from scipy import ndimage

OK, MAX_ITER, SINGULAR, LEFT_IMAGE, REVERTED, INVALID = range(6)

HM_A = np.array([[13.1, 1.7, 18.3], [-1.2, 12.4, 14.6], [9e-4, 6e-4, 1.0]])
HM_B = np.array([[41.3, 2.1, 20.7], [-1.9, 39.6, 8.2], [2e-4, 1e-4, 1.0]])
SHAPE = (96, 128)             # H, W
# (half window, start radius) the iteration was measured to converge at from every start, on image A and on image B
CASES_A = [(2, 0.7), (3, 1.0), (5, 2.0), (8, 2.0)]
CASES_B = [(11, 2.0), (15, 2.0)]
STARTS_B = 8                  # starts around the one corner of image B
MAX_ITERATIONS_MEASURED = 21


def _pair(v):
  return (int(v), int(v)) if np.ndim(v) == 0 else (int(v[0]), int(v[1]))


def refine(image, corners, window, zero_zone=-1, max_iter=30, eps=1e-4):
  """(refined [n, 2], status [n], iterations [n], quality [n]) of corners [n, 2] in one grey image [H, W]"""
  img = np.asarray(image).astype(np.float64)
  H, W = img.shape
  wx, wy = _pair(window)
  zx, zy = _pair(zero_zone)
  jj, ii = np.meshgrid(np.arange(-wx, wx + 1), np.arange(-wy, wy + 1))
  m = np.exp(-(ii / wy) ** 2) * np.exp(-(jj / wx) ** 2)
  if zx >= 0 and zy >= 0 and 2 * zx + 1 < 2 * wx + 1 and 2 * zy + 1 < 2 * wy + 1:
    m[(np.abs(ii) <= zy) & (np.abs(jj) <= zx)] = 0.0
  pj, pi = np.meshgrid(np.arange(-wx - 1, wx + 2), np.arange(-wy - 1, wy + 2))
  corners = np.asarray(corners, dtype=np.float64).reshape(-1, 2)
  n = len(corners)
  refined, status = corners.copy(), np.zeros(n, dtype=np.uint8)
  iterations, quality = np.zeros(n, dtype=np.int32), np.full(n, np.nan)
  for k, (x0, y0) in enumerate(corners):
    if not (np.isfinite(x0) and np.isfinite(y0) and 0 <= x0 < W and 0 <= y0 < H):
      status[k] = INVALID
      continue
    c = np.array([x0, y0])
    st = MAX_ITER
    for it in range(1, max_iter + 1):
      S = ndimage.map_coordinates(img, [c[1] + pi, c[0] + pj], order=1, mode="nearest")
      gx = S[1:-1, 2:] - S[1:-1, :-2]
      gy = S[2:, 1:-1] - S[:-2, 1:-1]
      a, b, d = np.sum(m * gx * gx), np.sum(m * gx * gy), np.sum(m * gy * gy)
      p = np.sum(m * (gx * gx * jj + gx * gy * ii))
      q = np.sum(m * (gx * gy * jj + gy * gy * ii))
      iterations[k] = it
      quality[k] = np.linalg.eigvalsh(np.array([[a, b], [b, d]]))[0] / m.sum()
      det = a * d - b * b
      if abs(det) <= np.finfo(np.float64).eps ** 2:
        st = SINGULAR
        break
      step = np.array([d * p - b * q, a * q - b * p]) / det
      c = c + step
      if not (0 <= c[0] < W and 0 <= c[1] < H):
        st = LEFT_IMAGE
        break
      if step @ step <= eps * eps:
        st = OK
        break
    if abs(c[0] - x0) > wx or abs(c[1] - y0) > wy or not np.isfinite(c).all():
      st = REVERTED
    else:
      refined[k] = c
    status[k] = st
  return refined, status, iterations, quality


def render_checker(Hm, n, shape=SHAPE, sub=4):
  """checker of n x n unit squares under the homography Hm (board -> pixel): grey 40 / 210, 210 outside the board, sub x sub
  sub-samples a pixel box-averaged, gaussian_filter(sigma = 1, nearest), rounded to uint8; pixel centres at integer coordinates"""
  H, W = shape
  off = (np.arange(sub) + 0.5) / sub - 0.5
  xs = (np.arange(W)[:, None] + off[None, :]).reshape(-1)
  ys = (np.arange(H)[:, None] + off[None, :]).reshape(-1)
  X, Y = np.meshgrid(xs, ys)
  uvw = np.einsum("ij,jhw->ihw", np.linalg.inv(Hm), np.stack([X, Y, np.ones_like(X)]))
  u, v = uvw[0] / uvw[2], uvw[1] / uvw[2]
  inside = (u >= 0) & (u < n) & (v >= 0) & (v < n)
  dark = inside & ((np.floor(u) + np.floor(v)) % 2 == 0)
  fine = np.where(dark, 40.0, 210.0)
  img = fine.reshape(H, sub, W, sub).mean(axis=(1, 3))
  img = ndimage.gaussian_filter(img, sigma=1.0, mode="nearest")
  return np.rint(img).astype(np.uint8)


def inner_corners(Hm, n):
  """pixel positions [(n - 1)^2, 2] of the inner corners of the board"""
  g = np.arange(1, n)
  b = np.stack([np.tile(g, n - 1), np.repeat(g, n - 1), np.ones((n - 1) ** 2)])
  p = Hm @ b
  return (p[:2] / p[2]).T


def _frozen(*arrays):
  for a in arrays:
    a.setflags(write=False)
  return arrays


@functools.lru_cache(maxsize=None)
def image_a():
  """(image A uint8 [96, 128], its 25 true corners)"""
  return _frozen(render_checker(HM_A, 6), inner_corners(HM_A, 6))


@functools.lru_cache(maxsize=None)
def image_b():
  """(image B uint8 [96, 128], its one true corner repeated STARTS_B times)"""
  return _frozen(render_checker(HM_B, 2), np.repeat(inner_corners(HM_B, 2), STARTS_B, axis=0))


@functools.lru_cache(maxsize=None)
def texture():
  """a smooth random texture uint8 [96, 128] with gradients everywhere, the borders included"""
  rng = np.random.default_rng(5)
  t = ndimage.gaussian_filter(rng.normal(size=SHAPE), sigma=2.0, mode="nearest")
  return _frozen(np.rint(128.0 + 100.0 * t / np.abs(t).max()).astype(np.uint8))[0]


def starts(truth, radius, seed=11):
  """truth plus uniform noise of that radius per axis"""
  rng = np.random.default_rng(seed)
  return truth + rng.uniform(-radius, radius, size=truth.shape)


def planted_cases():
  """[(name, image uint8, truth [n, 2], half window, start radius)] of the measured cases"""
  A, tA = image_a()
  B, tB = image_b()
  return [(f"A-w{w}", A, tA, w, r) for w, r in CASES_A] + [(f"B-w{w}", B, tB, w, r) for w, r in CASES_B]


def as_dtype(image, dtype):
  return np.ascontiguousarray(np.asarray(image).astype(dtype))


@functools.lru_cache(maxsize=None)
def reference_run(case, fixed):
  """the restatement on planted case number `case`: fixed count (eps = 0, 30 iterations) or the reference's criteria.  Images of both
  dtypes hold the same values, so one run serves both."""
  name, img, truth, w, r = planted_cases()[case]
  out = refine(img, starts(truth, r), w, max_iter=30, eps=0.0 if fixed else 1e-4)
  return _frozen(*out)
