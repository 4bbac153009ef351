"""TEST INFRASTRUCTURE: an independent numpy restatement of the triangulation -- it does not read csrc/mcba_triangulate.h.

  projection  the restated cv2.projectPoints / cv2.fisheye.projectPoints of undistort_reference (float64);
  inverse     Newton on that projection with a central-difference 2 x 2 Jacobian, all pixels of a camera at once;
  start       the plane intersection of DESIGN.md section 3.12 in numpy;
  refinement  damped Gauss-Newton on the pixel residuals with a CENTRAL-DIFFERENCE 2 x 3 Jacobian (step 1e-5 m), all points of a
              problem at once, run until no point moves by more than 1e-12 px (whitened) or 12 rounds.
Its own floor is the truncation and rounding of the differences: the whitened gradient at its optimum is about 1e-11 px (2e-10 px with a step of 1e-6 m).
"""
import numpy as np

import undistort_reference as ref

FD_STEP = 1e-5          # metres


def undistort(camera, uv, rounds=30):
  """([n, 2] normalised points, [n] converged): Newton on the restated projection"""
  uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
  K = np.asarray(camera.intrinsic, dtype=np.float64)
  xy = (uv - [K[0, 2], K[1, 2]]) / [K[0, 0], K[1, 1]]
  h = 1e-6

  def f(q):
    return ref.project(camera, np.concatenate([q, np.ones((len(q), 1))], axis=1)) - uv
  ok = np.isfinite(uv).all(axis=1)
  xy = np.where(ok[:, None], xy, 0.0)
  with np.errstate(all="ignore"):
    for _ in range(rounds):
      r = f(xy)
      J = np.stack([(f(xy + [h, 0.0]) - f(xy - [h, 0.0])) / (2 * h), (f(xy + [0.0, h]) - f(xy - [0.0, h])) / (2 * h)], axis=-1)
      det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
      ok &= det > 0
      step = np.stack([J[:, 1, 1] * r[:, 0] - J[:, 0, 1] * r[:, 1], J[:, 0, 0] * r[:, 1] - J[:, 1, 0] * r[:, 0]], axis=1) / det[:, None]
      xy = np.where(ok[:, None], xy - step, 0.0)
    ok &= np.abs(f(xy)).max(axis=1) < 1e-8
  return xy, ok


class Problem(object):
  """One call flattened to N = F * M points: obs [N, C, 2], matrices [N, C, 3, 4] (the lerp of every observation's own row under
  rolling shutter), usable [N, C]."""

  def __init__(self, cameras, views, points, valid, views_end=None, view_valid=None):
    self.cameras = list(cameras)
    views = np.asarray(views, dtype=np.float64)[:, :, :3, :]
    C, F = views.shape[:2]
    points = np.asarray(points, dtype=np.float64)
    M = points.shape[2]
    self.C, self.F, self.M = C, F, M
    ok = np.asarray(valid).astype(bool) & np.isfinite(points).all(axis=-1)
    if view_valid is not None:
      ok &= np.asarray(view_valid).astype(bool)[:, :, None]
    mats = np.broadcast_to(views[:, :, None], (C, F, M, 3, 4)).copy()
    if views_end is not None:
      end = np.asarray(views_end, dtype=np.float64)[:, :, :3, :]
      heights = np.array([c.image_size[1] for c in self.cameras], dtype=np.float64)
      t = np.where(ok, points[..., 1], 0.0) / heights[:, None, None]
      mats = (1.0 - t)[..., None, None] * views[:, :, None] + t[..., None, None] * end[:, :, None]
    self.rays = np.zeros((C, F, M, 2))
    for c, cam in enumerate(self.cameras):
      xy, good = undistort(cam, np.where(ok[c][..., None], points[c], 0.0).reshape(-1, 2))
      self.rays[c] = xy.reshape(F, M, 2)
      ok[c] &= good.reshape(F, M)
    N = F * M
    self.obs = np.moveaxis(points, 0, 2).reshape(N, C, 2)
    self.mats = np.moveaxis(mats, 0, 2).reshape(N, C, 3, 4)
    self.rays = np.moveaxis(self.rays, 0, 2).reshape(N, C, 2)
    self.usable = np.moveaxis(ok, 0, 2).reshape(N, C)
    self.n_views = self.usable.sum(axis=1)

  # ---- the start ----------------------------------------------------------------------------------------------------------
  def linear_start(self):
    """([N, 3], [N] solvable): intersection of the unit-normal planes of the usable views"""
    m = self.mats
    rows = np.stack([m[:, :, 0] - self.rays[..., :1] * m[:, :, 2], m[:, :, 1] - self.rays[..., 1:] * m[:, :, 2]], axis=2)   # [N,C,2,4]
    rows = rows / np.linalg.norm(rows[..., :3], axis=-1, keepdims=True)
    rows = rows * self.usable[:, :, None, None]
    Nm = np.einsum('ncki,nckj->nij', rows[..., :3], rows[..., :3])
    b = -np.einsum('ncki,nck->ni', rows[..., :3], rows[..., 3])
    X = np.full((len(m), 3), np.nan)
    solvable = self.n_views >= 2
    with np.errstate(all="ignore"):
      ev = np.linalg.eigvalsh(Nm)
    solvable &= ev[:, 0] > 1e-12 * ev.sum(axis=1)
    X[solvable] = np.linalg.solve(Nm[solvable], b[solvable][..., None])[..., 0]
    return X, solvable

  # ---- residuals and their differences ------------------------------------------------------------------------------------------
  def depths(self, X):
    return np.einsum('ncj,nj->nc', self.mats[:, :, 2, :3], X) + self.mats[:, :, 2, 3]

  def residuals(self, X):
    """[N, C, 2] pixels, 0 where the view is not usable"""
    Xc = np.einsum('ncij,nj->nci', self.mats[..., :3], X) + self.mats[..., 3]
    r = np.zeros_like(self.obs)
    for c, cam in enumerate(self.cameras):
      u = self.usable[:, c]
      if u.any():
        r[u, c] = ref.project(cam, Xc[u, c]) - self.obs[u, c]
    return r

  def normal_equations(self, X):
    """H [N, 3, 3], g [N, 3], sse [N], r at X; central differences"""
    r = self.residuals(X)
    J = np.zeros(r.shape + (3,))
    for k in range(3):
      e = np.zeros(3)
      e[k] = FD_STEP
      J[..., k] = (self.residuals(X + e) - self.residuals(X - e)) / (2 * FD_STEP)
    H = np.einsum('ncki,nckj->nij', J, J)
    g = np.einsum('ncki,nck->ni', J, r)
    return H, g, (r * r).sum(axis=(1, 2)), r

  def refine(self, X0, rounds=12):
    """damped Gauss-Newton from X0 [N, 3] (rows of NaN stay NaN); returns X"""
    X = np.array(X0, dtype=np.float64)
    live = np.isfinite(X).all(axis=1)
    idx = np.nonzero(live)[0]
    sub = self.subset(idx)
    x = X[idx]
    lam = np.full(len(x), 1e-6)
    H, g, cost, _ = sub.normal_equations(x)
    for _ in range(rounds):
      Hd = H + lam[:, None, None] * (H * np.eye(3))
      d = np.linalg.solve(Hd, -g[..., None])[..., 0]
      q = x + d
      Hq, gq, cq, _ = sub.normal_equations(q)
      # (from the linear start Gauss-Newton only descends; the test keeps a step that diverges out.  The slack is far above the
      #  rounding of the cost: a point at its optimum must keep moving with the gradient, not with the noise of the cost)
      better = cq <= cost * (1.0 + 1e-9) + 1e-20
      whitened = np.sqrt(np.einsum('ni,nij,nj->n', d, H, d))
      x = np.where(better[:, None], q, x)
      H = np.where(better[:, None, None], Hq, H)
      g = np.where(better[:, None], gq, g)
      cost = np.where(better, cq, cost)
      lam = np.where(better, np.maximum(lam * 0.1, 1e-15), np.minimum(lam * 10.0, 1e30))
      if (whitened[better] <= 1e-12).all() and better.all():
        break
    X[idx] = x
    return X

  def subset(self, idx):
    p = object.__new__(Problem)
    p.cameras, p.C = self.cameras, self.C
    p.obs, p.mats, p.rays, p.usable, p.n_views = self.obs[idx], self.mats[idx], self.rays[idx], self.usable[idx], self.n_views[idx]
    return p


def whitened_norm(H, v):
  """|L^T v| with H = L L^T: the length of the displacement v [N, 3] in pixels"""
  return np.sqrt(np.maximum(np.einsum('ni,nij,nj->n', v, H, v), 0.0))


def whitened_gradient(H, g):
  """|L^-1 g| with H = L L^T"""
  return np.sqrt(np.maximum(np.einsum('ni,ni->n', g, np.linalg.solve(H, g[..., None])[..., 0]), 0.0))
