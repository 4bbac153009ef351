"""TEST INFRASTRUCTURE: an independent restatement of the residual field in dense numpy / scipy.

The basis comes from scipy.interpolate.BSpline on the extended uniform knot vector (not from the cubic formulas of the header), the
rows are stacked into a dense matrix R = [B | r_x | r_y], and every quantity of multical_amd.residual_field is recomputed from the
dense B and r directly, fold by fold: least squares on the stacked system [B; Pen^1/2], sums of squared errors from the fitted
values, the trace by an explicit inverse."""
import numpy as np
import scipy.linalg
from scipy.interpolate import BSpline


def basis_1d(u, extent, n):
  """[len(u), n + 3]: the cubic B-splines of the extended uniform knot vector -3 .. n + 3 at the coordinate u n / extent in [0, n].
  (Knots in interval units are exact; in pixel units extent / n is rounded, which moves every knot by up to n ulp and a small
  weight by thousands of ulp of itself -- measured against rational arithmetic -- far outside a summation bound.)"""
  knots = np.arange(-3, n + 4).astype(np.float64)
  return BSpline.design_matrix(np.asarray(u, dtype=np.float64) * n / float(extent), knots, 3).toarray()


def basis(pixels, image_size, nx, ny):
  """dense b(u, v) [n, K], control point (a along y, b along x) in column a (nx + 3) + b"""
  px = np.asarray(pixels, dtype=np.float64).reshape(-1, 2)
  bx, by = basis_1d(px[:, 0], image_size[0], nx), basis_1d(px[:, 1], image_size[1], ny)
  return np.einsum("na,nb->nab", by, bx).reshape(px.shape[0], -1)


def camera_rows(t, c, nx, ny, inliers_only=True):
  """(R [n, K + 2], frame [n], outside) of camera c of tables t (residual_field_host_lib.tables): the rows in slot order"""
  W, H = t.sizes[c]
  mask = t.valid[c] & (t.inlier[c] | (not inliers_only))
  obs = t.observed[c]
  inside = (obs[..., 0] >= 0) & (obs[..., 0] <= W) & (obs[..., 1] >= 0) & (obs[..., 1] <= H)
  take = mask & inside
  f = np.broadcast_to(np.arange(take.shape[0])[:, None, None], take.shape)[take]
  r = (t.projected[c] - obs)[take]
  return np.hstack([basis(obs[take], (W, H), nx, ny), r]), f, int((mask & ~inside).sum())


def dense_gram(t, nx, ny, n_folds, inliers_only=True):
  """(gram [C, n_folds, NC, NC], count [C, n_folds], outside [C]) as R^T R of the dense rows"""
  n_cam, nc = t.valid.shape[0], (nx + 3) * (ny + 3) + 2
  G, count, outside = np.zeros((n_cam, n_folds, nc, nc)), np.zeros((n_cam, n_folds), dtype=np.int64), np.zeros(n_cam, dtype=np.int64)
  for c in range(n_cam):
    R, f, outside[c] = camera_rows(t, c, nx, ny, inliers_only)
    for k in range(n_folds):
      Rk = R[f % n_folds == k]
      G[c, k], count[c, k] = Rk.T @ Rk, Rk.shape[0]
  return G, count, outside


def coverage(t, cov_w, cov_h):
  """[C, 2, cov_h, cov_w]: valid slots inside the image per cell, inliers | valid but not inliers"""
  out = np.zeros((t.valid.shape[0], 2, cov_h, cov_w), dtype=np.int32)
  for c, (W, H) in enumerate(t.sizes):
    obs = t.observed[c]
    inside = (obs[..., 0] >= 0) & (obs[..., 0] <= W) & (obs[..., 1] >= 0) & (obs[..., 1] <= H)
    for plane, mask in enumerate((t.valid[c] & t.inlier[c], t.valid[c] & ~t.inlier[c])):
      q = obs[mask & inside]
      ix = np.minimum(np.floor(q[:, 0] * cov_w / W).astype(int), cov_w - 1)
      iy = np.minimum(np.floor(q[:, 1] * cov_h / H).astype(int), cov_h - 1)
      np.add.at(out[c, plane], (iy, ix), 1)
  return out


def second_differences(nx, ny):
  gx, gy = nx + 3, ny + 3
  rows = []
  for a in range(gy):
    for b in range(gx - 2):
      row = np.zeros((gy, gx))
      row[a, b:b + 3] = 1.0, -2.0, 1.0
      rows.append(row.ravel())
  for a in range(gy - 2):
    for b in range(gx):
      row = np.zeros((gy, gx))
      row[a:a + 3, b] = 1.0, -2.0, 1.0
      rows.append(row.ravel())
  return np.array(rows)


def penalty_root(nx, ny, sigma2, prior_px, tau0):
  """Pen^1/2 as stacked rows: [sigma / tau L; sigma / tau0 I]"""
  K = (nx + 3) * (ny + 3)
  return np.vstack([np.sqrt(sigma2) / prior_px * second_differences(nx, ny), np.sqrt(sigma2) / tau0 * np.eye(K)])


def fit_dense(B, r, root):
  """c [K, 2]: least squares of the stacked system [B; Pen^1/2] c = [r; 0]"""
  A = np.vstack([B, root])
  return np.linalg.lstsq(A, np.vstack([r, np.zeros((root.shape[0], 2))]), rcond=None)[0]


def analyse_dense(R, frame, n_folds, nx, ny, sigma2, prior_px=1.0, tau0=100.0):
  """dict(c, sse, sse0, explained, cv_gain, T, nu, z, rms, systematic_rms) of one camera from its dense rows"""
  K = (nx + 3) * (ny + 3)
  B, r = R[:, :K], R[:, K:]
  root = penalty_root(nx, ny, sigma2, prior_px, tau0)
  c = fit_dense(B, r, root)
  sse0, sse = float(np.sum(r * r)), float(np.sum((r - B @ c) ** 2))
  held = 0.0
  for k in range(n_folds):
    out = frame % n_folds == k
    ck = fit_dense(B[~out], r[~out], root)
    held += float(np.sum((r[out] - B[out] @ ck) ** 2))
  M = np.linalg.inv(B.T @ B + root.T @ root)
  Btr = B.T @ r
  T = float(np.sum(Btr * (M @ Btr))) / sigma2
  nu = 2.0 * float(np.trace(B.T @ B @ M))
  n = R.shape[0]
  return dict(c=c, sse=sse, sse0=sse0, explained=1.0 - sse / sse0, cv_gain=1.0 - held / sse0, T=T, nu=nu, z=(T - nu) / np.sqrt(2.0 * nu),
              rms=np.sqrt(sse0 / n), systematic_rms=np.sqrt(float(np.sum((B @ c) ** 2)) / n))
