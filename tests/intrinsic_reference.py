"""TEST INFRASTRUCTURE: an independent numpy / scipy restatement of single-camera intrinsic calibration, the yardstick of
multical_amd/csrc/mcba_intrinsic.h.  Nothing of the header is used: the projection below is written from the model equations
(Brown-Conrady with rational, thin-prism and tilt terms as cv2.projectPoints documents them; Kannala-Brandt as
cv2.fisheye.projectPoints), the Jacobian is its COMPLEX-STEP derivative (exact to rounding, no step-size error -- 2-point
differences leave K undetermined at 1e-4 .. 1e-3 px), and the optimiser is scipy's least_squares (trf, x_scale='jac',
ftol = xtol = gtol = 1e-15) followed by exact Gauss-Newton steps on the same Jacobian (Problem.solve says why)."""
import numpy as np
from scipy.optimize import least_squares

from multical_amd.structs import struct

MODELS = dict(standard=(5, False), rational=(8, False), thin_prism=(12, False), tilted=(14, False), pin4=(4, False),
              fisheye=(4, True))
STEP = 1e-30


def rotation(w):
  """Rodrigues' formula, valid for complex arguments; w [..., 3] -> [..., 3, 3]."""
  w = np.asarray(w)
  t2 = (w * w).sum(axis=-1)
  t2 = np.where(np.abs(t2) < 1e-300, 1e-300, t2)
  t = np.sqrt(t2)
  a, b = np.sin(t) / t, (1 - np.cos(t)) / t2
  x, y, z = w[..., 0], w[..., 1], w[..., 2]
  zero = np.zeros_like(x)
  K = np.stack([np.stack([zero, -z, y], -1), np.stack([z, zero, -x], -1), np.stack([-y, x, zero], -1)], -2)
  return np.eye(3) + a[..., None, None] * K + b[..., None, None] * (K @ K)


def tilt_matrix(tx, ty):
  cx, sx, cy, sy = np.cos(tx), np.sin(tx), np.cos(ty), np.sin(ty)
  one, zero = np.ones_like(cx), np.zeros_like(cx)
  rx = np.array([[one, zero, zero], [zero, cx, sx], [zero, -sx, cx]])
  ry = np.array([[cy, zero, -sy], [zero, one, zero], [sy, zero, cy]])
  r = ry @ rx
  pz = np.array([[r[2, 2], zero, -r[0, 2]], [zero, r[2, 2], -r[1, 2]], [zero, zero, one]])
  return pz @ r


def project(f, c, k, fisheye, X):
  """f [2], c [2], k [nd], X [n, 3] camera-frame points -> [n, 2] pixels."""
  x, y = X[:, 0] / X[:, 2], X[:, 1] / X[:, 2]
  r2 = x * x + y * y
  if fisheye:
    r = np.sqrt(r2)
    th = np.arctan(r)
    th2 = th * th
    s = th * (1 + k[0] * th2 + k[1] * th2**2 + k[2] * th2**3 + k[3] * th2**4) / r
    xd, yd = x * s, y * s
  else:
    kk = np.zeros(14, dtype=np.result_type(k, X))
    kk[:len(k)] = k
    r4, r6 = r2 * r2, r2 * r2 * r2
    radial = (1 + kk[0] * r2 + kk[1] * r4 + kk[4] * r6) / (1 + kk[5] * r2 + kk[6] * r4 + kk[7] * r6)
    xd = x * radial + 2 * kk[2] * x * y + kk[3] * (r2 + 2 * x * x) + kk[8] * r2 + kk[9] * r4
    yd = y * radial + kk[2] * (r2 + 2 * y * y) + 2 * kk[3] * x * y + kk[10] * r2 + kk[11] * r4
    if len(k) == 14:
      T = tilt_matrix(kk[12], kk[13])
      vx, vy, vz = (T[i, 0] * xd + T[i, 1] * yd + T[i, 2] for i in range(3))
      xd, yd = vx / vz, vy / vz
  return np.stack([f[0] * xd + c[0], f[1] * yd + c[1]], axis=-1)


class Problem(object):
  """One camera: views = [(observed [n, 2], board points [n, 3])]; free = bool mask over the model's coefficients."""

  def __init__(self, views, model, fix_aspect=False, free=None, held=None):
    self.nd, self.fisheye = MODELS[model]
    self.views = [(np.asarray(o, dtype=np.float64), np.asarray(X, dtype=np.float64)) for o, X in views]
    self.fix_aspect = fix_aspect
    self.free = np.ones(self.nd, dtype=bool) if free is None else np.asarray(free, dtype=bool)[:self.nd]
    self.held = np.zeros(self.nd) if held is None else np.asarray(held, dtype=np.float64)[:self.nd]   # values of held coefficients
    self.nf = 1 if fix_aspect else 2
    self.ni = self.nf + 2 + int(self.free.sum())
    self.rows = np.cumsum([0] + [2 * len(o) for o, _ in self.views])

  # x = [f (1 or 2) | cx cy | free coefficients | rotation vector, translation per view]
  def pack(self, block, poses):
    f = block[:1] if self.fix_aspect else block[:2]
    return np.concatenate([f, block[2:4], np.asarray(block[5:5 + self.nd])[self.free], np.asarray(poses).ravel()])

  def intrinsics(self, x):
    f = x[[0, 0]] if self.fix_aspect else x[:2]
    k = np.array(self.held, dtype=x.dtype)
    k[self.free] = x[self.nf + 2:self.ni]
    return f, x[self.nf:self.nf + 2], k

  def block(self, x):
    f, c, k = self.intrinsics(np.asarray(x))
    return np.concatenate([f, c, [0.0], k])

  def poses(self, x):
    return np.asarray(x[self.ni:]).reshape(-1, 6)

  def view_residual(self, x, v):
    f, c, k = self.intrinsics(x)
    p = x[self.ni + 6 * v:self.ni + 6 * v + 6]
    obs, X = self.views[v]
    Xc = X @ rotation(p[:3]).T + p[3:]
    return (project(f, c, k, self.fisheye, Xc) - obs).ravel()

  def residual(self, x):
    return np.concatenate([self.view_residual(x, v) for v in range(len(self.views))])

  def jacobian(self, x):
    """Complex step: exact to rounding.  The intrinsic columns one at a time, the six pose columns of all views together."""
    J = np.zeros((self.rows[-1], len(x)))
    xc = np.asarray(x, dtype=np.complex128)
    for j in range(self.ni):
      xs = xc.copy()
      xs[j] += 1j * STEP
      J[:, j] = np.concatenate([self.view_residual(xs, v) for v in range(len(self.views))]).imag / STEP
    for q in range(6):
      xs = xc.copy()
      xs[self.ni + q::6] += 1j * STEP
      for v in range(len(self.views)):
        J[self.rows[v]:self.rows[v + 1], self.ni + 6 * v + q] = self.view_residual(xs, v).imag / STEP
    return J

  def solve(self, block, poses, max_nfev=400, polish=6):
    """block [5 + nd] = [fx fy cx cy skew k...], poses [V, 6] -> struct(block, poses, cost = sum of squares, sse per view, ...)."""
    res = least_squares(self.residual, self.pack(np.asarray(block, dtype=np.float64), poses), jac=self.jacobian, method='trf',
                        x_scale='jac', ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=max_nfev)
    # least_squares ends on ftol with K still 1e-7 .. 1e-5 px from the optimum (the cost no longer resolves the step).  A few exact
    # Gauss-Newton steps on the same Jacobian take it there; a step is kept while the cost does not rise beyond its rounding.
    x, cost = res.x, float(np.sum(self.residual(res.x) ** 2))
    for _ in range(polish):
      d = np.linalg.lstsq(self.jacobian(x), -self.residual(x), rcond=None)[0]
      c = float(np.sum(self.residual(x + d) ** 2))
      if not c <= cost * (1 + 1e-13):
        break
      x, cost = x + d, c
      if np.abs(d[:self.ni]).max() < 1e-12:
        break
    res.x = x
    r = self.residual(res.x)
    sse = np.array([np.sum(r[self.rows[v]:self.rows[v + 1]] ** 2) for v in range(len(self.views))])
    return struct(x=res.x, block=self.block(res.x), poses=self.poses(res.x), cost=float(np.sum(r * r)), sse=sse, nfev=res.nfev,
                  status=res.status)

  def scaled_singular_values(self, x):
    J = self.jacobian(np.asarray(x, dtype=np.float64))
    n = np.linalg.norm(J, axis=0)
    return np.linalg.svd(J / np.where(n > 0, n, 1.0), compute_uv=False)


def pose_matrix(p):
  m = np.eye(4)
  m[:3, :3] = rotation(np.asarray(p[:3], dtype=np.float64))
  m[:3, 3] = p[3:]
  return m


def pose_params(m):
  from scipy.spatial.transform import Rotation
  return np.concatenate([Rotation.from_matrix(np.asarray(m)[:3, :3]).as_rotvec(), np.asarray(m)[:3, 3]])
