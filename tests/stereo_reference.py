"""TEST INFRASTRUCTURE: an independent numpy / scipy restatement of the pairwise stereo calibration -- it does not read
csrc/mcba_stereo.h.

  unknowns    T_rel (left-camera frame -> right-camera frame) and one board pose per view, each as rotation vector | translation,
              rotations through scipy's Rotation.from_rotvec;
  views       the (frame, board) slots with a valid start pose in both cameras and min_common corners valid in both; only the common
              corners enter (tables.matching_points' rule);
  projection  the restated cv2.projectPoints / cv2.fisheye.projectPoints of oracle/shims/cv2 (float64): not a projection written
              here, but one that shares no code with csrc/;
  Jacobian    Richardson-extrapolated central differences of the residuals (steps 1e-4 and 5e-5: the h^2 term cancels, 1e-12
              relative on these rigs); a view's columns are perturbed for all views at once -- a view's residuals depend on its own
              pose only;
  optimum     scipy.optimize.least_squares over all 6 + 6 n_views unknowns with every tolerance at 1e-15;
  covariance  sigma^2 times the T_rel block of (J^T J)^-1, sigma^2 = sse / (4 n_points - 6 - 6 n_views).
"""
import numpy as np
from scipy.optimize import least_squares
from scipy.spatial.transform import Rotation

from oracle.shims import cv2 as cv2_restated


def is_fisheye(camera):
  return type(camera).__name__ == "CameraFisheye" or getattr(camera, "model", None) == "fisheye"


def project(camera, X):
  X = np.asarray(X, dtype=np.float64).reshape(-1, 1, 3)
  f = cv2_restated.fisheye.projectPoints if is_fisheye(camera) else cv2_restated.projectPoints
  with np.errstate(all="ignore"):
    uv, _ = f(X, np.zeros(3), np.zeros(3), camera.intrinsic, camera.dist)
  return np.asarray(uv).reshape(-1, 2)


def to_matrix(x6):
  m = np.eye(4)
  m[:3, :3] = Rotation.from_rotvec(x6[:3]).as_matrix()
  m[:3, 3] = x6[3:6]
  return m


def from_matrix(m):
  return np.concatenate([Rotation.from_matrix(m[:3, :3]).as_rotvec(), m[:3, 3]])


class Pair(object):
  """One pair (l, r) of a case (stereo_host_lib.make_case)."""

  def __init__(self, case, l, r, min_common=4):
    self.case, self.l, self.r = case, l, r
    self.left, self.right = case.cameras[l], case.cameras[r]
    self.views = []     # (f, b, board points [n, 3], left pixels [n, 2], right pixels [n, 2])
    Cn, F, B, P = case.valid.shape
    for f in range(F):
      for b in range(B):
        both = case.valid[l, f, b] & case.valid[r, f, b]
        if case.view_valid[l, f, b] and case.view_valid[r, f, b] and both.sum() >= min_common:
          ids = np.flatnonzero(both)
          self.views.append((f, b, np.asarray(case.board_points[b])[ids], case.points[l, f, b, ids], case.points[r, f, b, ids]))
    self.nv = len(self.views)
    self.n_points = sum(len(v[2]) for v in self.views)
    self.first = np.cumsum([0] + [4 * len(v[2]) for v in self.views])

  def start_vector(self, T_rel, view_poses=None):
    """parameters at T_rel and the given board -> left camera poses (default: the case's start poses)"""
    x = [from_matrix(T_rel)]
    for k, (f, b, _, _, _) in enumerate(self.views):
      x.append(from_matrix(self.case.view_poses[self.l, f, b] if view_poses is None else view_poses[k]))
    return np.concatenate(x)

  def residuals(self, x):
    """per view: left residuals [n, 2] flattened, then right residuals"""
    Trel = to_matrix(x[:6])
    out = []
    for k, (_, _, X, pl, pr) in enumerate(self.views):
      Tv = to_matrix(x[6 + 6 * k:12 + 6 * k])
      Xl = X @ Tv[:3, :3].T + Tv[:3, 3]
      Xr = Xl @ Trel[:3, :3].T + Trel[:3, 3]
      out.append((project(self.left, Xl) - pl).ravel())
      out.append((project(self.right, Xr) - pr).ravel())
    return np.concatenate(out)

  def _central(self, x, step):
    n = 6 + 6 * self.nv
    J = np.zeros((4 * self.n_points, n))
    for k in range(6):
      d = np.zeros(n)
      d[k] = step
      J[:, k] = (self.residuals(x + d) - self.residuals(x - d)) / (2.0 * step)
    for k in range(6):
      d = np.zeros(n)
      d[6 + k::6] = step
      col = (self.residuals(x + d) - self.residuals(x - d)) / (2.0 * step)
      for v in range(self.nv):
        J[self.first[v]:self.first[v + 1], 6 + 6 * v + k] = col[self.first[v]:self.first[v + 1]]
    return J

  def jacobian(self, x, step=1e-4):
    return (4.0 * self._central(x, 0.5 * step) - self._central(x, step)) / 3.0

  def solve(self, x0):
    return least_squares(self.residuals, np.asarray(x0, dtype=np.float64), jac=self.jacobian, x_scale='jac', xtol=1e-15, ftol=1e-15,
                         gtol=1e-15, max_nfev=100)

  def summary(self, x, sigma=None):
    """struct-like dict of T [4, 4], params [6], sse, rms, cov [6, 6], view_poses [nv, 4, 4], view_sse [nv, 2]"""
    r = self.residuals(x)
    sse = float(r @ r)
    J = self.jacobian(x)
    dof = 4 * self.n_points - 6 - 6 * self.nv
    s2 = sigma * sigma if sigma else (sse / dof if dof > 0 else np.nan)
    cov = s2 * np.linalg.inv(J.T @ J)[:6, :6]
    view_sse = np.zeros((self.nv, 2))
    for v in range(self.nv):
      rv = r[self.first[v]:self.first[v + 1]]
      half = len(rv) // 2
      view_sse[v] = rv[:half] @ rv[:half], rv[half:] @ rv[half:]
    return dict(T=to_matrix(x[:6]), params=np.asarray(x[:6]), sse=sse, rms=np.sqrt(sse / (2 * self.n_points)), cov=cov,
                view_poses=np.stack([to_matrix(x[6 + 6 * v:12 + 6 * v]) for v in range(self.nv)]), view_sse=view_sse)
