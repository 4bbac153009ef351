"""TEST INFRASTRUCTURE: an independent numpy / scipy restatement of the rig localisation -- it does not read csrc/mcba_localize.h.

  chain       X_cam = camera_pose[c] . rig . board_pose[b] . X (rolling shutter: the lerp of the two transformed points at
              t = v_observed / image height), rotations through scipy's Rotation.from_rotvec;
  projection  the restated cv2.projectPoints / cv2.fisheye.projectPoints of oracle/shims/cv2 (float64);
  Jacobian    central differences of the residuals (step 1e-6: 1e-9 relative on these rigs);
  optimum     scipy.optimize.least_squares per frame with every tolerance at 1e-15.
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


class Frame(object):
  """One frame of a rig (localize_host_lib.make_rig): its usable observations in (camera, board, point) order."""

  def __init__(self, rig, f):
    Cn, F, B, P = rig.shape
    self.rig, self.rolling = rig, rig.rolling
    self.K = 12 if rig.rolling else 6
    world = []
    for b, pts in enumerate(rig.board_points):
      x = np.zeros((P, 3))
      x[:len(pts)] = np.asarray(pts, dtype=np.float64)
      world.append(x @ rig.board_poses[b][:3, :3].T + rig.board_poses[b][:3, 3])
    world = np.stack(world)
    self.cams = []          # (camera, camera pose, world points [n, 3], pixels [n, 2]) of every camera that saw something
    for c in range(Cn):
      idx = np.argwhere(rig.valid[c, f])
      if len(idx):
        self.cams.append((c, world[idx[:, 0], idx[:, 1]], rig.points[c, f][idx[:, 0], idx[:, 1]]))
    self.n = sum(len(w) for _, w, _ in self.cams)

  def residuals(self, x):
    start = to_matrix(x[:6])
    end = to_matrix(x[6:12]) if self.rolling else None
    out = []
    for c, w, uv in self.cams:
      cam, T = self.rig.cameras[c], self.rig.camera_poses[c]
      M = T @ start
      X = w @ M[:3, :3].T + M[:3, 3]
      if self.rolling:
        Me = T @ end
        t = (uv[:, 1] / cam.image_size[1])[:, None]
        X = (1.0 - t) * X + t * (w @ Me[:3, :3].T + Me[:3, 3])
      out.append(project(cam, X) - uv)
    return np.concatenate(out).ravel() if out else np.zeros(0)

  def jacobian(self, x, step=1e-6):
    J = np.zeros((2 * self.n, self.K))
    for k in range(self.K):
      d = np.zeros(self.K)
      d[k] = step
      J[:, k] = (self.residuals(x + d) - self.residuals(x - d)) / (2.0 * step)
    return J

  def solve(self, x0):
    return least_squares(self.residuals, np.asarray(x0, dtype=np.float64), jac=self.jacobian, x_scale='jac', xtol=1e-15, ftol=1e-15,
                         gtol=1e-15, max_nfev=200)

  def lm_step(self, x0, lam=1e-3):
    """x0 + the first Levenberg-Marquardt step with Marquardt scaling: (H + lam diag H) d = -g"""
    J, r = self.jacobian(x0), self.residuals(x0)
    H = J.T @ J
    return x0 + np.linalg.solve(H + lam * np.diag(np.diag(H)), -J.T @ r)


def start_vector(rig, f, poses=None, poses_end=None):
  """the parameter vector of frame f at the given poses (default: the rig's truth)"""
  poses = rig.rig_poses if poses is None else poses
  x = from_matrix(poses[f])
  if rig.rolling:
    end = rig.rig_poses_end if poses_end is None else poses_end
    x = np.concatenate([x, from_matrix(end[f])])
  return x
