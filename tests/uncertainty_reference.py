"""TEST INFRASTRUCTURE: an independent numpy restatement of the projection-uncertainty chain -- it does not read
csrc/mcba_uncertainty.h and uses no analytic derivative.

  forward     undistort_reference.project (the restated cv2 projections);
  inverse     undistort_reference.undistort_normalised at the estimate, polished (and re-solved for perturbed cameras) by Newton
              steps whose 2 x 2 Jacobian is a central difference of the forward function;
  chain       stored parameters theta = (camera b: fx fy cx cy skew dist.. | rvec tvec of b | rvec tvec of a | camera a) -> pixel
              in b of the point that is fixed in the rig frame (reference None) or that camera a sees at pixel q at distance 1 / rho;
  Jacobian    Richardson-extrapolated central differences of the chain over theta, with the difference between the two finest
              levels as the error estimate of every entry.
"""
import numpy as np
from scipy.spatial.transform import Rotation

import undistort_reference as ref

STEP = dict(focal=0.5, centre=0.5, skew=0.5, dist=2e-3, rvec=2e-3, tvec=2e-3)


class Camera(object):           # (undistort_reference.is_fisheye looks at the class name)
  def __init__(self, intrinsic, dist):
    self.intrinsic, self.dist = intrinsic, dist


class CameraFisheye(Camera):
  pass


def camera_block(camera, fix_aspect=False):
  """stored block fx fy cx cy skew dist.. of a camera (fix_aspect: both focal entries hold the mean, as Camera.params does)"""
  K = np.asarray(camera.intrinsic, dtype=np.float64)
  f = [K[0, 0], K[1, 1]] if not fix_aspect else [0.5 * (K[0, 0] + K[1, 1])] * 2
  return np.concatenate([f, [K[0, 2], K[1, 2], 0.0], np.asarray(camera.dist, dtype=np.float64).ravel()])


def camera_of(block, fisheye, fix_aspect):
  fx, fy = (block[0], block[0]) if fix_aspect else (block[0], block[1])
  K = np.array([[fx, 0.0, block[2]], [0.0, fy, block[3]], [0.0, 0.0, 1.0]])
  return (CameraFisheye if fisheye else Camera)(K, np.array(block[5:], dtype=np.float64))


def pose_of(rt):
  return Rotation.from_rotvec(rt[:3]).as_matrix(), np.asarray(rt[3:], dtype=np.float64)


def inverse(camera, uv, start=None):
  """normalised point whose projection is uv: Newton on the forward function with a central-difference Jacobian, from `start` or
  from undistort_reference.undistort_normalised; None where it does not settle"""
  uv = np.asarray(uv, dtype=np.float64)
  q = ref.undistort_normalised(camera, uv[None])[0] if start is None else np.array(start, dtype=np.float64)
  h = 1e-6
  for _ in range(12):
    P = np.array([[q[0], q[1], 1.0], [q[0] + h, q[1], 1.0], [q[0] - h, q[1], 1.0], [q[0], q[1] + h, 1.0], [q[0], q[1] - h, 1.0]])
    p = ref.project(camera, P)
    Jm = np.stack([(p[1] - p[2]) / (2 * h), (p[3] - p[4]) / (2 * h)], axis=1)
    if not np.isfinite(Jm).all() or abs(np.linalg.det(Jm)) < 1e-300:
      return None
    step = np.linalg.solve(Jm, p[0] - uv)
    q = q - step
    if np.abs(step).max() < 1e-15 * max(1.0, np.abs(q).max()):
      return q
  return q if np.abs(step).max() < 1e-12 else None


class Chain(object):
  """one job: cameras b (and a), their stored blocks and poses at the estimate"""

  def __init__(self, cam_b, rt_b, cam_a=None, rt_a=None, rho=0.0, fix_aspect_b=False, fix_aspect_a=False):
    self.fish_b, self.fa_b = ref.is_fisheye(cam_b), fix_aspect_b
    self.has_a = cam_a is not None
    blocks = [camera_block(cam_b, fix_aspect_b), np.asarray(rt_b, dtype=np.float64)]
    if self.has_a:
      self.fish_a, self.fa_a = ref.is_fisheye(cam_a), fix_aspect_a
      blocks += [np.asarray(rt_a, dtype=np.float64), camera_block(cam_a, fix_aspect_a)]
    self.sizes = [len(b) for b in blocks]
    self.theta = np.concatenate(blocks)
    self.rho = float(rho)
    nb = self.sizes[0]
    self.steps = np.array([STEP["focal"]] * 2 + [STEP["centre"]] * 2 + [STEP["skew"]] + [STEP["dist"]] * (nb - 5) + [STEP["rvec"]] * 3 +
                          [STEP["tvec"]] * 3)
    if self.has_a:
      na = self.sizes[3]
      self.steps = np.concatenate([self.steps, [STEP["rvec"]] * 3 + [STEP["tvec"]] * 3 + [STEP["focal"]] * 2 + [STEP["centre"]] * 2 +
                                   [STEP["skew"]] + [STEP["dist"]] * (na - 5)])

  def split(self, theta):
    out, pos = [], 0
    for n in self.sizes:
      out.append(theta[pos:pos + n])
      pos += n
    return out

  def source(self, q):
    """what of a query does not change with the parameters of b: (the solution of the inverse at the estimate, the fixed point)"""
    parts = self.split(self.theta)
    cam = camera_of(parts[3], self.fish_a, self.fa_a) if self.has_a else camera_of(parts[0], self.fish_b, self.fa_b)
    xy = inverse(cam, q)
    if xy is None:
      return None
    n = np.array([xy[0], xy[1], 1.0])
    n /= np.linalg.norm(n)
    fixed = None
    if not self.has_a:
      R, t = pose_of(parts[1])
      fixed = R.T @ (n - self.rho * t)               # rho X_rig
    return xy, fixed

  def predict(self, theta, q, source):
    """pixel in b at the parameters theta (the exact chain: inverse through a, transform, project through b)"""
    parts = self.split(np.asarray(theta, dtype=np.float64))
    Rb, tb = pose_of(parts[1])
    if self.has_a:
      xy = source[0]
      if not np.array_equal(parts[3], self.split(self.theta)[3]):
        xy = inverse(camera_of(parts[3], self.fish_a, self.fa_a), q, start=xy)
      n = np.array([xy[0], xy[1], 1.0])
      n /= np.linalg.norm(n)
      Ra, ta = pose_of(parts[2])
      Y = Rb @ (Ra.T @ (n - self.rho * ta)) + self.rho * tb
    else:
      Y = Rb @ source[1] + self.rho * tb
    return ref.project(camera_of(parts[0], self.fish_b, self.fa_b), Y[None])[0], Y

  def jacobian(self, q):
    """(J [2, p], err [2, p]) by Richardson extrapolation of central differences at steps h, h / 2, h / 4; None outside the model"""
    src = self.source(q)
    if src is None:
      return None
    p = len(self.theta)
    D = np.zeros((3, 2, p))
    for k in range(p):
      for level in range(3):
        h = self.steps[k] / (1 << level)
        e = np.zeros(p)
        e[k] = h
        D[level, :, k] = (self.predict(self.theta + e, q, src)[0] - self.predict(self.theta - e, q, src)[0]) / (2.0 * h)
    r1a, r1b = (4.0 * D[1] - D[0]) / 3.0, (4.0 * D[2] - D[1]) / 3.0
    r2 = (16.0 * r1b - r1a) / 15.0
    return r2, np.abs(r2 - r1b)
