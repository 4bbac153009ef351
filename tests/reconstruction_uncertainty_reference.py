"""TEST INFRASTRUCTURE: an independent numpy restatement of the reconstruction-uncertainty chain -- it does not read
csrc/mcba_recon.h and uses no analytic derivative.

  forward       undistort_reference.project (the restated cv2 projections) of R_c X + t_c;
  chain         stored parameters theta = per slot (camera: fx fy cx cy skew dist.. | rvec tvec) -> the point triangulated from the
                FIXED noise-free pixels q_c = project_c(theta_0; X_0) of the views: Gauss-Newton on the pixel residuals to
                convergence, its 2 x 3 Jacobians four-level Richardson-extrapolated central differences of the forward function (their error
                times the residual that stays is a bias of the minimiser that grows with the step of theta); expressed in
                the rig frame or in the frame of a camera of the group (R_a(theta) X + t_a(theta));
  Jacobian      Richardson-extrapolated central differences of the chain over theta, with the difference between the two finest
                levels as the error estimate of every entry;
  SampleChain   the same chain vectorised over samples of theta, with a projection of its own (Brown-Conrady with up to 12
                coefficients and Kannala-Brandt, no tilt) that the tests pin to undistort_reference.project.
"""
import numpy as np
from scipy.spatial.transform import Rotation

import uncertainty_reference as ur
import undistort_reference as ref

STEP = ur.STEP


def slot_steps(n_dist):
  return np.array([STEP["focal"]] * 2 + [STEP["centre"]] * 2 + [STEP["skew"]] + [STEP["dist"]] * n_dist + [STEP["rvec"]] * 3 +
                  [STEP["tvec"]] * 3)


class Chain(object):
  """one point of one job: cameras [G] (slot order) with their stored poses rtvecs [G, 6] at the estimate, the point X0 in the rig
  frame and the slots that are its views"""

  def __init__(self, cameras, rtvecs, fix_aspect, X0, views):
    self.fish = [ref.is_fisheye(c) for c in cameras]
    self.fa = list(fix_aspect)
    blocks = [np.concatenate([ur.camera_block(c, fa), np.asarray(rt, dtype=np.float64)]) for c, rt, fa in zip(cameras, rtvecs, fix_aspect)]
    self.sizes = [len(b) for b in blocks]
    self.first = np.concatenate([[0], np.cumsum(self.sizes)])
    self.theta = np.concatenate(blocks)
    self.steps = np.concatenate([slot_steps(n - 11) for n in self.sizes])
    self.X0 = np.asarray(X0, dtype=np.float64)
    self.views = list(views)
    self.q = {s: self.pixel(self.theta, s, self.X0[None])[0] for s in self.views}

  def slot(self, theta, s):
    part = theta[self.first[s]:self.first[s + 1]]
    return ur.camera_of(part[:-6], self.fish[s], self.fa[s]), ur.pose_of(part[-6:])

  def pixel(self, theta, s, X):
    cam, (R, t) = self.slot(theta, s)
    return ref.project(cam, X @ R.T + t)

  def residuals(self, theta, X):
    """[n, 2 V] of the points X [n, 3]"""
    return np.concatenate([self.pixel(theta, s, X) - self.q[s] for s in self.views], axis=1)

  def triangulate(self, theta):
    """the minimiser of the pixel residuals at theta, from X0"""
    X = self.X0.copy()
    h0, levels = 2e-2 * np.linalg.norm(X), 4
    offsets = [np.zeros(3)]
    for level in range(levels):
      for k in range(3):
        e = np.zeros(3)
        e[k] = h0 / (1 << level)
        offsets += [e, -e]
    offsets = np.array(offsets)
    for _ in range(20):
      r = self.residuals(theta, X[None] + offsets)
      D = np.zeros((levels, r.shape[1], 3))
      for level in range(levels):
        for k in range(3):
          i = 1 + 6 * level + 2 * k
          D[level, :, k] = (r[i] - r[i + 1]) / (2.0 * h0 / (1 << level))
      for order in range(1, levels):                  # Richardson: h^2, h^4, h^6 leave in turn
        D = [(4.0 ** order * D[i + 1] - D[i]) / (4.0 ** order - 1.0) for i in range(len(D) - 1)]
      J = D[0]
      step = np.linalg.solve(J.T @ J, -J.T @ r[0])
      X = X + step
      if np.abs(step).max() <= 1e-15 * np.linalg.norm(X):
        break
    return X

  def express(self, theta, X, reference):
    if reference is None:
      return X
    R, t = self.slot(theta, reference)[1]
    return R @ X + t

  def jacobian(self, references):
    """{reference: (J [3, p], err [3, p])} by Richardson extrapolation of central differences at steps h, h / 2, h / 4; the
    triangulations are shared by the references"""
    p = len(self.theta)
    D = {a: np.zeros((3, 3, p)) for a in references}
    for k in range(p):
      for level in range(3):
        h = self.steps[k] / (1 << level)
        e = np.zeros(p)
        e[k] = h
        Xp, Xm = self.triangulate(self.theta + e), self.triangulate(self.theta - e)
        for a in references:
          D[a][level, :, k] = (self.express(self.theta + e, Xp, a) - self.express(self.theta - e, Xm, a)) / (2.0 * h)
    out = {}
    for a in references:
      r1a, r1b = (4.0 * D[a][1] - D[a][0]) / 3.0, (4.0 * D[a][2] - D[a][1]) / 3.0
      r2 = (16.0 * r1b - r1a) / 15.0
      out[a] = (r2, np.abs(r2 - r1b))
    return out


# ---- vectorised over samples ---------------------------------------------------------------------------------------------------
def project_samples(block, fisheye, fix_aspect, Y):
  """pixels [N, 2] of the camera-frame points Y [N, 3] through the stored blocks [N, 5 + nd] (fx fy cx cy skew dist..): cv2's
  Brown-Conrady model (k1 k2 p1 p2 k3 | k4 k5 k6 | s1 s2 s3 s4, no tilt) or the Kannala-Brandt fisheye"""
  fx, fy = block[:, 0], block[:, 0] if fix_aspect else block[:, 1]
  cx, cy, d = block[:, 2], block[:, 3], block[:, 5:]
  x, y = Y[:, 0] / Y[:, 2], Y[:, 1] / Y[:, 2]
  r2 = x * x + y * y
  if fisheye:
    r = np.sqrt(r2)
    th = np.arctan(r)
    t2 = th * th
    thd = th * (1.0 + t2 * (d[:, 0] + t2 * (d[:, 1] + t2 * (d[:, 2] + t2 * d[:, 3]))))
    s = np.where(r > 1e-8, thd / np.where(r > 1e-8, r, 1.0), 1.0)
    return np.stack([fx * (x * s) + cx, fy * (y * s) + cy], axis=1)
  nd = d.shape[1]
  k = lambda i: d[:, i] if i < nd else 0.0
  radial = (1.0 + r2 * (k(0) + r2 * (k(1) + r2 * k(4)))) / (1.0 + r2 * (k(5) + r2 * (k(6) + r2 * k(7))))
  xd = x * radial + 2.0 * k(2) * x * y + k(3) * (r2 + 2.0 * x * x) + r2 * (k(8) + r2 * k(9))
  yd = y * radial + k(2) * (r2 + 2.0 * y * y) + 2.0 * k(3) * x * y + r2 * (k(10) + r2 * k(11))
  return np.stack([fx * xd + cx, fy * yd + cy], axis=1)


class SampleChain(object):
  """the chain of `chain` (a Chain without a tilted camera) over N samples of theta at once"""

  def __init__(self, chain):
    self.c = chain

  def pixel(self, thetas, s, X):
    c = self.c
    part = thetas[:, c.first[s]:c.first[s + 1]]
    R = Rotation.from_rotvec(part[:, -6:-3]).as_matrix()
    Y = np.einsum("nij,nj->ni", R, X) + part[:, -3:]
    return project_samples(part[:, :-6], c.fish[s], c.fa[s], Y)

  def residuals(self, thetas, X):
    return np.concatenate([self.pixel(thetas, s, X) - self.c.q[s][None] for s in self.c.views], axis=1)

  def triangulate(self, thetas):
    """[N, 3]: Gauss-Newton per sample from X0, central-difference Jacobians (their error enters times the residual that stays: far below the sampling error)"""
    N = len(thetas)
    X = np.tile(self.c.X0, (N, 1))
    h = 1e-5 * np.linalg.norm(self.c.X0)
    for _ in range(30):
      r = self.residuals(thetas, X)
      J = np.zeros((N, r.shape[1], 3))
      for k in range(3):
        e = np.zeros(3)
        e[k] = h
        J[:, :, k] = (self.residuals(thetas, X + e) - self.residuals(thetas, X - e)) / (2.0 * h)
      H = np.einsum("nri,nrj->nij", J, J)
      g = np.einsum("nri,nr->ni", J, r)
      step = np.linalg.solve(H, -g[..., None])[..., 0]
      X = X + step
      if np.abs(step).max() <= 1e-13 * np.linalg.norm(self.c.X0):
        break
    return X

  def express(self, thetas, X, reference):
    if reference is None:
      return X
    c = self.c
    part = thetas[:, c.first[reference]:c.first[reference + 1]]
    R = Rotation.from_rotvec(part[:, -6:-3]).as_matrix()
    return np.einsum("nij,nj->ni", R, X) + part[:, -3:]
