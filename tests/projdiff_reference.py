"""TEST INFRASTRUCTURE: an independent numpy / scipy restatement of the projection difference.  It shares no formula
code with csrc/mcba_projdiff.h: its own projection (OpenCV's documented Brown-Conrady model with rational, thin-prism and tilt terms;
Kannala-Brandt), its own inverse by root finding (scipy.optimize.root on the projection itself), scipy's rotations and
scipy.optimize.least_squares at tight tolerances for the implied transform.  Cameras are read as plain data: `intrinsic`, `dist` and
`model` ("fisheye" or not) of uncertainty.RigModel.cameras, which carries the fix_aspect rule."""
import numpy as np
from scipy.optimize import least_squares, root
from scipy.spatial.transform import Rotation


def _tilt(tx, ty):
  cx, sx, cy, sy = np.cos(tx), np.sin(tx), np.cos(ty), np.sin(ty)
  Rx = np.array([[1, 0, 0], [0, cx, sx], [0, -sx, cx]])
  Ry = np.array([[cy, 0, -sy], [0, 1, 0], [sy, 0, cy]])
  R = Ry @ Rx
  Pz = np.array([[R[2, 2], 0, -R[0, 2]], [0, R[2, 2], -R[1, 2]], [0, 0, 1]])
  return Pz @ R


def distort(cam, x, y):
  """distorted normalised coordinates of the normalised point(s) (x, y)"""
  d = np.zeros(14)
  k = np.asarray(cam.dist, dtype=np.float64).ravel()
  if cam.model == "fisheye":
    r = np.sqrt(x * x + y * y)
    th = np.arctan(r)
    t2 = th * th
    thd = th * (1 + k[0] * t2 + k[1] * t2 ** 2 + k[2] * t2 ** 3 + k[3] * t2 ** 4)
    with np.errstate(invalid="ignore", divide="ignore"):
      s = np.where(r > 1e-300, thd / np.where(r > 1e-300, r, 1.0), 1.0)
    return s * x, s * y
  d[:len(k)] = k
  k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4, tx, ty = d
  r2 = x * x + y * y
  radial = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
  xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x) + s1 * r2 + s2 * r2 ** 2
  yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y + s3 * r2 + s4 * r2 ** 2
  if tx != 0.0 or ty != 0.0:
    T = _tilt(tx, ty)
    v = T @ np.stack([xd, yd, np.ones_like(xd)])
    xd, yd = v[0] / v[2], v[1] / v[2]
  return xd, yd


def project(cam, X):
  """pixels [n, 2] of the camera-frame points X [n, 3] (any positive scale)"""
  X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
  K = np.asarray(cam.intrinsic, dtype=np.float64)
  xd, yd = distort(cam, X[:, 0] / X[:, 2], X[:, 1] / X[:, 2])
  return np.stack([K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]], axis=-1)


def unit_ray(cam, q):
  """(n [3], converged) of one pixel: root of project(x, y, 1) = q"""
  K = np.asarray(cam.intrinsic, dtype=np.float64)
  q = np.asarray(q, dtype=np.float64)

  def f(p):
    return project(cam, [[p[0], p[1], 1.0]])[0] - q

  start = np.array([(q[0] - K[0, 2]) / K[0, 0], (q[1] - K[1, 2]) / K[1, 1]])
  sol = root(f, start, method="hybr", tol=1e-15)
  p = sol.x
  for _ in range(3):                                   # polish: two secant-Newton steps on a central difference
    h = 1e-6
    J = np.stack([(f(p + [h, 0]) - f(p - [h, 0])) / (2 * h), (f(p + [0, h]) - f(p - [0, h])) / (2 * h)], axis=-1)
    p = p - np.linalg.solve(J, f(p))
  ok = bool(np.abs(f(p)).max() < 1e-9)
  n = np.array([p[0], p[1], 1.0])
  return n / np.linalg.norm(n), ok


def unit_rays(cam, pixels):
  rays = [unit_ray(cam, q) for q in np.asarray(pixels, dtype=np.float64).reshape(-1, 2)]
  return np.array([r[0] for r in rays]).reshape(-1, 3), np.array([r[1] for r in rays], dtype=bool)


def moved(transform, Y, rho):
  """R(omega) Y + rho tau"""
  t = np.asarray(transform, dtype=np.float64)
  return Rotation.from_rotvec(t[:3]).apply(Y) + rho * t[3:]


def intrinsic_diff(cam0, cam1, transform, rho, pixels):
  """diff [n, 2] of the intrinsics mode under a given transform"""
  pixels = np.asarray(pixels, dtype=np.float64).reshape(-1, 2)
  Y, _ = unit_rays(cam0, pixels)
  return project(cam1, moved(transform, Y, rho)) - pixels


def fit_transform(cam1, Y, targets, rho, unknowns, method="trf"):
  """(omega | tau) [6] minimising sum |project_1(R(omega) Y + rho tau) - targets|^2 from the identity; unknowns 0, 3 or 6"""
  if unknowns == 0:
    return np.zeros(6)

  def f(p):
    t = np.zeros(6)
    t[:unknowns] = p
    return (project(cam1, moved(t, Y, rho)) - targets).ravel()

  kw = dict(xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
  if method == "trf":
    kw["x_scale"] = "jac"
  sol = least_squares(f, np.zeros(unknowns), method=method, **kw)
  out = np.zeros(6)
  out[:unknowns] = sol.x
  return out


def displacement(cam1, Y, rho, t_a, t_b):
  """the largest pixel displacement between two transforms over the points Y"""
  return float(np.abs(project(cam1, moved(t_a, Y, rho)) - project(cam1, moved(t_b, Y, rho))).max())


def transfer_diff(rig0, rig1, b, a, rho, pixels):
  """(diff [n, 2], landing [n, 2]) of the transfer mode; rig: uncertainty.RigModel (cameras, poses [C, 4, 4])"""
  out = []
  for rig in (rig0, rig1):
    Y, _ = unit_rays(rig.cameras[a], pixels)
    T = rig.poses[b] @ np.linalg.inv(rig.poses[a])
    out.append(project(rig.cameras[b], Y @ T[:3, :3].T + rho * T[:3, 3]))
  return out[1] - out[0], out[0]


def fit_camera(cam0, unknowns, pixels, targets):
  """An `unknowns`-coefficient Brown-Conrady camera fitted by this module's own least squares to pixels <- rays of cam0: (K [3, 3],
  dist): the cross-family case"""
  Y, ok = unit_rays(cam0, pixels)
  K0 = np.asarray(cam0.intrinsic, dtype=np.float64)
  from types import SimpleNamespace

  def cam_of(p):
    K = np.array([[p[0], 0, p[2]], [0, p[1], p[3]], [0, 0, 1.0]])
    return SimpleNamespace(intrinsic=K, dist=p[4:], model="pinhole")

  start = np.concatenate([[K0[0, 0], K0[1, 1], K0[0, 2], K0[1, 2]], np.zeros(unknowns)])
  start[4:4 + min(unknowns, len(cam0.dist))] = np.asarray(cam0.dist)[:unknowns]
  sol = least_squares(lambda p: (project(cam_of(p), Y[ok]) - targets[ok]).ravel(), start, x_scale="jac", xtol=1e-14, ftol=1e-14, gtol=1e-14)
  c = cam_of(sol.x)
  return c.intrinsic, c.dist
