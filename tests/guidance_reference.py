"""TEST INFRASTRUCTURE: an independent numpy restatement of the view-information chain -- it does not read csrc/mcba_guidance.h,
uses no analytic derivative and has its own projection (checked against undistort_reference.project by the tests).

  forward     OpenCV's pinhole model (radial, rational, tangential, thin prism, tilt) and the Kannala-Brandt fisheye model, written
              out here in numpy over the stored block theta = fx fy cx cy skew dist.. (fix_aspect: the first focal length is both);
  inverse     Newton on the forward function with a central-difference 2 x 2 Jacobian;
  rows        Richardson-extrapolated central differences (steps h, h / 2, h / 4, as uncertainty_reference) of the pixels of the
              points over theta (K [2P, p]) and over a left perturbation exp(omega) Y + rho tau of the view's own pose (E [2P, nn]);
  visibility  in front, inside the image by the margin, det d(u, v) / d(x, y) > 0 by differences;
  Schur       S = (K F)^T (I - Q Q^T) (K F) with Q from a QR of E; the normal-equation route beside it gives the restatement's own
              spread;
  scores      log-determinants by slogdet and traces through numpy's inverse.
"""
import numpy as np

STEP = dict(focal=0.5, centre=0.5, skew=0.5, dist=2e-3, pose=2e-3)


def steps_of(p):
  return np.array([STEP["focal"]] * 2 + [STEP["centre"]] * 2 + [STEP["skew"]] + [STEP["dist"]] * (p - 5))


def stored_block(camera, fix_aspect=False):
  K = np.asarray(camera.intrinsic, dtype=np.float64)
  f = [K[0, 0], K[1, 1]] if not fix_aspect else [0.5 * (K[0, 0] + K[1, 1])] * 2
  return np.concatenate([f, [K[0, 2], K[1, 2], 0.0], np.asarray(camera.dist, dtype=np.float64).ravel()])


def project(theta, fisheye, fix_aspect, X):
  """pixels [n, 2] of camera-frame points [n, 3] (any positive scale of a point gives the same pixel)"""
  X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
  fx, fy = (theta[0], theta[0]) if fix_aspect else (theta[0], theta[1])
  cx, cy, k = theta[2], theta[3], np.asarray(theta[5:], dtype=np.float64)
  with np.errstate(all="ignore"):
    x, y = X[:, 0] / X[:, 2], X[:, 1] / X[:, 2]
    r2 = x * x + y * y
    if fisheye:
      r = np.sqrt(r2)
      t = np.arctan(r)
      t2 = t * t
      td = t * (1.0 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))
      s = np.where(r > 1e-12, td / np.where(r > 1e-12, r, 1.0), 1.0)
      xd, yd = x * s, y * s
    else:
      k = np.concatenate([k, np.zeros(14 - len(k))])
      k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4, tx, ty = k
      radial = (1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1.0 + r2 * (k4 + r2 * (k5 + r2 * k6)))
      xd = x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x) + r2 * (s1 + r2 * s2)
      yd = y * radial + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y + r2 * (s3 + r2 * s4)
      if tx != 0.0 or ty != 0.0:
        cxr, sxr, cyr, syr = np.cos(tx), np.sin(tx), np.cos(ty), np.sin(ty)
        Rx = np.array([[1.0, 0.0, 0.0], [0.0, cxr, sxr], [0.0, -sxr, cxr]])
        Ry = np.array([[cyr, 0.0, -syr], [0.0, 1.0, 0.0], [syr, 0.0, cyr]])
        R = Ry @ Rx
        T = np.array([[R[2, 2], 0.0, -R[0, 2]], [0.0, R[2, 2], -R[1, 2]], [0.0, 0.0, 1.0]]) @ R
        v = np.stack([xd, yd, np.ones_like(xd)], axis=1) @ T.T
        xd, yd = v[:, 0] / v[:, 2], v[:, 1] / v[:, 2]
    return np.stack([fx * xd + cx, fy * yd + cy], axis=1)


def richardson(f, x0, steps):
  """d f / d x [.., len(x0)] at x0 by central differences at three step sizes, extrapolated twice"""
  x0 = np.asarray(x0, dtype=np.float64)
  cols = []
  for k in range(len(x0)):
    D = []
    for level in range(3):
      h = steps[k] / (1 << level)
      e = np.zeros(len(x0))
      e[k] = h
      D.append((f(x0 + e) - f(x0 - e)) / (2.0 * h))
    r1a, r1b = (4.0 * D[1] - D[0]) / 3.0, (4.0 * D[2] - D[1]) / 3.0
    cols.append((16.0 * r1b - r1a) / 15.0)
  return np.stack(cols, axis=-1)


def rodrigues(w):
  t = float(np.linalg.norm(w))
  Kx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
  if t < 1e-12:
    return np.eye(3) + Kx
  return np.eye(3) + np.sin(t) / t * Kx + (1.0 - np.cos(t)) / (t * t) * (Kx @ Kx)


def ray(theta, fisheye, fix_aspect, pixel):
  """unit ray whose projection is the pixel; None where Newton does not settle"""
  fx, fy = (theta[0], theta[0]) if fix_aspect else (theta[0], theta[1])
  q = np.array([(pixel[0] - theta[2]) / fx, (pixel[1] - theta[3]) / fy])
  h, step = 1e-6, np.array([1.0, 1.0])
  for _ in range(30):
    P = np.array([[q[0], q[1], 1.0], [q[0] + h, q[1], 1.0], [q[0] - h, q[1], 1.0], [q[0], q[1] + h, 1.0], [q[0], q[1] - h, 1.0]])
    p = project(theta, fisheye, fix_aspect, P)
    J = np.stack([(p[1] - p[2]) / (2 * h), (p[3] - p[4]) / (2 * h)], axis=1)
    if not np.isfinite(J).all() or abs(np.linalg.det(J)) < 1e-300:
      return None
    step = np.linalg.solve(J, p[0] - np.asarray(pixel, dtype=np.float64))
    q = q - step
    if np.abs(step).max() < 1e-15 * max(1.0, np.abs(q).max()):
      break
  if not np.abs(step).max() < 1e-12:
    return None
  n = np.array([q[0], q[1], 1.0])
  return n / np.linalg.norm(n)


def visible(theta, fisheye, fix_aspect, X, image_size=None, margin=0.0):
  """[n] bool: in front, (a board: inside the image by the margin,) the model monotone where the point lands"""
  X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
  ok = X[:, 2] > 0.0
  Z = np.where(ok[:, None], X, [0.0, 0.0, 1.0])
  n = Z / Z[:, 2:3]
  h = 1e-6
  uv = project(theta, fisheye, fix_aspect, n)
  dx = (project(theta, fisheye, fix_aspect, n + [h, 0, 0]) - project(theta, fisheye, fix_aspect, n - [h, 0, 0])) / (2 * h)
  dy = (project(theta, fisheye, fix_aspect, n + [0, h, 0]) - project(theta, fisheye, fix_aspect, n - [0, h, 0])) / (2 * h)
  with np.errstate(invalid="ignore"):
    ok &= np.isfinite(uv).all(axis=1) & (dx[:, 0] * dy[:, 1] - dx[:, 1] * dy[:, 0] > 0.0)
    if image_size is not None:
      W, H = image_size
      ok &= (uv[:, 0] >= margin) & (uv[:, 1] >= margin) & (uv[:, 0] <= W - 1.0 - margin) & (uv[:, 1] <= H - 1.0 - margin)
  return ok


def rows(theta, fisheye, fix_aspect, Y, rho, n_nuisance):
  """(K [2P, p] over the stored block, E [2P, n_nuisance] over the left perturbation (omega | tau) of the view's own pose) at the
  scaled points Y [P, 3]: the pixel of exp(omega) Y + rho tau"""
  Y = np.asarray(Y, dtype=np.float64).reshape(-1, 3)
  theta = np.asarray(theta, dtype=np.float64)
  K = richardson(lambda th: project(th, fisheye, fix_aspect, Y).ravel(), theta, steps_of(len(theta)))
  if n_nuisance == 0:
    return K, np.zeros((2 * len(Y), 0))
  E = richardson(lambda x: project(theta, fisheye, fix_aspect, Y @ rodrigues(x[:3]).T + rho * x[3:]).ravel(), np.zeros(6),
                 [STEP["pose"]] * 6)
  return K, E[:, :n_nuisance]


def schur(KW, E):
  """(S by the QR route, S by the normal equations)"""
  if E.shape[1] == 0:
    S = KW.T @ KW
    return S, S
  Q, _ = np.linalg.qr(E)
  R = KW - Q @ (Q.T @ KW)
  G = E.T @ KW
  return R.T @ R, KW.T @ KW - G.T @ np.linalg.solve(E.T @ E, G)


def board_view(theta, fisheye, fix_aspect, points, T, n_nuisance, F, image_size, margin=0.0):
  """(S_qr, S_ne, visible mask, |K F|_F^2) of a board view"""
  X = np.asarray(points, dtype=np.float64).reshape(-1, 3) @ np.asarray(T)[:3, :3].T + np.asarray(T)[:3, 3]
  ok = visible(theta, fisheye, fix_aspect, X, image_size, margin)
  K, E = rows(theta, fisheye, fix_aspect, X[ok], 1.0, n_nuisance)
  KW = K @ F
  return schur(KW, E) + (ok, float((KW * KW).sum()))


def focus_view(theta, fisheye, fix_aspect, pixels, rho, n_nuisance, F):
  """(S_qr, S_ne, visible mask, |K F|_F^2) of a focus: the unit rays of the pixels, fixed while the intrinsics vary"""
  rays = [ray(theta, fisheye, fix_aspect, q) for q in np.asarray(pixels, dtype=np.float64).reshape(-1, 2)]
  ok = np.array([n is not None for n in rays])
  Y = np.array([n for n in rays if n is not None]).reshape(-1, 3)
  ok[ok] = visible(theta, fisheye, fix_aspect, Y)
  Y = np.array([n for n, good in zip(rays, ok) if good]).reshape(-1, 3)
  K, E = rows(theta, fisheye, fix_aspect, Y, rho, n_nuisance)
  KW = K @ F
  return schur(KW, E) + (ok, float((KW * KW).sum()))


def gain(B, A):
  return 0.5 * (np.linalg.slogdet(B + A)[1] - np.linalg.slogdet(B)[1])


def focus_rms(B, A, Q, n):
  return float(np.sqrt(np.trace(np.linalg.inv(B + A) @ Q) / n))


def greedy(S, status, Q, n_focus, sigma2, n, criterion):
  """(picks, gains, focus after) of a numpy greedy over the S [V, r, r] of one camera's candidates"""
  r = S.shape[1]
  B, taken, out = np.eye(r), set(), []
  for _ in range(n):
    best, best_score = -1, None
    for v in range(len(S)):
      if status[v] != 0 or v in taken:
        continue
      score = gain(B, S[v] / sigma2) if criterion == "gain" else -focus_rms(B, S[v] / sigma2, Q, n_focus)
      if best < 0 or score > best_score:
        best, best_score = v, score
    if best < 0:
      break
    out.append((best, gain(B, S[best] / sigma2), focus_rms(B, S[best] / sigma2, Q, n_focus) if Q is not None else np.nan))
    taken.add(best)
    B = B + S[best] / sigma2
  return out
