"""Using a calibration: how far can it be trusted at a pixel where no board ever was?  

One entry point of libmcba.so (csrc/mcba_uncertainty.h): the 2 x 2 covariance of where a point projects into a camera when the
shared parameters vary with their covariance, one lane per pixel of a grid generated on the device or of a list.

  reference=None   the point behind pixel q of camera b at the given distance is fixed in the RIG frame (with the default hold: the
                   frame of the held camera, whose own map is then intrinsics-only);
  reference=a      camera a sees the point at pixel q at that distance: the covariance of where camera b sees it (transfer /
                   epipolar uncertainty; does not depend on the gauge).

This module marshals: the index set of a job into param_vec, the sub-block of cov.shared, held / unobserved flags, the map M from
the stored parameters (rotation vector | translation of a pose; the single focal length of fix_aspect) to the columns the device
works in, the factor W = M F of the covariance (F F^T = Sigma_sub by a symmetric eigendecomposition; an eigenvalue at or below
len(Sigma_sub) * eps * the largest one -- negative ones among them -- is dropped), and grid or pixel-list jobs.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import dp as _dp, entry as _entry, f64 as _f64, up as _up   # noqa: F401 (_entry: see _lib.entry)
from .structs import struct
from .tables import _is_fisheye
from .undistort import CameraSetInputs

OK, NOT_CONVERGED, BEHIND, UNCONSTRAINED = _lib.UNC_OK, _lib.UNC_NOT_CONVERGED, _lib.UNC_BEHIND, _lib.UNC_UNCONSTRAINED
MAX_K = _lib.UNC_MAX_K


# ---- stored parameters -> the columns of the device --------------------------------------------------------------------------
def skew(v):
  return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def left_jacobian(w):
  """L(w) of SO(3): exp([w + dw]x) = exp([L dw]x) exp([w]x) to first order"""
  w = np.asarray(w, dtype=np.float64)
  t2 = float(w @ w)
  if t2 < 1e-8:
    b, c = 0.5 - t2 / 24.0, 1.0 / 6.0 - t2 / 120.0
  else:
    t = np.sqrt(t2)
    b, c = (1.0 - np.cos(t)) / t2, (t - np.sin(t)) / (t2 * t)
  K = skew(w)
  return np.eye(3) + b * K + c * (K @ K)


def pose_map(rtvec):
  """G [6, 6] = d(omega, tau) / d(rvec, tvec): the left perturbation T -> exp(omega, tau) T that a change of the stored pose
  parameters amounts to.  G = [[L, 0], [[t]x L, I]] -- view_pose_column of csrc/mcba_math.h with an identity prefix rotation."""
  rt = np.asarray(rtvec, dtype=np.float64).reshape(6)
  L = left_jacobian(rt[:3])
  G = np.zeros((6, 6))
  G[:3, :3] = L
  G[3:, :3] = skew(rt[3:]) @ L
  G[3:, 3:] = np.eye(3)
  return G


def camera_map(n_dist, fix_aspect):
  """[4 + n_dist, 5 + n_dist]: columns (fx fy cx cy dist..) of the device from the stored block (fx fy cx cy skew dist..); under
  fix_aspect the first stored focal length is both (camera.py:159-160); the skew enters neither projection"""
  M = np.zeros((4 + n_dist, 5 + n_dist))
  M[0, 0] = 1.0
  M[1, 0 if fix_aspect else 1] = 1.0
  M[2, 2] = M[3, 3] = 1.0
  for i in range(n_dist):
    M[4 + i, 5 + i] = 1.0
  return M


def factor(sigma):
  """F [p, r] with F F^T = sigma (symmetrised): eigenvectors scaled by the roots of the eigenvalues above p * eps * the largest"""
  S = 0.5 * (np.asarray(sigma, dtype=np.float64) + np.asarray(sigma, dtype=np.float64).T)
  if S.size == 0:
    return np.zeros((S.shape[0], 0))
  lam, V = np.linalg.eigh(S)
  top = float(lam.max()) if lam.size else 0.0
  keep = lam > max(len(lam) * np.finfo(np.float64).eps * top, 0.0)
  return V[:, keep] * np.sqrt(lam[keep])


class RigModel(object):
  """What a job needs of the rig: the cameras (fx = fy = the first focal length under fix_aspect, as the bundle adjustment reads
  them), their own coefficient counts, the stored pose parameters and the pose matrices."""

  def __init__(self, cameras, camera_poses, rtvecs=None):
    from . import transform
    from types import SimpleNamespace
    self.fix_aspect = [bool(getattr(c, "fix_aspect", False)) for c in cameras]
    self.cameras = []
    for c, fa in zip(cameras, self.fix_aspect):
      K = np.array(c.intrinsic, dtype=np.float64)
      if fa:
        K[0, 0] = K[1, 1] = 0.5 * (K[0, 0] + K[1, 1])       # (Camera.params: the mean of the two)
      self.cameras.append(SimpleNamespace(intrinsic=K, dist=np.asarray(c.dist, dtype=np.float64).ravel(),
                                          model="fisheye" if _is_fisheye(c) else "pinhole", image_size=getattr(c, "image_size", None)))
    self.n_dist = [4 if _is_fisheye(c) else int(c.dist.size) for c in self.cameras]
    self.poses = np.ascontiguousarray(_f64(camera_poses))
    assert self.poses.shape == (len(self.cameras), 4, 4), "camera_poses are [C, 4, 4]"
    self.rtvecs = transform.from_matrix(self.poses).reshape(-1, 6) if rtvecs is None else _f64(rtvecs).reshape(-1, 6)

  def stored_map(self, b, a):
    """M [K, p]: columns of the device (camera b | pose b | pose a | camera a) from the stored parameters in the same order"""
    blocks = [camera_map(self.n_dist[b], self.fix_aspect[b]), pose_map(self.rtvecs[b])]
    if a is not None:
      blocks += [pose_map(self.rtvecs[a]), camera_map(self.n_dist[a], self.fix_aspect[a])]
    M = np.zeros((sum(m.shape[0] for m in blocks), sum(m.shape[1] for m in blocks)))
    r = c = 0
    for m in blocks:
      M[r:r + m.shape[0], c:c + m.shape[1]] = m
      r, c = r + m.shape[0], c + m.shape[1]
    return M

  def stored_count(self, b, a):
    return (5 + self.n_dist[b]) + 6 + (0 if a is None else 6 + 5 + self.n_dist[a])


class Job(object):
  """One job of the call: camera b, reference a (None: the rig frame), distance, the covariance of the stored parameters
  (camera b | pose b | pose a | camera a) with zero rows where held, `loose` [p] (unobserved and not held), and its queries: grid
  (gw, gh, u0, v0, du, dv) or pixels [n, 2]."""

  def __init__(self, camera, reference, distance, sigma, loose=None, grid=None, pixels=None):
    self.camera, self.reference = int(camera), None if reference is None else int(reference)
    self.rho = 0.0 if np.isinf(distance) else 1.0 / float(distance)
    self.sigma = _f64(sigma)
    self.loose = np.zeros(len(self.sigma), dtype=bool) if loose is None else np.asarray(loose, dtype=bool)
    assert (grid is None) != (pixels is None), "a job has a grid or a list of pixels"
    self.grid = grid
    self.pixels = None if pixels is None else np.ascontiguousarray(_f64(pixels).reshape(-1, 2))

  @property
  def n(self):
    return self.grid[0] * self.grid[1] if self.grid is not None else len(self.pixels)

  def pixel_array(self):
    """[n, 2] the pixels of the job as the device generates them (a product and a sum, each rounded once)"""
    if self.grid is None:
      return self.pixels
    gw, gh, u0, v0, du, dv = self.grid
    u = u0 + np.arange(gw, dtype=np.float64) * du
    v = v0 + np.arange(gh, dtype=np.float64) * dv
    return np.stack(np.broadcast_arrays(u[None, :], v[:, None]), axis=-1).reshape(-1, 2)


def grid_of(image_size, grid):
  """(gw, gh, u0, v0, du, dv): centres u_i = (i + 0.5) W / gw - 0.5, so that grid = image_size is every pixel"""
  (W, H), (gw, gh) = image_size, grid
  du, dv = float(W) / gw, float(H) / gh
  return int(gw), int(gh), 0.5 * du - 0.5, 0.5 * dv - 0.5, du, dv


def run_jobs(rig, jobs, with_std=True):
  """mcba_projection_uncertainty over the jobs: (cov [n_total, 3], std [n_total] or None, status [n_total]), job after job"""
  inp = CameraSetInputs(rig.cameras)
  recs = (_lib.UncertaintyJob * max(len(jobs), 1))()
  keep = []
  for rec, job in zip(recs, jobs):
    p = rig.stored_count(job.camera, job.reference)
    assert job.sigma.shape == (p, p), f"the covariance of this job's stored parameters is [{p}, {p}]"
    sigma = np.where(job.loose[:, None] | job.loose[None, :], 0.0, job.sigma)
    M = rig.stored_map(job.camera, job.reference)
    W = np.ascontiguousarray(M @ factor(sigma))
    flags = np.ascontiguousarray(((np.abs(M) @ job.loose.astype(np.float64)) > 0).astype(np.uint8))
    rec.camera, rec.reference = job.camera, -1 if job.reference is None else job.reference
    rec.inv_distance = job.rho
    rec.K, rec.r = W.shape
    rec.W, rec.unconstrained = _dp(W), _up(flags)
    if job.grid is not None:
      rec.grid_w, rec.grid_h, rec.u0, rec.v0, rec.du, rec.dv = job.grid
    else:
      rec.grid_w, rec.grid_h, rec.n, rec.uv = 0, 0, len(job.pixels), _dp(job.pixels)
    keep += [W, flags]
  n = sum(job.n for job in jobs)
  cov, status = np.empty((n, 3)), np.empty(n, dtype=np.uint8)
  std = np.empty(n) if with_std else None
  _entry("projection_uncertainty")(C.byref(inp.struct()), _dp(rig.poses), len(jobs), recs, _dp(cov), _dp(std), _up(status))
  return cov, std, status


def covariance_matrices(cov3):
  """[..., 3] (uu uv vv) -> [..., 2, 2]"""
  return np.asarray(cov3)[..., [0, 1, 1, 2]].reshape(np.shape(cov3)[:-1] + (2, 2))


def stored_covariance(cov, index):
  """(sigma [p, p], loose [p]) of the stored parameters `index` [p] into param_vec (-1: not a parameter, contributes nothing) from a
  covariance struct (shared, shared_index, std, held): held rows are zero, an unobserved parameter (std NaN, not held) is loose"""
  index = np.asarray(index, dtype=np.int64)
  p = len(index)
  sigma, loose = np.zeros((p, p)), np.zeros(p, dtype=bool)
  where = {int(g): i for i, g in enumerate(np.asarray(cov.shared_index))}
  present = [k for k in range(p) if index[k] >= 0]
  rows = []
  for k in present:
    assert int(index[k]) in where, f"parameter {int(index[k])} is not a shared parameter of the covariance"
    rows.append(where[int(index[k])])
  if present:
    sigma[np.ix_(present, present)] = np.asarray(cov.shared)[np.ix_(rows, rows)]
    held = np.asarray(cov.held, dtype=bool)[index[present]] if "held" in cov else np.zeros(len(present), dtype=bool)
    loose[present] = np.isnan(np.asarray(cov.std)[index[present]]) & ~held
    dead = np.zeros(p, dtype=bool)
    dead[present] = held
    dead |= loose
    sigma[dead, :] = 0.0
    sigma[:, dead] = 0.0
  assert np.isfinite(sigma).all(), "the covariance of an observed parameter is not finite"
  return sigma, loose


def projection_uncertainty(cameras, camera_poses, cov, camera_index, pose_index, query_cameras=None, reference=None, distance=np.inf,
                           grid=(16, 12), pixels=None, rtvecs=None):
  """The functional entry: no Calibration needed.  cameras: anything with `intrinsic`, `dist`, `image_size` (and `fix_aspect`);
  camera_poses [C, 4, 4] rig -> camera (rtvecs [C, 6]: the stored parameters, default: from the matrices); cov: struct(shared,
  shared_index, std, held) of Calibration.covariance; camera_index[c] / pose_index[c]: where the stored block of camera c (fx fy cx
  cy skew dist..) / of its pose (6) sits in param_vec, or None where the block is not optimised.  One device call for all
  query_cameras (default: all).  Returns struct(cov [C', gh, gw, 2, 2], std [C', gh, gw], pixels [C', gh, gw, 2], status); with
  pixels [n, 2] and one camera: cov [n, 2, 2], std [n], pixels [n, 2], status [n]."""
  rig = RigModel(cameras, camera_poses, rtvecs)
  query = list(range(len(rig.cameras))) if query_cameras is None else [int(c) for c in np.atleast_1d(query_cameras)]
  if pixels is not None:
    assert len(query) == 1, "a list of pixels belongs to one camera"

  def block(index, c, n):
    return np.full(n, -1, dtype=np.int64) if index is None or index[c] is None else np.asarray(index[c], dtype=np.int64)

  jobs = []
  for b in query:
    idx = [block(camera_index, b, 5 + rig.n_dist[b]), block(pose_index, b, 6)]
    if reference is not None:
      a = int(reference)
      idx += [block(pose_index, a, 6), block(camera_index, a, 5 + rig.n_dist[a])]
    sigma, loose = stored_covariance(cov, np.concatenate(idx))
    where = dict(pixels=pixels) if pixels is not None else dict(grid=grid_of(cameras[b].image_size, grid))
    jobs.append(Job(b, reference, distance, sigma, loose, **where))
  c3, std, status = run_jobs(rig, jobs)
  px = np.concatenate([j.pixel_array() for j in jobs]) if jobs else np.zeros((0, 2))
  if pixels is not None:
    return struct(cov=covariance_matrices(c3), std=std, pixels=px, status=status)
  gw, gh = int(grid[0]), int(grid[1])
  shape = (len(query), gh, gw)
  return struct(cov=covariance_matrices(c3).reshape(shape + (2, 2)), std=std.reshape(shape), pixels=px.reshape(shape + (2,)),
                status=status.reshape(shape))


def last_call_ms():
  """mcba_debug_projection_uncertainty_ms of this thread's last call: (dict(upload, kernel, download, call) in ms, queries launched)."""
  return _lib.call_ms("projection_uncertainty", ("upload", "kernel", "download", "call"))
