"""Using a calibration: how well does this rig measure 3-D?  

One entry point of libmcba.so (csrc/mcba_recon.h): the 3 x 3 covariance of the point a camera group triangulates, under the
covariance of the calibration itself (cov_cal: systematic, the same for every point of a scene, growing with the square of the
distance) beside the pixel noise of the point alone (cov_noise = sigma2 H^-1, what triangulate() reports).

  reference=None   the point is expressed in the RIG frame (with the default hold: the frame of the held camera);
  reference=a      the point is expressed in the frame of camera a of the group: the gauge-free form, in which a common motion of
                   all camera poses cancels.

The value is exact for the point triangulated from its noise-free pixels; for a point that came out of triangulate() with non-zero
residuals it is the Gauss-Newton approximation at the model-projected pixels.  The motion model plays no part (the point is fixed
in the rig frame at one instant).

A second entry point serves PAIRS of points: the calibration's error is common to both ends of a measured
length and largely cancels in their difference, so the covariance of X_a - X_b, of |X_a - X_b| and the cross covariance of the two ends
come from the per-column difference of the two responses (pair_uncertainty, run_pair_jobs), never from cov_a + cov_b.

This module marshals: the per-camera factors of the joint covariance (guidance.rig_factors), the jobs, the points of a pixel grid
of the reference camera at a list of distances, the range / lateral standard deviations, and the pair lists.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import dp as _dp, entry as _entry, f64 as _f64, ip as _ip, up as _up   # noqa: F401 (_entry: see _lib.entry)
from .structs import struct
from .undistort import CameraSetInputs

OK, TOO_FEW, DEGENERATE, UNCONSTRAINED = _lib.RECON_OK, _lib.RECON_TOO_FEW, _lib.RECON_DEGENERATE, _lib.RECON_UNCONSTRAINED
MAX_CAMERAS, MAX_R, COLUMNS = _lib.RECON_MAX_CAMERAS, _lib.RIG_MAX_R, _lib.RIG_COLUMNS
_u64p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint64))
_i64p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))


class Job(object):
  """One job of the call: group (camera indices, slot order), reference (a camera of the group or None: the rig frame), factors[s] =
  (W [24, r], unconstrained) per slot with one r, points [n, 3] in the rig frame, masks [n] uint64 (bit s: slot s may be used) or
  None."""

  def __init__(self, group, reference, factors, points, masks=None):
    self.group = [int(c) for c in group]
    self.reference = None if reference is None else int(reference)
    self.factors = [(np.ascontiguousarray(_f64(W)), bool(loose)) for W, loose in factors]
    self.points = np.ascontiguousarray(_f64(points).reshape(-1, 3))
    self.masks = None if masks is None else np.ascontiguousarray(np.asarray(masks, dtype=np.uint64).reshape(-1))
    assert self.masks is None or len(self.masks) == len(self.points), "one mask per point"
    assert len(self.factors) == len(self.group), "one factor per camera of the group"


def _marshal(cameras, camera_poses, jobs):
  """what both entries take: (camera set inputs, poses [C, 3, 4], the job records, points [n, 3], masks [n] or None)"""
  inp = CameraSetInputs(cameras)
  poses = np.ascontiguousarray(_f64(camera_poses).reshape(len(cameras), 4, 4)[:, :3, :])
  recs = (_lib.ReconJob * max(len(jobs), 1))()
  any_mask = any(job.masks is not None for job in jobs)
  points = np.concatenate([job.points for job in jobs]) if jobs else np.zeros((0, 3))
  masks = np.concatenate([np.full(len(job.points), ~np.uint64(0)) if job.masks is None else job.masks for job in jobs]) if any_mask else None
  for rec, job in zip(recs, jobs):
    rec.G, rec.reference, rec.n = len(job.group), -1 if job.reference is None else job.reference, len(job.points)
    rec.r = job.factors[0][0].shape[1] if job.factors else 0
    for s, c in enumerate(job.group[:MAX_CAMERAS]):
      W, loose = job.factors[s]
      assert W.shape == (COLUMNS, rec.r), "every W of a job is [24, r] with one r"
      rec.cameras[s], rec.W[s], rec.unconstrained[s] = c, _dp(W), int(loose)
      if 0 <= c < len(cameras):
        rec.image_w[s], rec.image_h[s] = [float(x) for x in cameras[c].image_size]
  return inp, poses, recs, np.ascontiguousarray(points), None if masks is None else np.ascontiguousarray(masks)


def run_jobs(cameras, camera_poses, jobs, sigma2=1.0, margin=0.0):
  """mcba_reconstruction_uncertainty over the jobs, job after job: struct(cov_cal [n, 6], cov_noise [n, 6] (upper triangles), n_views
  [n], views [n] uint64, status [n]).  cameras: anything with intrinsic, dist, image_size; camera_poses [C, 4, 4] rig -> camera."""
  inp, poses, recs, points, masks = _marshal(cameras, camera_poses, jobs)
  n = len(points)
  out = struct(cov_cal=np.empty((n, 6)), cov_noise=np.empty((n, 6)), n_views=np.empty(n, dtype=np.int32),
               views=np.empty(n, dtype=np.uint64), status=np.empty(n, dtype=np.uint8))
  _entry("reconstruction_uncertainty")(C.byref(inp.struct()), _dp(poses), len(jobs), recs, _dp(points), _u64p(masks), float(sigma2),
                                       float(margin), _dp(out.cov_cal), _dp(out.cov_noise), _ip(out.n_views), _u64p(out.views),
                                       _up(out.status))
  return out


def run_pair_jobs(cameras, camera_poses, jobs, pairs, sigma2=1.0, margin=0.0):
  """mcba_reconstruction_pairs over the jobs (as for run_jobs) and, per job, pairs[j] [K_j, 2]: indices (a, b) into the job's own points.
  struct(cov_diff_cal [K, 6], cross_cal [K, 9] (row-major 3 x 3), cov_diff_noise [K, 6], length, length_var_cal, length_var_noise [K],
  views_a, views_b [K] uint64, status [K]), the pairs of a job after those of the job before it."""
  assert len(pairs) == len(jobs), "one pair list per job"
  inp, poses, recs, points, masks = _marshal(cameras, camera_poses, jobs)
  lists = [np.asarray(p, dtype=np.int64).reshape(-1, 2) for p in pairs]
  n_pairs = np.array([len(p) for p in lists] + [0], dtype=np.int64)
  table = np.ascontiguousarray(np.concatenate(lists + [np.zeros((0, 2), dtype=np.int64)]))
  K = len(table)
  out = struct(cov_diff_cal=np.empty((K, 6)), cross_cal=np.empty((K, 9)), cov_diff_noise=np.empty((K, 6)), length=np.empty(K),
               length_var_cal=np.empty(K), length_var_noise=np.empty(K), views_a=np.empty(K, dtype=np.uint64),
               views_b=np.empty(K, dtype=np.uint64), status=np.empty(K, dtype=np.uint8))
  _entry("reconstruction_pairs")(C.byref(inp.struct()), _dp(poses), len(jobs), recs, _dp(points), _u64p(masks), _i64p(n_pairs),
                                 _i64p(table), float(sigma2), float(margin), _dp(out.cov_diff_cal), _dp(out.cross_cal),
                                 _dp(out.cov_diff_noise), _dp(out.length), _dp(out.length_var_cal), _dp(out.length_var_noise),
                                 _u64p(out.views_a), _u64p(out.views_b), _up(out.status))
  return out


def covariance_matrices(cov6):
  """[..., 6] (xx xy xz yy yz zz) -> [..., 3, 3]"""
  return np.asarray(cov6)[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(np.shape(cov6)[:-1] + (3, 3))


def range_lateral_std(cov, direction):
  """(range_std, lateral_std) of covariances [n, 3, 3] along / across the unit vectors `direction` [n, 3]: the standard deviation
  along the vector, and the root of the largest eigenvalue of the covariance projected on the plane perpendicular to it"""
  cov, d = np.asarray(cov, dtype=np.float64), np.asarray(direction, dtype=np.float64)
  with np.errstate(invalid="ignore"):
    rng = np.sqrt(np.maximum(np.einsum("ni,nij,nj->n", d, cov, d), 0.0))
    Pm = np.eye(3)[None] - d[:, :, None] * d[:, None, :]
    across = Pm @ cov @ Pm
    ok = np.isfinite(across).all(axis=(1, 2))
    lam = np.full(len(cov), np.nan)
    if ok.any():
      lam[ok] = np.linalg.eigvalsh(0.5 * (across[ok] + across[ok].transpose(0, 2, 1)))[:, -1]
    return np.where(ok, rng, np.nan), np.sqrt(np.maximum(lam, 0.0))


def grid_points(cameras, camera_poses, camera, pixels, distances):
  """points [D, n, 3] in the rig frame: the pixels [n, 2] of `camera` at the distances [D] from its centre (the device's
  undistort_points and T_camera^-1); NaN where the model cannot have produced the pixel"""
  from . import undistort
  xy, _ = undistort.undistort_points([cameras[camera]], pixels)
  ray = np.concatenate([xy, np.ones((len(xy), 1))], axis=1)
  ray /= np.linalg.norm(ray, axis=1, keepdims=True)
  T = np.linalg.inv(_f64(camera_poses)[camera])
  Y = np.asarray(distances, dtype=np.float64).reshape(-1, 1, 1) * ray[None]
  return Y @ T[:3, :3].T + T[:3, 3]


def _group_factors(who, cameras, camera_poses, cov, camera_index, pose_index, group, rtvecs):
  """(the full RigModel, the members of the group, the RigModel of the group, its per-slot factors of `cov`, r)"""
  from . import guidance, uncertainty
  full = uncertainty.RigModel(cameras, camera_poses, rtvecs)
  members = list(range(len(cameras))) if group is None else [int(c) for c in np.atleast_1d(group)]
  if not 2 <= len(members) <= MAX_CAMERAS:
    raise ValueError(f"{who}: group of {len(members)} cameras: a group has 2 .. {MAX_CAMERAS} cameras")
  rig = uncertainty.RigModel([cameras[c] for c in members], full.poses[members], full.rtvecs[members])
  pick = lambda index: None if index is None else [index[c] for c in members]
  factors, r = guidance.rig_factors(rig, cov, pick(camera_index), pick(pose_index))
  return full, members, rig, factors, r


def reconstruction_uncertainty(cameras, camera_poses, cov, camera_index, pose_index, group=None, reference=None, points=None,
                               pixels=None, grid=(16, 12), distances=None, masks=None, sigma2=None, margin=0.0, rtvecs=None):
  """The functional entry: no Calibration needed.  cameras, camera_poses [C, 4, 4] (rtvecs [C, 6]: the stored parameters), cov,
  camera_index, pose_index as for uncertainty.projection_uncertainty; group: 2 .. 8 camera indices (None: all); reference: a camera of
  the group (the result is in its frame) or None (the rig frame).  points [n, 3] in the rig frame with masks [n] (bit s: slot s of the
  group may be used), or -- without points -- the pixels [n, 2] (default: the centres of `grid`) of the reference camera (None: the
  first of the group) at every one of `distances` from that camera.  sigma2: None = cov.sigma2.
  Returns struct(cov_cal, cov_noise, cov_total [N, 3, 3], n_views, views, status [N], points [N, 3], range_std_cal, lateral_std_cal,
  range_std_noise, lateral_std_noise [N] along / across the unit vector from the reference origin (the rig origin without a
  reference camera), r); from a grid N = D gh gw and every array is [D, gh, gw, ...], from pixels [D, n, ...]."""
  from . import uncertainty
  full, members, rig, factors, r = _group_factors("reconstruction_uncertainty", cameras, camera_poses, cov, camera_index, pose_index,
                                                  group, rtvecs)
  shape = None
  if points is None:
    assert distances is not None, "without points: distances from the reference camera"
    a = members[0] if reference is None else int(reference)
    if pixels is None:
      g = uncertainty.grid_of(cameras[a].image_size, grid)
      px = uncertainty.Job(0, None, 1.0, np.zeros((0, 0)), grid=g).pixel_array()
      shape = (len(np.atleast_1d(distances)), g[1], g[0])
    else:
      px = _f64(pixels).reshape(-1, 2)
      shape = (len(np.atleast_1d(distances)), len(px))
    points = grid_points(full.cameras, full.poses, a, px, np.atleast_1d(distances)).reshape(-1, 3)
    lost = ~np.isfinite(points).all(axis=1)
    if lost.any():                                       # a pixel the model cannot have produced: a point no camera sees
      masks = np.where(lost, np.uint64(0), ~np.uint64(0) if masks is None else np.asarray(masks, dtype=np.uint64).reshape(-1))
      points = np.where(lost[:, None], 0.0, points)
  points = _f64(points).reshape(-1, 3)
  s2 = float(cov.sigma2) if sigma2 is None else float(sigma2)
  if reference is not None and int(reference) not in members:
    raise ValueError(f"reconstruction_uncertainty: reference {reference} is not a camera of the group {members}")
  ref_slot = None if reference is None else members.index(int(reference))
  out = run_jobs(rig.cameras, rig.poses, [Job(list(range(len(members))), ref_slot, factors, points, masks)], s2, margin)
  return finish(out, rig.poses, ref_slot, points, r, shape)


def finish(out, poses, ref_slot, points, r, shape=None):
  """the struct of reconstruction_uncertainty from the raw outputs of one job"""
  cal, noise = covariance_matrices(out.cov_cal), covariance_matrices(out.cov_noise)
  T = np.eye(4) if ref_slot is None else _f64(poses)[ref_slot]
  Y = points @ T[:3, :3].T + T[:3, 3]
  with np.errstate(invalid="ignore", divide="ignore"):
    d = Y / np.linalg.norm(Y, axis=1, keepdims=True)
  rc, lc = range_lateral_std(cal, d)
  rn, ln = range_lateral_std(noise, d)
  res = struct(cov_cal=cal, cov_noise=noise, cov_total=cal + noise, n_views=out.n_views, views=out.views, status=out.status,
               points=points, range_std_cal=rc, lateral_std_cal=lc, range_std_noise=rn, lateral_std_noise=ln)
  if shape is not None:
    res = struct(**{k: np.asarray(v).reshape(shape + np.shape(v)[1:]) for k, v in res.items()})
  return res._extend(r=r)


# ---- pairs of points: the uncertainty of a measured length ----------------------------------------------
def cross_matrices(cross9):
  """[..., 9] (row-major) -> [..., 3, 3]"""
  return np.asarray(cross9).reshape(np.shape(cross9)[:-1] + (3, 3))


def finish_pairs(out, r):
  """the struct of pair_uncertainty from the raw outputs of run_pair_jobs"""
  cal, noise = covariance_matrices(out.cov_diff_cal), covariance_matrices(out.cov_diff_noise)
  with np.errstate(invalid="ignore"):
    std = lambda var: np.sqrt(np.maximum(var, 0.0))           # (NaN stays NaN)
    return struct(cov_diff_cal=cal, cov_diff_noise=noise, cov_diff_total=cal + noise, cross_cal=cross_matrices(out.cross_cal),
                  length=out.length, length_std_cal=std(out.length_var_cal), length_std_noise=std(out.length_var_noise),
                  length_std=std(out.length_var_cal + out.length_var_noise), status=out.status, views_a=out.views_a,
                  views_b=out.views_b, r=r)


def pair_uncertainty(cameras, camera_poses, cov, camera_index, pose_index, points_a=None, points_b=None, points=None, pairs=None,
                     group=None, reference=None, masks=None, sigma2=None, margin=0.0, rtvecs=None):
  """The functional entry of the pair form: no Calibration needed.  cameras .. pose_index, group, reference, sigma2, margin, rtvecs as
  for reconstruction_uncertainty.  Either points_a, points_b [K, 3] (rig frame; masks: None or (masks_a, masks_b), [K] each), or
  points [n, 3] with pairs [K, 2] of indices into them (masks [n]): the second form computes nothing more than the first, but says
  which ends are one point (a == b is exactly 0).
  Returns struct(cov_diff_cal, cov_diff_noise, cov_diff_total [K, 3, 3]: the covariance of X_a - X_b under the calibration's covariance
  / the pixel noise of the two points / both; cross_cal [K, 3, 3] = cov(X_a, X_b) under the calibration; length [K] = |X_a - X_b|;
  length_std_cal, length_std_noise, length_std [K]; status [K] (that of a unless OK, then that of b; NaN unless OK); views_a, views_b
  [K] uint64; r)."""
  _, members, rig, factors, r = _group_factors("pair_uncertainty", cameras, camera_poses, cov, camera_index, pose_index, group, rtvecs)
  if points is None:
    assert points_a is not None and points_b is not None and pairs is None, "points_a and points_b, or points and pairs"
    a, b = _f64(points_a).reshape(-1, 3), _f64(points_b).reshape(-1, 3)
    assert len(a) == len(b), "one b end per a end"
    points, pairs = np.concatenate([a, b]), np.stack([np.arange(len(a)), len(a) + np.arange(len(a))], axis=1)
    if masks is not None:
      masks = np.concatenate([np.asarray(m, dtype=np.uint64).reshape(-1) for m in masks])
  else:
    assert points_a is None and points_b is None and pairs is not None, "points_a and points_b, or points and pairs"
  points = _f64(points).reshape(-1, 3)
  s2 = float(cov.sigma2) if sigma2 is None else float(sigma2)
  if reference is not None and int(reference) not in members:
    raise ValueError(f"pair_uncertainty: reference {reference} is not a camera of the group {members}")
  ref_slot = None if reference is None else members.index(int(reference))
  out = run_pair_jobs(rig.cameras, rig.poses, [Job(list(range(len(members))), ref_slot, factors, points, masks)], [pairs], s2, margin)
  return finish_pairs(out, r)


def farthest_corner_pairs(board_points):
  """[P, 2]: per corner p of a board (points [P, 3] in its own frame) the pair (p, the corner farthest from p, ties to the lowest
  index): long baselines, every corner once as an a end, the same list whichever corners were seen"""
  x = _f64(board_points).reshape(-1, 3)
  d = np.linalg.norm(x[:, None] - x[None], axis=-1)
  return np.stack([np.arange(len(x)), np.argmax(d, axis=1)], axis=1).astype(np.int64)


def last_pair_call_ms():
  """mcba_debug_reconstruction_pairs_ms of this thread's last call: (dict(upload, kernel, download, call) in ms, pairs launched)."""
  return _lib.call_ms("reconstruction_pairs", ("upload", "kernel", "download", "call"))


def last_call_ms():
  """mcba_debug_reconstruction_uncertainty_ms of this thread's last call: (dict(upload, kernel, download, call) in ms, points
  launched)."""
  return _lib.call_ms("reconstruction_uncertainty", ("upload", "kernel", "download", "call"))
