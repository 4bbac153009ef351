"""Planning the next captures: where should the board be held so that the calibration gets better?  

One entry point of libmcba.so (csrc/mcba_guidance.h): per candidate view -- camera c sees a board at a board-in-camera pose in a new
frame whose rig pose is free -- the Schur complement S_v of the view's own pose in the Gram matrix of its whitened rows, the expected
information gain (log det(B + S_v / sigma2) - log det B) / 2 and the RMS projection uncertainty over a focus grid after the view,
and a greedy selection of n views per camera on the device.  A second entry point (csrc/mcba_rigview.h, section 3.17) scores
views that several cameras of a group see at once: they inform the camera poses too, and the focus is the transfer uncertainty
between the cameras.

This module marshals: the factor W_c = M_c F of a camera's intrinsics covariance (uncertainty.factor and camera_map), candidate
poses (host numpy), views and foci, and the outputs.
"""
import ctypes as C

import numpy as np

from . import _lib, uncertainty
from ._lib import dp as _dp, entry as _entry, f64 as _f64, ip as _ip, up as _up   # noqa: F401 (_entry: see _lib.entry)
from .structs import struct
from .undistort import CameraSetInputs

OK, TOO_FEW, DEGENERATE, UNCONSTRAINED = _lib.GUIDE_OK, _lib.GUIDE_TOO_FEW, _lib.GUIDE_DEGENERATE, _lib.GUIDE_UNCONSTRAINED
CRITERIA = dict(focus=_lib.GUIDE_BY_FOCUS, gain=_lib.GUIDE_BY_GAIN)
MAX_R = _lib.GUIDE_MAX_R
DEFAULT_TILTS = ((0.0, 0.0), (30.0, 0.0), (-30.0, 0.0), (0.0, 30.0), (0.0, -30.0))   # degrees about x, about y


class View(object):
  """camera c sees board b at the board-in-camera pose T [4, 4] (or [3, 4]); n_nuisance free parameters of the view's own"""

  def __init__(self, camera, board, pose, n_nuisance=6, min_points=4):
    self.camera, self.board, self.n_nuisance, self.min_points = int(camera), int(board), int(n_nuisance), int(min_points)
    self.pose = np.ascontiguousarray(_f64(pose)[:3, :4])


class Focus(object):
  """the region of camera c that matters: grid (gw, gh, u0, v0, du, dv) or pixels [n, 2], at `distance` (inf: directions); the
  implied rotation (distance inf) or rigid motion is fitted out unless n_nuisance says otherwise"""

  def __init__(self, camera, distance=np.inf, grid=None, pixels=None, n_nuisance=None, min_points=4):
    assert (grid is None) != (pixels is None), "a focus has a grid or a list of pixels"
    self.camera, self.min_points = int(camera), int(min_points)
    self.rho = 0.0 if np.isinf(distance) else 1.0 / float(distance)
    self.n_nuisance = (3 if self.rho == 0.0 else 6) if n_nuisance is None else int(n_nuisance)
    self.grid = grid
    self.pixels = None if pixels is None else np.ascontiguousarray(_f64(pixels).reshape(-1, 2))


def camera_factor(cov, index, n_dist, fix_aspect):
  """(W [4 + n_dist, r], unconstrained) of a camera whose stored block fx fy cx cy skew dist.. sits at `index` in param_vec (None:
  the block is not optimised, r = 0), formed exactly as uncertainty.run_jobs forms the W of a job"""
  M = uncertainty.camera_map(n_dist, fix_aspect)
  if index is None:
    return np.zeros((4 + n_dist, 0)), False
  sigma, loose = uncertainty.stored_covariance(cov, np.asarray(index, dtype=np.int64))
  W = np.ascontiguousarray(M @ uncertainty.factor(sigma))
  return W, bool(((np.abs(M) @ loose.astype(np.float64)) > 0).any())


def _rays(camera, pixels):
  """unit rays [n, 3] of pixels [n, 2]: Newton on the numpy projection from the distortion-free start"""
  from . import synthetic
  from .tables import _is_fisheye
  K, dist = np.asarray(camera.intrinsic, dtype=np.float64), np.asarray(camera.dist, dtype=np.float64).ravel()
  project = synthetic.project_fisheye if _is_fisheye(camera) else synthetic.project_pinhole
  px = _f64(pixels).reshape(-1, 2)
  xy = np.stack([(px[:, 0] - K[0, 2]) / K[0, 0], (px[:, 1] - K[1, 2]) / K[1, 1]], axis=1)
  h = 1e-6
  for _ in range(8):
    def at(dx, dy):
      return project(np.concatenate([xy + [dx, dy], np.ones((len(xy), 1))], axis=1), K, dist)
    p0 = at(0.0, 0.0)
    J = np.stack([(at(h, 0.0) - at(-h, 0.0)) / (2 * h), (at(0.0, h) - at(0.0, -h)) / (2 * h)], axis=2)
    with np.errstate(all="ignore"):
      step = np.linalg.solve(J + 1e-12 * np.eye(2), (p0 - px)[:, :, None])[:, :, 0]
    xy = xy - np.where(np.isfinite(step), step, 0.0)
  n = np.concatenate([xy, np.ones((len(xy), 1))], axis=1)
  return n / np.linalg.norm(n, axis=1, keepdims=True)


def candidate_poses(camera, board, centres=(7, 5), distances=None, tilts_deg=DEFAULT_TILTS):
  """Board-in-camera poses [n, 4, 4] (host numpy): the board's centre on the rays of a centres[0] x centres[1] pixel grid, at each
  of `distances` (default: those at which the board's width spans half of, and the whole of, the image width), facing the camera
  and tilted by each (about x, about y) of tilts_deg."""
  from scipy.spatial.transform import Rotation
  pts = _f64(getattr(board, "adjusted_points", board)).reshape(-1, 3)
  centre = 0.5 * (pts.min(axis=0) + pts.max(axis=0))
  width = float((pts.max(axis=0) - pts.min(axis=0))[0])
  W, H = camera.image_size
  fx = float(np.asarray(camera.intrinsic)[0, 0])
  if distances is None:
    distances = (2.0 * fx * width / W, fx * width / W)
  gw, gh, u0, v0, du, dv = uncertainty.grid_of((W, H), centres)
  px = np.stack(np.broadcast_arrays((u0 + np.arange(gw) * du)[None, :], (v0 + np.arange(gh) * dv)[:, None]), axis=-1).reshape(-1, 2)
  rays = _rays(camera, px)
  out = []
  for d in distances:
    for ray in rays:
      for ax, ay in tilts_deg:
        R = Rotation.from_euler("xy", [ax, ay], degrees=True).as_matrix()
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = ray * (float(d) / ray[2]) - R @ centre
        out.append(T)
  return np.array(out).reshape(-1, 4, 4)


def _fill_view(rec, v, keep):
  rec.camera, rec.n_nuisance, rec.min_points = v.camera, v.n_nuisance, v.min_points
  if isinstance(v, View):
    rec.board = v.board
    rec.pose[:] = list(v.pose.ravel())
    return
  rec.board, rec.inv_distance = -1, v.rho
  if v.grid is not None:
    rec.grid_w, rec.grid_h, rec.u0, rec.v0, rec.du, rec.dv = v.grid
  else:
    rec.grid_w, rec.grid_h, rec.n, rec.uv = 0, 0, len(v.pixels), _dp(v.pixels)
    keep.append(v.pixels)


def view_information(cameras, factors, boards, views, foci=None, n=0, criterion="focus", sigma2=1.0, margin=0.0, with_S=True,
                     with_rounds=False):
  """mcba_view_information: cameras (anything with intrinsic, dist, image_size; fx = fy under fix_aspect is the caller's business:
  pass uncertainty.RigModel(...).cameras), factors[c] = (W [KI_c, r], unconstrained), boards: list of [P_b, 3], views: list of
  View, foci: None or one Focus / None per camera.  Returns struct(n_visible, status, gain, focus_rms [V] against the base I; S
  [V, rs, rs]; focus_status, focus_n_visible, focus_before [C]; Q [C, rs, rs]; picks [C, n] (-1: none), pick_gain, pick_focus_rms;
  posterior [C, rs, rs]; round_gain, round_focus_rms [n, V] with with_rounds; r [C])."""
  inp = CameraSetInputs(cameras)
  Cn, V = len(cameras), len(views)
  keep = []
  info = (_lib.GuidanceCamera * Cn)()
  for c, (W, loose) in enumerate(factors):
    W = np.ascontiguousarray(_f64(W))
    keep.append(W)
    info[c].r, info[c].unconstrained, info[c].W = W.shape[1], int(bool(loose)), _dp(W)
    info[c].image_w, info[c].image_h = [float(x) for x in cameras[c].image_size]
  stride = max([len(b) for b in boards] + [1])
  table = np.zeros((max(len(boards), 1), stride, 3))
  for b, pts in enumerate(boards):
    table[b, :len(pts)] = _f64(pts).reshape(-1, 3)
  board_n = np.array([len(b) for b in boards] + [0] * (0 if boards else 1), dtype=np.int32)
  recs = (_lib.GuidanceView * max(V, 1))()
  for rec, v in zip(recs, views):
    _fill_view(rec, v, keep)
  frecs = None
  if foci is not None:
    frecs = (_lib.GuidanceView * Cn)()
    for c in range(Cn):
      frecs[c].camera = -1
      if foci[c] is not None:
        assert foci[c].camera == c, "foci[c] is the focus of camera c"
        _fill_view(frecs[c], foci[c], keep)
  rs = max([1] + [int(info[c].r) for c in range(Cn)])
  out = struct(n_visible=np.zeros(V, dtype=np.int32), status=np.zeros(V, dtype=np.uint8), gain=np.zeros(V), focus_rms=np.zeros(V),
               S=np.zeros((V, rs, rs)) if with_S else None, focus_status=np.zeros(Cn, dtype=np.uint8),
               focus_n_visible=np.zeros(Cn, dtype=np.int32), focus_before=np.zeros(Cn), Q=np.zeros((Cn, rs, rs)),
               picks=np.zeros((Cn, n), dtype=np.int32), pick_gain=np.zeros((Cn, n)), pick_focus_rms=np.zeros((Cn, n)),
               posterior=np.zeros((Cn, rs, rs)), round_gain=np.zeros((n, V)) if with_rounds else None,
               round_focus_rms=np.zeros((n, V)) if with_rounds else None)
  res = _lib.GuidanceResult(_ip(out.n_visible), _up(out.status), _dp(out.gain), _dp(out.focus_rms), _dp(out.S), _up(out.focus_status),
                            _ip(out.focus_n_visible), _dp(out.focus_before), _dp(out.Q), _ip(out.picks), _dp(out.pick_gain),
                            _dp(out.pick_focus_rms), _dp(out.posterior), _dp(out.round_gain), _dp(out.round_focus_rms))
  _entry("view_information")(C.byref(inp.struct()), info, len(boards), stride, _ip(board_n), _dp(table), float(margin), float(sigma2), V,
                             recs, frecs, int(n), CRITERIA[criterion], C.byref(res))
  return out._extend(r=np.array([int(info[c].r) for c in range(Cn)]))


def suggest_views(cameras, cov, camera_index, boards, n=3, query_cameras=None, board=0, candidates=None, focus_grid=(16, 12),
                  focus_distance=np.inf, criterion="focus", margin=0.0, min_points=4):
  """The functional entry: no Calibration needed.  cameras: anything with intrinsic, dist, image_size (and fix_aspect); cov: struct
  of Calibration.covariance; camera_index[c]: where the stored block of camera c sits in param_vec (None: not optimised); boards:
  list of objects with adjusted_points (or arrays [P, 3]); candidates: None (candidate_poses per camera) or {camera: poses
  [n, 4, 4]}.  Returns struct(cameras [C'], poses [C', n, 4, 4] (NaN where no candidate is left), candidate_index, gain,
  focus_rms_before, focus_rms_after, n_visible [C', n], status [C'] (OK, UNCONSTRAINED, or TOO_FEW: no candidate is usable),
  candidates, scores: the struct of view_information)."""
  rig = uncertainty.RigModel(cameras, np.tile(np.eye(4), (len(cameras), 1, 1)), np.zeros((len(cameras), 6)))
  query = list(range(len(cameras))) if query_cameras is None else [int(c) for c in np.atleast_1d(query_cameras)]
  factors = [camera_factor(cov, None if camera_index is None or c not in query else camera_index[c], rig.n_dist[c], rig.fix_aspect[c])
             for c in range(len(cameras))]
  tables = [_f64(getattr(b, "adjusted_points", b)).reshape(-1, 3) for b in boards]
  views, first, poses = [], {}, {}
  for c in query:
    T = candidate_poses(rig.cameras[c], tables[board]) if candidates is None else _f64(candidates[c]).reshape(-1, 4, 4)
    first[c], poses[c] = len(views), T
    views += [View(c, board, t, 6, min_points) for t in T]
  foci = [Focus(c, focus_distance, grid=uncertainty.grid_of(cameras[c].image_size, focus_grid)) if c in query else None
          for c in range(len(cameras))]
  s = view_information(rig.cameras, factors, tables, views, foci, n=n, criterion=criterion, sigma2=float(cov.sigma2), margin=margin,
                       with_S=False)
  picked = np.full((len(query), n, 4, 4), np.nan)
  index = np.full((len(query), n), -1, dtype=np.int64)
  n_visible = np.zeros((len(query), n), dtype=np.int64)
  status = np.zeros(len(query), dtype=np.uint8)
  for i, c in enumerate(query):
    mine = slice(first[c], first[c] + len(poses[c]))
    status[i] = UNCONSTRAINED if factors[c][1] else OK if (s.status[mine] == OK).any() else TOO_FEW
    for k in range(n):
      v = int(s.picks[c, k])
      if v >= 0:
        index[i, k], picked[i, k], n_visible[i, k] = v - first[c], poses[c][v - first[c]], s.n_visible[v]
  return struct(cameras=np.array(query), poses=picked, candidate_index=index, gain=s.pick_gain[query],
                focus_rms_before=s.focus_before[query], focus_rms_after=s.pick_focus_rms[query], n_visible=n_visible, status=status,
                candidates=poses, scores=s)


# ---- views seen by several cameras (csrc/mcba_rigview.h) ------------------------------------------------
RIG_MAX_R, RIG_COLUMNS = _lib.RIG_MAX_R, _lib.RIG_COLUMNS


class RigView(object):
  """board b at the board-in-rig pose Z [4, 4] (or [3, 4]) in a new frame with a free rig pose; a camera contributes with at least
  min_points visible corners"""

  def __init__(self, board, pose, min_points=4):
    self.board, self.min_points = int(board), int(min_points)
    self.pose = np.ascontiguousarray(_f64(pose)[:3, :4])


class RigFocus(object):
  """what matters to the rig: the pixels of a grid (gw, gh, u0, v0, du, dv) of camera `reference` at `distance` (inf: directions),
  transferred into every camera of `members`"""

  def __init__(self, reference, members, grid, distance=np.inf):
    self.reference, self.members = int(reference), np.ascontiguousarray(np.asarray(members, dtype=np.int32).ravel())
    self.grid = grid
    self.rho = 0.0 if np.isinf(distance) else 1.0 / float(distance)


def scaled_factor(sigma):
  """uncertainty.factor of the correlation matrix, scaled back: F F^T = sigma.  Focal lengths (variances of pixels^2) and poses
  (variances of 1e-8) share this matrix; factoring it as it stands leaves the small entries with the absolute error of the large"""
  sigma = _f64(sigma)
  d = np.sqrt(np.diag(sigma))
  d = np.where(d > 0, d, 1.0)
  return d[:, None] * uncertainty.factor(sigma / np.outer(d, d))


def rig_factors(rig, cov, camera_index, pose_index):
  """(factors, r): factors[c] = (W_c [24, r], unconstrained) for every camera of the uncertainty.RigModel `rig`, from ONE factor F of
  the joint covariance of all their stored blocks (camera fx fy cx cy skew dist.. | pose rvec tvec per camera; an index of None: the
  block is not optimised): W_c = blockdiag(camera map padded to 18 rows, pose map) F[rows of c]"""
  Cn = len(rig.cameras)

  def block(index, c, n):
    return np.full(n, -1, dtype=np.int64) if index is None or index[c] is None else np.asarray(index[c], dtype=np.int64)

  idx, rows, at = [], [], 0
  for c in range(Cn):
    n = 5 + rig.n_dist[c] + 6
    idx += [block(camera_index, c, 5 + rig.n_dist[c]), block(pose_index, c, 6)]
    rows.append(np.arange(at, at + n))
    at += n
  sigma, loose = uncertainty.stored_covariance(cov, np.concatenate(idx))
  F = scaled_factor(sigma)
  return [rig_device_factor(rig, c, F[rows[c]], loose[rows[c]]) for c in range(Cn)], F.shape[1]


def rig_device_factor(rig, c, F_c, loose_c=None):
  """(W_c [24, r], unconstrained) from the rows F_c [5 + n_dist + 6, r] of a factor over the stored blocks of camera c"""
  nd = rig.n_dist[c]
  M = np.zeros((RIG_COLUMNS, 5 + nd + 6))
  M[:4 + nd, :5 + nd] = uncertainty.camera_map(nd, rig.fix_aspect[c])
  M[18:, 5 + nd:] = uncertainty.pose_map(rig.rtvecs[c])
  unconstrained = False if loose_c is None else bool(((np.abs(M) @ np.asarray(loose_c, dtype=np.float64)) > 0).any())
  return np.ascontiguousarray(M @ _f64(F_c)), unconstrained


def rig_view_information(cameras, camera_poses, factors, boards, views, focus=None, n=0, criterion="focus", sigma2=1.0, margin=0.0,
                         min_cameras=2, with_A=True, with_rounds=False, boards_free=False, workspace_mb=1024):
  """mcba_rig_view_information: cameras: the group (as for view_information), camera_poses [C, 4, 4] rig -> camera, factors[c] =
  (W_c [24, r], unconstrained) with one r (rig_factors), boards: list of [P_b, 3], views: list of RigView, focus: None or a RigFocus.
  Returns struct(n_cameras [V], n_visible [V, C], status, gain, focus_rms [V] against the base I; A [V, rs, rs] (sigma2 A_v);
  focus_status, focus_n, focus_before; Q [rs, rs]; picks [n] (-1: none), pick_gain, pick_focus_rms; posterior [rs, rs];
  round_gain, round_focus_rms [n, V] with with_rounds; r)."""
  inp = CameraSetInputs(cameras)
  Cn, V = len(cameras), len(views)
  poses = np.ascontiguousarray(_f64(camera_poses).reshape(Cn, 4, 4)[:, :3, :])
  keep = []
  info = (_lib.RigCamera * max(Cn, 1))()
  r = None
  for c, (W, loose) in enumerate(factors):
    W = np.ascontiguousarray(_f64(W))
    assert W.ndim == 2 and W.shape[0] == RIG_COLUMNS and r in (None, W.shape[1]), "every W_c is [24, r] with one r"
    r = W.shape[1]
    keep.append(W)
    info[c].unconstrained, info[c].W = int(bool(loose)), _dp(W)
    info[c].image_w, info[c].image_h = [float(x) for x in cameras[c].image_size]
  r = 0 if r is None else int(r)
  stride = max([len(b) for b in boards] + [1])
  table = np.zeros((max(len(boards), 1), stride, 3))
  for b, pts in enumerate(boards):
    table[b, :len(pts)] = _f64(pts).reshape(-1, 3)
  board_n = np.array([len(b) for b in boards] + [0] * (0 if boards else 1), dtype=np.int32)
  recs = (_lib.RigView * max(V, 1))()
  for rec, v in zip(recs, views):
    rec.board, rec.min_points = v.board, v.min_points
    rec.pose[:] = list(v.pose.ravel())
  frec = None
  if focus is not None:
    frec = _lib.RigFocus()
    frec.reference, frec.n_members, frec.members = focus.reference, len(focus.members), _ip(focus.members)
    frec.grid_w, frec.grid_h, frec.u0, frec.v0, frec.du, frec.dv = focus.grid
    frec.inv_distance = focus.rho
  rs = max(1, r)
  big = r > RIG_MAX_R or V * rs * rs * 8 > workspace_mb * 2 ** 20          # (the call refuses these: no output is needed)
  out = struct(n_cameras=np.zeros(V, dtype=np.int32), n_visible=np.zeros((V, Cn), dtype=np.int32), status=np.zeros(V, dtype=np.uint8),
               gain=np.zeros(V), focus_rms=np.zeros(V), A=np.zeros((V, rs, rs)) if with_A and not big else None,
               focus_status=np.zeros(1, dtype=np.uint8), focus_n=np.zeros(1, dtype=np.int32), focus_before=np.zeros(1),
               Q=None if big else np.zeros((rs, rs)), picks=np.zeros(n, dtype=np.int32), pick_gain=np.zeros(n), pick_focus_rms=np.zeros(n),
               posterior=None if big else np.zeros((rs, rs)), round_gain=np.zeros((n, V)) if with_rounds else None,
               round_focus_rms=np.zeros((n, V)) if with_rounds else None)
  res = _lib.RigResult(_ip(out.n_cameras), _ip(out.n_visible), _up(out.status), _dp(out.gain), _dp(out.focus_rms), _dp(out.A),
                       _up(out.focus_status), _ip(out.focus_n), _dp(out.focus_before), _dp(out.Q), _ip(out.picks), _dp(out.pick_gain),
                       _dp(out.pick_focus_rms), _dp(out.posterior), _dp(out.round_gain), _dp(out.round_focus_rms))
  _entry("rig_view_information")(C.byref(inp.struct()), _dp(poses), r, info, int(bool(boards_free)), len(boards), stride, _ip(board_n),
                                 _dp(table), V, recs, int(min_cameras), float(margin), float(sigma2),
                                 None if frec is None else C.byref(frec), int(n), CRITERIA[criterion], int(workspace_mb), C.byref(res))
  return out._extend(r=r, focus_status=int(out.focus_status[0]), focus_n=int(out.focus_n[0]), focus_before=float(out.focus_before[0]))


def rig_candidate_poses(cameras, camera_poses, board, **kwargs):
  """Board-in-rig poses [n, 4, 4]: the union of candidate_poses(camera, board, ...) of every camera, each moved to the rig frame
  (Z = T_c^-1 T), camera after camera; and which camera each was made for [n]"""
  poses, owner = [], []
  for c, cam in enumerate(cameras):
    T = candidate_poses(cam, board, **kwargs)
    poses.append(np.linalg.inv(_f64(camera_poses[c]))[None] @ T)
    owner += [c] * len(T)
  return np.concatenate(poses).reshape(-1, 4, 4), np.array(owner, dtype=np.int64)


def suggest_rig_views(cameras, camera_poses, cov, camera_index, pose_index, boards, n=3, group=None, reference=None, board=0,
                      candidates=None, focus_grid=(16, 12), focus_distance=None, criterion="focus", min_cameras=2, margin=0.0,
                      min_points=4, rtvecs=None, boards_free=False, workspace_mb=1024):
  """The functional entry: no Calibration needed.  cameras, camera_poses [C, 4, 4] (rtvecs [C, 6]: the stored parameters), cov,
  camera_index, pose_index as for uncertainty.projection_uncertainty; group: the cameras that take part (indices; None: all);
  reference: the camera whose pixels the focus transfers into the others (None: the first of the group); candidates: None
  (rig_candidate_poses of the group) or poses [m, 4, 4] board in rig; focus_distance: None = the median distance of the candidates'
  board centres from the reference camera.  Returns struct(cameras (the group), reference, focus_distance, poses [n, 4, 4] board in
  rig (NaN where no candidate is left), camera_poses_of_board [n, C', 4, 4] board in each camera of the group, candidate_index [n],
  gain [n] (nats, each conditional on the earlier picks), focus_rms_before, focus_rms_after [n] (px), n_cameras [n], n_visible
  [n, C'], status (OK, UNCONSTRAINED, or TOO_FEW: no candidate is usable), candidates, scores: the struct of rig_view_information)."""
  full = uncertainty.RigModel(cameras, camera_poses, rtvecs)
  members = list(range(len(cameras))) if group is None else [int(c) for c in np.atleast_1d(group)]
  a = members[0] if reference is None else int(reference)
  assert a in members, "the reference camera belongs to the group"
  rig = uncertainty.RigModel([cameras[c] for c in members], full.poses[members], full.rtvecs[members])
  pick = lambda index: None if index is None else [index[c] for c in members]
  factors, r = rig_factors(rig, cov, pick(camera_index), pick(pose_index))
  tables = [_f64(getattr(b, "adjusted_points", b)).reshape(-1, 3) for b in boards]
  Z = rig_candidate_poses(rig.cameras, rig.poses, tables[board])[0] if candidates is None else _f64(candidates).reshape(-1, 4, 4)
  centre = 0.5 * (tables[board].min(axis=0) + tables[board].max(axis=0))
  ia = members.index(a)
  if focus_distance is None:
    at = (rig.poses[ia][None] @ Z)[:, :3, :3] @ centre + (rig.poses[ia][None] @ Z)[:, :3, 3]
    focus_distance = float(np.median(np.linalg.norm(at, axis=1))) if len(Z) else np.inf
  focus = RigFocus(ia, list(range(len(members))), uncertainty.grid_of(cameras[a].image_size, focus_grid), focus_distance)
  views = [RigView(board, z, min_points) for z in Z]
  s = rig_view_information(rig.cameras, rig.poses, factors, tables, views, focus, n=n, criterion=criterion, sigma2=float(cov.sigma2),
                           margin=margin, min_cameras=min_cameras, with_A=False, boards_free=boards_free, workspace_mb=workspace_mb)
  picked = np.full((n, 4, 4), np.nan)
  in_camera = np.full((n, len(members), 4, 4), np.nan)
  n_cameras, n_visible = np.zeros(n, dtype=np.int64), np.zeros((n, len(members)), dtype=np.int64)
  for k in range(n):
    v = int(s.picks[k])
    if v >= 0:
      picked[k], in_camera[k] = Z[v], rig.poses @ Z[v][None]
      n_cameras[k], n_visible[k] = s.n_cameras[v], s.n_visible[v]
  loose = any(f[1] for f in factors)
  status = OK if (s.status == OK).any() else UNCONSTRAINED if loose else TOO_FEW
  return struct(cameras=np.array(members), reference=a, focus_distance=float(focus_distance), poses=picked,
                camera_poses_of_board=in_camera, candidate_index=s.picks.astype(np.int64), gain=s.pick_gain,
                focus_rms_before=s.focus_before, focus_rms_after=s.pick_focus_rms, n_cameras=n_cameras, n_visible=n_visible,
                status=status, candidates=Z, scores=s)


def last_rig_call_ms():
  """mcba_debug_rig_view_information_ms of this thread's last call: (dict(upload, kernel, download, call) in ms, slots launched)."""
  return _lib.call_ms("rig_view_information", ("upload", "kernel", "download", "call"))


def last_call_ms():
  """mcba_debug_view_information_ms of this thread's last call: (dict(upload, kernel, download, call) in ms, views launched)."""
  return _lib.call_ms("view_information", ("upload", "kernel", "download", "call"))
