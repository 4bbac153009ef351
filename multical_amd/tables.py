"""Initialisation tables of the pose graph (multical/tables.py:134-230,326-377) with the numeric core on the MI355X.

The reference builds the bundle adjustment's starting point from the per-view board poses [cameras, frames, boards]:
relative camera poses and relative board poses through a spanning tree of pairwise robust alignments
(`estimate_relative_poses`, tables.py:207-230) and one rig pose per frame (`relative_between_n`, tables.py:337-345).  Every
alignment is `matrix.align_transforms_robust` (transform/matrix.py:140-153): relative poses -> robust mean (Ward clustering
of the whitened rotation-vector | translation 6-vectors, transform/common.py:6-21) -> upper-quartile outlier test -> robust
mean.  Here all alignments of a stage run as ONE batch on the device (mcba_align_poses_robust: a workgroup per problem);
what stays on the host is the control logic on tiny arrays -- the overlap matrix, the greedy spanning tree
(graph.select_pairs, graph.py:7-33), chaining the pair transforms along the tree -- and 4x4 matrix products.

The pose table itself -- one board pose per (camera, frame, board) view, `make_pose_table` (tables.py:44-66) -- is estimated on
the device as well: mcba_view_poses runs board.estimate_pose_points (undistort + solvePnP) for every view in one launch.

Tables are `structs.Table`s with `poses [..., 4, 4]`, `valid [...]` (+ `num_points` for the pose table), like the
reference's.  `make_point_table` (tables.py:68-81) is data marshalling of ragged detections and stays in numpy.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, dp, f64 as _f64, ip, up
from .structs import Table, struct


def align_transforms_robust_ragged(A, B, sizes, mask=None, threshold=1.5, invert=False):
  """The device call on an already concatenated batch: A, B [total, 4, 4], sizes [P] entries per problem (in order), mask
  [total] or None.  Returns (transforms [P,4,4], valid [P] bool, inlier flags [total] bool)."""
  lib = _lib.load()
  sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
  P = int(sizes.size)
  if P == 0:
    return np.zeros((0, 4, 4)), np.zeros(0, dtype=bool), np.zeros(0, dtype=bool)
  offsets = np.ascontiguousarray(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
  total = int(offsets[-1])
  A = _f64(A).reshape(-1, 4, 4) if total else np.zeros((1, 4, 4))
  B = _f64(B).reshape(-1, 4, 4) if total else np.zeros((1, 4, 4))
  assert A.shape[0] == max(total, 1) and B.shape[0] == max(total, 1)
  if mask is not None:
    mask = np.ascontiguousarray(np.asarray(mask).astype(np.uint8).reshape(-1)) if total else np.zeros(1, dtype=np.uint8)
  out = np.empty((P, 4, 4))
  valid = np.empty(P, dtype=np.uint8)
  inl = np.empty(max(total, 1), dtype=np.uint8)
  import os, time
  t0 = time.perf_counter()
  check(lib.mcba_align_poses_robust(P, offsets.ctypes.data_as(C.POINTER(C.c_int64)), dp(A), dp(B), up(mask), float(threshold),
                                    1 if invert else 0, dp(out), up(valid), up(inl)))
  if os.environ.get("MCBA_TIMING"):
    print(f"[mcba_align_poses_robust] {P} problems, {total} entries, largest {int(sizes.max())}: {(time.perf_counter() - t0) * 1e3:.2f} ms",
          flush=True)
  return out, valid.astype(bool), inl[:total].astype(bool)


def align_transforms_robust_indexed(table, index_a, index_b, sizes, mask=None, threshold=1.5, invert=False):
  """The same device batch with the pairs given as indices into ONE pose table [N, 4, 4] (mcba_align_poses_indexed): entry k is
  the pair (table[index_a[k]], table[index_b[k]]).  Returns (transforms [P,4,4], valid [P] bool, inlier flags [total] bool)."""
  lib = _lib.load()
  sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
  P = int(sizes.size)
  if P == 0:
    return np.zeros((0, 4, 4)), np.zeros(0, dtype=bool), np.zeros(0, dtype=bool)
  offsets = np.ascontiguousarray(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
  total = int(offsets[-1])
  table = _f64(table).reshape(-1, 4, 4)
  ia = np.ascontiguousarray(np.asarray(index_a).reshape(-1), dtype=np.int32) if total else np.zeros(1, dtype=np.int32)
  ib = np.ascontiguousarray(np.asarray(index_b).reshape(-1), dtype=np.int32) if total else np.zeros(1, dtype=np.int32)
  assert ia.size == max(total, 1) and ib.size == max(total, 1) and table.shape[0] > 0
  if mask is not None:
    mask = np.ascontiguousarray(np.asarray(mask).astype(np.uint8).reshape(-1)) if total else np.zeros(1, dtype=np.uint8)
  out = np.empty((P, 4, 4))
  valid = np.empty(P, dtype=np.uint8)
  inl = np.empty(max(total, 1), dtype=np.uint8)
  tp = dp(table)
  check(lib.mcba_align_poses_indexed(P, offsets.ctypes.data_as(C.POINTER(C.c_int64)), tp, table.shape[0], ip(ia), tp,
                                     table.shape[0], ip(ib), up(mask), float(threshold), 1 if invert else 0, dp(out), up(valid), up(inl)))
  return out, valid.astype(bool), inl[:total].astype(bool)


def align_transforms_robust_batch(problems, threshold=1.5, invert=False):
  """problems: list of (m1 [n,4,4], m2 [n,4,4], mask [n] bool or None).  Returns (transforms [P,4,4], valid [P] bool,
  list of inlier masks) -- per problem exactly matrix.align_transforms_robust(m1, m2, valid=mask, threshold)
  (invert=True: tables.relative_between_inv: inputs and result inverted)."""
  P = len(problems)
  if P == 0:
    return np.zeros((0, 4, 4)), np.zeros(0, dtype=bool), []
  sizes = [int(np.asarray(p[0]).shape[0]) for p in problems]
  total = sum(sizes)
  A = np.concatenate([np.asarray(p[0], dtype=np.float64).reshape(-1, 4, 4) for p in problems]) if total else np.zeros((0, 4, 4))
  B = np.concatenate([np.asarray(p[1], dtype=np.float64).reshape(-1, 4, 4) for p in problems]) if total else np.zeros((0, 4, 4))
  mask = None
  if any(p[2] is not None for p in problems):
    mask = np.concatenate([np.ones(n, dtype=np.uint8) if p[2] is None else np.asarray(p[2]).astype(np.uint8)
                           for p, n in zip(problems, sizes)]) if total else np.zeros(0, dtype=np.uint8)
  out, valid, inl = align_transforms_robust_ragged(A, B, sizes, mask, threshold, invert)
  offsets = np.concatenate([[0], np.cumsum(sizes)])
  return out, valid, [inl[offsets[i]:offsets[i + 1]] for i in range(P)]


# ---- host control logic on [n, n] matrices (tables.py:134-148, graph.py:7-33) -------------------------------------------
def pattern_overlaps(table, axis=0):
  """tables.py:134-148: overlaps[i, j] = sum over the entries both i and j see of min(num_points).  The reference sums
  `has_pose.astype(float32) * weight` per pair; the terms are integers, so the float32 sum is EXACT (independent of its order)
  while it stays below 2^24 -- then one row of min() per index replaces the n (n - 1) / 2 np.take pairs (6 ms at 16 cameras x 1000
  frames x 5 boards); larger sums keep the reference's expression."""
  n = table.valid.shape[axis]
  V = np.moveaxis(np.asarray(table.valid), axis, 0).reshape(n, -1)
  W = np.moveaxis(np.asarray(table.num_points), axis, 0).reshape(n, -1)
  Wv = np.where(V, W, 0).astype(np.int64)          # min(w_i, w_j) over the common entries = min of the masked weights
  overlaps = np.zeros([n, n])
  if n > 0 and int(Wv.sum(axis=1).max(initial=0)) < (1 << 24):
    for i in range(n):
      overlaps[i] = np.minimum(Wv[i][None], Wv).sum(axis=1)
    np.fill_diagonal(overlaps, 0.0)
    return overlaps
  for i in range(n):
    for j in range(i + 1, n):
      has_pose = V[i] & V[j]
      weight = np.minimum(W[i], W[j])
      overlaps[i, j] = overlaps[j, i] = np.sum(has_pose.astype(np.float32) * weight)
  return overlaps


def select_pairs(overlaps, hop_penalty=0.8):
  overlaps = overlaps.copy()
  n = overlaps.shape[0]
  master = int(np.argmax(overlaps.sum(1)))
  weight = (np.arange(n) == master).astype(np.float32).reshape(n, 1)
  overlaps[:, master] = 0
  pairs = []
  while len(pairs) + 1 < n:
    w = overlaps * weight
    parent, child = np.unravel_index(np.argmax(w), w.shape)
    if w[parent, child] <= 0:
      break
    overlaps[:, child] = 0
    weight[child] = weight[parent] * hop_penalty
    pairs.append((int(parent), int(child)))
  return master, pairs


def inverse_poses(m):
  """(R | t) -> (R^T | -R^T t): the closed form agrees with the reference's np.linalg.inv (tables.py:229-230 use) to the last
  bits (1e-16) and costs a tenth of it."""
  m = np.asarray(m, dtype=np.float64)
  out = np.zeros(m.shape)
  out[..., :3, :3] = np.swapaxes(m[..., :3, :3], -1, -2)
  t = m[..., :3, 3]
  out[..., :3, 3] = -((m[..., 0, :3] * t[..., 0:1] + m[..., 1, :3] * t[..., 1:2]) + m[..., 2, :3] * t[..., 2:3])
  out[..., 3, 3] = 1.0
  return out


def inverse(table):
  """tables.inverse (tables.py:229-230 use)."""
  return table._extend(poses=inverse_poses(table.poses))


def estimate_relative_poses(table, axis=0, hop_penalty=0.9, of_inverse=False):
  """tables.py:207-227: all pair alignments of the spanning tree in one device batch.
  of_inverse: the result for `inverse(table)` without forming that table -- the device inverts the gathered entries as it loads
  them (`invert`: relative_between_inv semantics, inputs AND result inverted) and the handful of results is inverted back here
  (the closed-form inverse of all 80 000 poses of a 16 x 1000 x 5 table was a third of the host time of an initialisation)."""
  n = table.valid.shape[axis]
  master, pairs = select_pairs(pattern_overlaps(table, axis=axis), hop_penalty)
  if pairs:
    # the pose table goes to the device as it is and the batch [pairs x entries] as two lists of indices into it (per-pair np.take
    # + a concatenation of the problems were three host copies of every side, 10 ms at 15 pairs x 5 000 entries, and 19 MB of
    # upload where the table has 10)
    shape3 = np.asarray(table.valid).shape
    idx = np.moveaxis(np.arange(int(np.prod(shape3)), dtype=np.int32).reshape(shape3), axis, 0).reshape(n, -1)
    V = np.moveaxis(np.asarray(table.valid), axis, 0).reshape(n, -1)
    par = np.fromiter((p for p, _ in pairs), dtype=np.intp, count=len(pairs))
    chi = np.fromiter((c for _, c in pairs), dtype=np.intp, count=len(pairs))
    ts, ok, _ = align_transforms_robust_indexed(table.poses, idx[par], idx[chi], np.full(len(pairs), V.shape[1], dtype=np.int64),
                                                (V[par] & V[chi]).reshape(-1), invert=of_inverse)
    if of_inverse:
      ts = inverse_poses(ts)
  else:
    ts, ok = np.zeros((0, 4, 4)), np.zeros(0, dtype=bool)
  pose_dict = {master: np.eye(4)}
  for (parent, child), t, good in zip(pairs, ts, ok):
    if not good:
      # no common entry, or none that passes the upper-quartile test of the first pass: the reference's
      # align_transforms_robust takes the mean of an empty set there (transform/matrix.py:140-153) and fails; the device
      # reports the case instead of a pose (an identity transform must never be chained into the spanning tree)
      raise ValueError(f"estimate_relative_poses (axis={axis}): no usable common poses for pair ({parent}, {child})")
    pose_dict[child] = t @ pose_dict[parent]
  poses = np.broadcast_to(np.eye(4), (n, 4, 4)).copy()
  valid = np.zeros(n, dtype=bool)
  for k in sorted(pose_dict):
    poses[k] = pose_dict[k]
    valid[k] = True
  return Table.create(poses=poses @ np.linalg.inv(poses[0]), valid=valid)


def estimate_relative_poses_inv(table, axis=2, hop_penalty=0.9):
  """tables.py:229-230."""
  return inverse(estimate_relative_poses(table, axis=axis, hop_penalty=hop_penalty, of_inverse=True))


def relative_between_n(table1, table2, axis=0, inv=False):
  """tables.py:337-345: one alignment per index of `axis`, restricted to the entries valid in both tables -- a ragged
  batch of small problems (at most cameras x boards entries each) on the device.  The batch is cut out of the tables with ONE
  boolean selection (the per-index `np.take` of the first version cost 0.7 s for the 1000 frames of a 16 x 1000 x 5 table --
  more than the device work of the whole initialisation)."""
  n = table1.valid.shape[axis]
  v = np.moveaxis(np.asarray(table1.valid) & np.asarray(table2.valid), axis, 0).reshape(n, -1)      # [n, entries]
  p1 = np.moveaxis(np.asarray(table1.poses), axis, 0).reshape(n, -1, 4, 4)
  p2 = np.moveaxis(np.asarray(table2.poses), axis, 0).reshape(n, -1, 4, 4)
  poses, valid, _ = align_transforms_robust_ragged(p1[v], p2[v], v.sum(axis=1), None, invert=inv)   # (k, entry) order
  return Table.create(poses=poses, valid=valid)


def initialise_poses(pose_table, camera_poses=None):
  """tables.py:353-377: camera / board / rig-pose tables from the per-view board poses [C, F, B]."""
  if camera_poses is not None:
    # (given poses replace the estimate, tables.py:357-361; the estimate is not formed first: cameras that share no view -- the
    # rigs that NEED given poses -- have no spanning tree to estimate from)
    camera = Table.create(poses=np.asarray(camera_poses, dtype=np.float64), valid=np.ones(len(camera_poses), dtype=bool))
  else:
    camera = estimate_relative_poses(pose_table, axis=0)
  board = estimate_relative_poses_inv(pose_table, axis=2)
  binv = inverse(board)
  # cam @ rig @ board = pose  ->  cam @ rig = board_relative = pose @ board^-1, then one alignment per frame between the camera
  # poses (expanded over frames and boards, tables.py:366-372) and board_relative over the entries valid in both:
  # `relative_between_n(expanded, board_relative, axis=1, inv=True)`.  Only those entries are ever read, so only they are formed
  # (the two full [C, F, B, 4, 4] tables, the broadcast copy and two boolean selections were 14 ms of host time at 16 x 1000 x 5,
  # where 15 455 of the 80 000 entries take part), in the order the reference's selection gives them: (frame | camera, board).
  poses = np.asarray(pose_table.poses, dtype=np.float64)
  C_, F, B = poses.shape[:3]
  v = (np.asarray(pose_table.valid) & binv.valid[None, None] & np.asarray(camera.valid)[:, None, None])
  vf = np.moveaxis(v, 1, 0).reshape(F, C_ * B)
  f_idx, e_idx = np.nonzero(vf)
  c_idx, b_idx = e_idx // B, e_idx % B
  p1 = np.asarray(camera.poses, dtype=np.float64)[c_idx]
  p2 = poses[c_idx, f_idx, b_idx] @ binv.poses[b_idx]
  rig, rig_valid, _ = align_transforms_robust_ragged(p1, p2, vf.sum(axis=1), None, invert=True)
  times = Table.create(poses=rig, valid=rig_valid)
  return struct(times=times, camera=camera, board=board)


# ---- robot-world hand-eye solves A_i X = Z B_i (hand_eye/hand_eye.py:82-121, transform/hand_eye.py:20-50) ------------------
HANDEYE_OK, HANDEYE_TOO_FEW, HANDEYE_DEGENERATE = 0, 1, 2   # mcba.h: MCBA_HANDEYE_*


class HandEyeInputs(object):
  """The arrays of one mcba_hand_eye_problem, kept alive next to the ctypes struct that points into them."""

  def __init__(self, table_a, valid_a, table_b, valid_b, index_a, index_b, invert=False):
    same = table_a is table_b and valid_a is valid_b
    self.table_a = _f64(table_a)
    self.valid_a = np.ascontiguousarray(np.asarray(valid_a).astype(np.uint8))
    self.table_b = self.table_a if same else _f64(table_b)
    self.valid_b = self.valid_a if same else np.ascontiguousarray(np.asarray(valid_b).astype(np.uint8))
    assert self.table_a.ndim == 4 and self.table_a.shape[2:] == (4, 4) and self.valid_a.shape == self.table_a.shape[:2]
    assert self.table_b.ndim == 4 and self.table_b.shape[2:] == (4, 4) and self.valid_b.shape == self.table_b.shape[:2]
    assert self.table_a.shape[1] == self.table_b.shape[1], "both tables hold one pose per frame"
    self.index_a = np.ascontiguousarray(np.asarray(index_a, dtype=np.int32).reshape(-1))
    self.index_b = np.ascontiguousarray(np.asarray(index_b, dtype=np.int32).reshape(-1))
    assert self.index_a.shape == self.index_b.shape
    self.n, self.F = int(self.index_a.size), int(self.table_a.shape[1])
    self.invert = bool(invert)

  def struct(self):
    s = _lib.HandEyeProblem()
    s.F, s.n_a, s.n_b = self.F, self.table_a.shape[0], self.table_b.shape[0]
    s.table_a, s.valid_a = dp(self.table_a), up(self.valid_a)
    s.table_b, s.valid_b = dp(self.table_b), up(self.valid_b)
    s.n_problems = self.n
    s.index_a, s.index_b = ip(self.index_a), ip(self.index_b)
    s.invert_inputs = 1 if self.invert else 0
    return s

  def outputs(self):
    return (np.empty((self.n, 4, 4)), np.empty((self.n, 4, 4)), np.empty(self.n, dtype=np.int32), np.empty(self.n, dtype=np.uint8),
            np.empty((self.n, self.F)))


def hand_eye_batch(table_a, valid_a, table_b, valid_b, index_a, index_b, invert=False):
  """mcba_hand_eye: problem p solves A_i X = Z B_i over the frames valid in row index_a[p] of table_a [n_a, F, 4, 4] and row
  index_b[p] of table_b [n_b, F, 4, 4] (pass the same objects for both sides and the table is uploaded once).  invert: every
  pose is inverted on the device first.  Returns X [n, 4, 4], Z [n, 4, 4], n_pairs [n], status [n] (HANDEYE_*), err [n, F]."""
  inp = HandEyeInputs(table_a, valid_a, table_b, valid_b, index_a, index_b, invert)
  X, Z, n_pairs, status, err = inp.outputs()
  s = inp.struct()
  check(_lib.load().mcba_hand_eye(C.byref(s), dp(X), dp(Z), ip(n_pairs), up(status), dp(err)))
  return X, Z, n_pairs, status, err


def make_point_table(detections, boards):
  """tables.py:68-81: ragged per-image detections (corners [k, 2], ids [k]) -> dense table [C, F, B, P] (+ mask).

  dtype: the reference fills one array per image with `values.dtype` (fill_sparse, tables.py:15-21) and stacks them
  (make_nd_table -> Table.stack -> np.stack), so the table carries numpy's PROMOTION of all per-image corner dtypes: float32
  when every detection is float32 (cv2.aruco), float64 as soon as one image contributes float64 corners -- e.g. an empty
  detection built as np.zeros([0, 2]).  One scatter for the whole table instead of one per image."""
  num_points = int(np.max([b.num_points for b in boards]))
  C_, F, B = len(detections), len(detections[0]), len(detections[0][0])
  flat = [detections[c][f][b] for c in range(C_) for f in range(F) for b in range(B)]
  corners = [np.asarray(d.corners) for d in flat]
  ids = [np.asarray(d.ids, dtype=np.int64).reshape(-1) for d in flat]
  dtype = np.result_type(*[a.dtype for a in corners])
  counts = np.array([i.size for i in ids], dtype=np.int64)
  points = np.zeros((C_ * F * B, num_points, 2), dtype=dtype)
  valid = np.zeros((C_ * F * B, num_points), dtype=bool)
  if counts.sum() > 0:
    image = np.repeat(np.arange(C_ * F * B), counts)
    point = np.concatenate(ids)
    points[image, point] = np.concatenate([a.reshape(-1, 2) for a, i in zip(corners, ids) if i.size]).astype(dtype, copy=False)
    valid[image, point] = True
  return Table.create(points=points.reshape(C_, F, B, num_points, 2), valid=valid.reshape(C_, F, B, num_points))


def refine_point_table(images, point_table, drop=(), **kw):
  """Refine every valid corner of a point table (points [C, F, B, P, 2], valid [C, F, B, P]) to sub-pixel in the images it was found
  in: images[c] is the [F, H, W] grey stack of camera c.  One subpix.refine_corners call per distinct image size (the cameras of one
  size go together); kw: its window, zero_zone, max_iter, eps.  Returns (table, status [C, F, B, P] uint8) with the dtype of the
  table kept, invalid slots untouched and their status subpix.INVALID.  drop: names of statuses ("singular", "reverted",
  "left_image", ...) whose slots lose `valid`; by default nothing is dropped."""
  from . import subpix
  points, valid = np.array(point_table.points), np.array(point_table.valid, dtype=bool)
  C_, F = valid.shape[:2]
  stacks = [np.asarray(s) for s in images]
  assert len(stacks) == C_ and all(s.ndim == 3 and s.shape[0] == F for s in stacks), "images[c] is the [F, H, W] stack of camera c"
  status = np.full(valid.shape, subpix.INVALID, dtype=np.uint8)
  for size in sorted({s.shape[1:] + (s.dtype.str,) for s in stacks}):
    cams = [c for c in range(C_) if stacks[c].shape[1:] + (stacks[c].dtype.str,) == size]
    c, f, b, p = np.nonzero(valid[cams])
    if c.size == 0:
      continue
    c = np.array(cams)[c]
    batch = np.concatenate([stacks[k] for k in cams])
    image_of = (np.searchsorted(cams, c) * F + f).astype(np.int32)
    refined, st = subpix.refine_corners(batch, points[c, f, b, p].astype(np.float64), image_of, **kw)[:2]
    points[c, f, b, p] = refined.astype(points.dtype)
    status[c, f, b, p] = st
  dropped = np.isin(status, [subpix.STATUS_NAMES[name] for name in drop]) & valid
  return point_table._extend(points=points, valid=valid & ~dropped), status


# ---- the pose table: one board pose per view from its detections (tables.py:38-66, board/common.py:30-47) -----------------
VIEW_OK, VIEW_TOO_FEW, VIEW_MASKED, VIEW_DEGENERATE, VIEW_NOT_CONVERGED = 0, 1, 2, 3, 4   # mcba.h: MCBA_VIEW_*


def _is_fisheye(camera):
  return type(camera).__name__ == "CameraFisheye" or getattr(camera, "model", None) == "fisheye"


class ViewPoseInputs(object):
  """The arrays of one mcba_view_pose_problem, kept alive next to the ctypes struct that points into them."""

  def __init__(self, points, valid, board_points, cameras, view_mask=None, init_poses=None, max_iterations=0, board_sizes=None):
    self.points = _f64(points)
    self.valid = np.ascontiguousarray(np.asarray(valid).astype(np.uint8))
    self.shape = self.valid.shape[:3]
    C_, F, B = self.shape
    P = self.valid.shape[3]
    assert self.points.shape == (C_, F, B, P, 2) and len(cameras) == C_ and len(board_points) == B
    self.board_sizes = np.ascontiguousarray(np.array([len(b) for b in board_points] if board_sizes is None else board_sizes,
                                                     dtype=np.int32))
    self.board_points = np.zeros((B, P, 3))
    for b, pts in enumerate(board_points):
      self.board_points[b, :len(pts)] = np.asarray(pts, dtype=np.float64)
    # camera blocks [fx fy cx cy skew dist...]: the INTRINSIC MATRIX as it is -- estimate_pose_points hands cv2 camera.intrinsic,
    # not the fix_aspect parameterisation of the bundle adjustment (board/common.py:42)
    nds = [int(np.asarray(c.dist).size) for c in cameras]
    self.n_dist = max(nds + [4])
    self.cameras = np.zeros((C_, 5 + self.n_dist))
    for i, c in enumerate(cameras):
      K = np.asarray(c.intrinsic, dtype=np.float64)
      self.cameras[i, :5] = [K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 1]]
      self.cameras[i, 5:5 + nds[i]] = np.asarray(c.dist, dtype=np.float64).ravel()
    self.camera_n_dist = np.ascontiguousarray(np.array(nds, dtype=np.int32))
    self.is_fisheye = np.ascontiguousarray(np.array([_is_fisheye(c) for c in cameras], dtype=np.uint8))
    self.view_mask = None if view_mask is None else np.ascontiguousarray(np.asarray(view_mask).astype(np.uint8))
    self.init_poses = None if init_poses is None else _f64(init_poses)
    assert self.view_mask is None or self.view_mask.shape == self.shape
    assert self.init_poses is None or self.init_poses.shape == self.shape + (4, 4)
    self.max_iterations = int(max_iterations)
    self.lm_iterations = np.zeros(self.shape, dtype=np.int32)

  def struct(self):
    s = _lib.ViewPoseProblem()
    s.C, s.F, s.B = self.shape
    s.P = self.valid.shape[3]
    s.points, s.valid = dp(self.points), up(self.valid)
    s.board_points, s.board_sizes = dp(self.board_points), ip(self.board_sizes)
    s.cameras, s.n_dist = dp(self.cameras), self.n_dist
    s.camera_n_dist, s.is_fisheye = ip(self.camera_n_dist), up(self.is_fisheye)
    s.fix_aspect = None
    s.view_mask = up(self.view_mask)
    s.init_poses = dp(self.init_poses)
    s.max_iterations = self.max_iterations
    s.lm_iterations = ip(self.lm_iterations)
    return s

  def outputs(self):
    return (np.empty(self.shape + (4, 4)), np.empty(self.shape), np.empty(self.shape, dtype=np.int32),
            np.empty(self.shape, dtype=np.uint8))


def view_poses(points, valid, board_points, cameras, view_mask=None, init_poses=None, max_iterations=0):
  """mcba_view_poses: (poses [C,F,B,4,4], sse [C,F,B], n_used, status, lm_iterations) of every view of the detection table;
  board_points: one [P_b, 3] array per board.  Views that are masked out or hold fewer than 4 corners are not launched."""
  inp = ViewPoseInputs(points, valid, board_points, cameras, view_mask, init_poses, max_iterations)
  poses, sse, n_used, status = inp.outputs()
  s = inp.struct()
  check(_lib.load().mcba_view_poses(C.byref(s), dp(poses), dp(sse), ip(n_used), up(status)))
  return poses, sse, n_used, status, inp.lm_iterations


def min_detections_mask(valid, boards):
  """board.has_min_detections of every view [C, F, B] (has_min_detections_grid, board/common.py:30-34), vectorised: integer work on
  the ids.  The ids of a view are the indices of its valid corners (tables.sparse_points); they are unravelled over (h, w) of the
  board's `size` -- as the reference does, also for a charuco board whose corners form an (h-1) x (w-1) grid -- and an AprilGrid
  tests the TAG ids `ids // 4` (board/aprilgrid.py:197-199) while its count stays the number of corners.  `size`, `min_rows`,
  `min_points` are read from the board objects by duck typing; a board without them (a bare point set) passes every view."""
  valid = np.asarray(valid).astype(bool)
  C_, F, B, P = valid.shape
  mask = np.ones((C_, F, B), dtype=bool)
  for b, board in enumerate(boards):
    size, min_rows, min_points = (getattr(board, k, None) for k in ("size", "min_rows", "min_points"))
    if size is None or min_rows is None or min_points is None:
      continue
    w, h = int(size[0]), int(size[1])
    n = min(P, int(board.num_points)) if hasattr(board, "num_points") else P
    ids = np.arange(n)
    if type(board).__name__ == "AprilGrid" or hasattr(board, "tag_length"):
      ids = ids // 4
    if n > 0 and int(ids.max()) >= h * w:
      raise ValueError(f"board {b}: ids beyond its {h} x {w} grid")     # (np.unravel_index raises in the reference)
    v = valid[:, :, b, :n].reshape(-1, n).astype(np.float32)
    rows = (v @ (ids[:, None] // w == np.arange(h)[None]).astype(np.float32) > 0).sum(axis=1)
    cols = (v @ (ids[:, None] % w == np.arange(w)[None]).astype(np.float32) > 0).sum(axis=1)
    count = valid[:, :, b, :n].reshape(-1, n).sum(axis=1)
    mask[:, :, b] = ((count >= min_points) & (rows >= min_rows) & (cols >= min_rows)).reshape(C_, F)
  return mask


def make_pose_table(point_table, boards, cameras, exclude_bad_poses=True, pose_error_limit=1.0, error_norm='point',
                    return_info=False):
  """tables.make_pose_table (tables.py:44-66): the board pose of every (camera, frame, board) view from its detections, all views in
  ONE device call (mcba_view_poses) instead of one cv2.solvePnPGeneric per view.  Returns the reference's table -- poses [C,F,B,4,4],
  valid, num_points, reprojection_error, view_angles [C,F,B,3] -- whose invalid entries are tables.invalid_pose (identity, 0, 0,
  [0, 0, 0]); it feeds `initialise_poses` unchanged.

  A view is estimated when it passes board.has_min_detections (`min_detections_mask`) and holds 4 corners.  It is valid when the
  estimate converged (status 0) and -- with exclude_bad_poses -- its reprojection_error does not exceed pose_error_limit.

  error_norm: 'point' -> sqrt(sse / n), the RMS distance per corner (the convention synthetic.view_pose_errors states);
  'coordinate' -> sqrt(sse / 2n), the RMS per coordinate.  OpenCV's solvePnPGeneric is believed to report the latter
  (norm / sqrt(2 N)); that could not be checked -- no cv2 on the machines this was built on -- so the default stays with the
  project's own convention and the choice is the caller's.  The two differ by exactly sqrt(2).

  Deviations from the reference's numbers, by construction: the undistortion is the exact inverse of the projection,
  not cv2's five fixed-point sweeps; points stay float64; the refinement is iterated to the optimum, not to cv2's stop.

  return_info: also return struct(status, sse, num_used, error, lm_iterations, view_mask) over [C,F,B] (error: before invalid
  entries are zeroed)."""
  if error_norm not in ('point', 'coordinate'):
    raise ValueError(f"error_norm {error_norm!r}: 'point' or 'coordinate'")
  valid_pts = np.asarray(point_table.valid).astype(bool)
  view_mask = min_detections_mask(valid_pts, boards)
  poses, sse, n_used, status, iters = view_poses(point_table.points, valid_pts, [np.asarray(b.points) for b in boards], cameras,
                                                 view_mask=view_mask)
  per = 1.0 if error_norm == 'point' else 2.0
  error = np.sqrt(sse / (per * np.maximum(n_used, 1)))
  valid = status == VIEW_OK
  if exclude_bad_poses:
    valid = valid & (error <= pose_error_limit)
  from scipy.spatial.transform import Rotation
  angles = np.zeros(valid.shape + (3,))
  if valid.any():
    angles[valid] = Rotation.from_matrix(poses[valid][:, :3, :3]).as_euler('xyz', degrees=True)   # transform/rtvec.py:55-58
  table = Table.create(poses=np.where(valid[..., None, None], poses, np.eye(4)), valid=valid,
                       num_points=np.where(valid, valid_pts.sum(axis=3), 0),
                       reprojection_error=np.where(valid, error, 0.0), view_angles=angles)
  if return_info:
    return table, struct(status=status, sse=sse, num_used=n_used, error=error, lm_iterations=iters, view_mask=view_mask)
  return table


# ---- intrinsic calibration: every camera from its own detections (camera.py:69-105, camera_fisheye.py:71-94) ---------------
CAMERA_OK, CAMERA_TOO_FEW_VIEWS, CAMERA_DEGENERATE, CAMERA_NOT_CONVERGED, CAMERA_MASKED = 0, 1, 2, 3, 4   # mcba.h: MCBA_CAMERA_*

# model -> (distortion coefficients, fisheye, coefficients estimated by default).  The masks restate OpenCV's flag semantics FROM
# KNOWLEDGE OF OPENCV, unverifiable without a cv2 binary: without CALIB_RATIONAL_MODEL k4 k5 k6 stay 0, CALIB_THIN_PRISM_MODEL adds
# s1..s4 and CALIB_TILTED_MODEL adds tau_x tau_y, each on top of k1 k2 p1 p2 k3 only.
INTRINSIC_MODELS = dict(
  standard=(5, False, [1] * 5),
  rational=(8, False, [1] * 8),
  thin_prism=(12, False, [1] * 5 + [0] * 3 + [1] * 4),
  tilted=(14, False, [1] * 5 + [0] * 7 + [1] * 2),
  pin4=(4, False, [1] * 4),
  fisheye=(4, True, [1] * 4),
)


def _per_camera(value, n):
  return list(value) if isinstance(value, (list, tuple, np.ndarray)) else [value] * n


class IntrinsicInputs(object):
  """The arrays of one mcba_intrinsic_problem, kept alive next to the ctypes struct that points into them."""

  def __init__(self, points, valid, board_points, image_sizes, model='standard', fix_aspect=False, view_mask=None, init=None,
               free_dist=None, max_iterations=0):
    self.points = _f64(points)
    self.valid = np.ascontiguousarray(np.asarray(valid).astype(np.uint8))
    self.shape = self.valid.shape[:3]
    C_, F, B = self.shape
    P = self.valid.shape[3]
    assert self.points.shape == (C_, F, B, P, 2) and len(board_points) == B and len(image_sizes) == C_
    self.board_sizes = np.ascontiguousarray(np.array([len(b) for b in board_points], dtype=np.int32))
    self.board_points = np.zeros((B, P, 3))
    for b, pts in enumerate(board_points):
      self.board_points[b, :len(pts)] = np.asarray(pts, dtype=np.float64)
    self.image_sizes = _f64(np.asarray(image_sizes, dtype=np.float64).reshape(C_, 2))
    self.models = _per_camera(model, C_)
    for m in self.models:
      if m not in INTRINSIC_MODELS:
        raise ValueError(f"camera model {m!r}: one of {sorted(INTRINSIC_MODELS)}")
    nds = [INTRINSIC_MODELS[m][0] for m in self.models]
    self.n_dist = max(nds)
    self.camera_n_dist = np.ascontiguousarray(np.array(nds, dtype=np.int32))
    self.is_fisheye = np.ascontiguousarray(np.array([INTRINSIC_MODELS[m][1] for m in self.models], dtype=np.uint8))
    self.fix_aspect = np.ascontiguousarray(np.array(_per_camera(fix_aspect, C_), dtype=np.uint8))
    self.free_dist = np.zeros((C_, self.n_dist), dtype=np.uint8)
    for c, m in enumerate(self.models):
      self.free_dist[c, :nds[c]] = INTRINSIC_MODELS[m][2]
    if free_dist is not None:
      fd = np.asarray(free_dist).astype(np.uint8)
      fd = np.broadcast_to(fd, (C_,) + fd.shape[-1:])
      self.free_dist[:, :fd.shape[1]] = fd[:, :self.n_dist]
      for c in range(C_):
        self.free_dist[c, nds[c]:] = 0
    self.view_mask = None if view_mask is None else np.ascontiguousarray(np.asarray(view_mask).astype(np.uint8))
    assert self.view_mask is None or self.view_mask.shape == self.shape
    self.init_cameras = self.init_poses = None
    if init is not None:
      cams, poses = init
      self.init_cameras = np.zeros((C_, 5 + self.n_dist))
      cams = np.asarray(cams, dtype=np.float64)
      self.init_cameras[:, :cams.shape[1]] = cams[:, :5 + self.n_dist]
      self.init_poses = _f64(poses)
      assert self.init_poses.shape == self.shape + (4, 4)
    self.max_iterations = int(max_iterations)
    self.lm_iterations = np.zeros(C_, dtype=np.int32)

  def struct(self):
    s = _lib.IntrinsicProblem()
    s.C, s.F, s.B = self.shape
    s.P = self.valid.shape[3]
    s.points, s.valid = dp(self.points), up(self.valid)
    s.board_points, s.board_sizes = dp(self.board_points), ip(self.board_sizes)
    s.image_sizes, s.n_dist = dp(self.image_sizes), self.n_dist
    s.camera_n_dist, s.is_fisheye = ip(self.camera_n_dist), up(self.is_fisheye)
    s.fix_aspect, s.free_dist = up(self.fix_aspect), up(self.free_dist)
    s.view_mask = up(self.view_mask)
    s.init_cameras = dp(self.init_cameras)
    s.init_poses = dp(self.init_poses)
    s.max_iterations = self.max_iterations
    s.lm_iterations = ip(self.lm_iterations)
    return s

  def call(self, fn, *extra):
    """fn(struct, cameras, poses, sse, n_used, view_status, camera_status, *extra) -> rc; returns (rc, result struct)."""
    C_ = self.shape[0]
    cameras, poses, sse = np.zeros((C_, 5 + self.n_dist)), np.empty(self.shape + (4, 4)), np.empty(self.shape)
    n_used, vstat, cstat = np.empty(self.shape, dtype=np.int32), np.empty(self.shape, dtype=np.uint8), np.empty(C_, dtype=np.uint8)
    s = self.struct()
    rc = fn(C.byref(s), dp(cameras), dp(poses), dp(sse), ip(n_used), up(vstat), up(cstat), *extra)
    n_cam, sse_cam = n_used.reshape(C_, -1).sum(axis=1), sse.reshape(C_, -1).sum(axis=1)
    return rc, struct(cameras=cameras, camera_n_dist=self.camera_n_dist.copy(), poses=poses, sse=sse, n_used=n_used,
                      view_status=vstat, camera_status=cstat, lm_iterations=self.lm_iterations,
                      error=np.sqrt(sse_cam / np.maximum(n_cam, 1)), error_perview=np.sqrt(sse / np.maximum(n_used, 1)))


def calibrate_intrinsics(point_table, boards, image_sizes, model='standard', fix_aspect=False, view_mask=None, init=None,
                         free_dist=None, max_iterations=0):
  """mcba_calibrate_intrinsics: the intrinsics of every camera of a detection table from its own detections, all cameras in ONE
  device call -- what the reference gets from one cv2.calibrateCameraExtended / cv2.fisheye.calibrate per camera (camera.py:86-88,
  camera_fisheye.py:84-86).  A view is one (frame, board) slot.

  model: a name of INTRINSIC_MODELS or one per camera (a rig may mix them); fix_aspect: bool or one per camera; view_mask [C,F,B]:
  views to use (default: board.has_min_detections, `min_detections_mask`); init: (cameras [C, 5 + n_dist], poses [C,F,B,4,4]) warm
  start; free_dist [C, n_dist] or [n_dist]: coefficients to estimate (default: INTRINSIC_MODELS' mask), the others stay at their
  start value; max_iterations: Levenberg-Marquardt passes (0: 100).

  Returns struct(cameras [C, 5 + n_dist] blocks [fx fy cx cy skew dist...], camera_n_dist, poses [C,F,B,4,4], sse, n_used,
  view_status [C,F,B] (VIEW_*), camera_status [C] (CAMERA_*), lm_iterations [C], error [C] = sqrt(sum sse / sum n),
  error_perview [C,F,B] = sqrt(sse / n)).  The solution is the optimum of the reprojection cost, not cv2's (10, 1e-3) stop."""
  boards_pts = [np.asarray(getattr(b, "points", b)) for b in boards]
  valid = np.asarray(point_table.valid).astype(bool)
  if view_mask is None:
    view_mask = min_detections_mask(valid, boards)
  inp = IntrinsicInputs(point_table.points, valid, boards_pts, image_sizes, model, fix_aspect, view_mask, init, free_dist,
                        max_iterations)
  rc, out = inp.call(_lib.load().mcba_calibrate_intrinsics)
  check(rc)
  return out


# ---- stereo pairs (tables.py:111-128, 380-382) ---------------------------------------------------------------------------------
def matching_points(points, board, cam1, cam2):
  """tables.matching_points (tables.py:115-128): the corners cameras cam1 and cam2 both detected, view by view, as a struct of
  parallel lists points1, points2, object_points, ids.  points: a point table [C, F, P] of one board (the reference's form: one
  entry per frame, empty ones included) or [C, F, B, P] with `board` a list of boards (one entry per (frame, board) slot, frame-major).
  Boards are objects with `points`, or [P_b, 3] arrays."""
  pts, valid = np.asarray(points.points, dtype=np.float64), np.asarray(points.valid).astype(bool)
  if valid.ndim == 3:
    pts, valid, board = pts[:, :, None], valid[:, :, None], [board]
  elif not isinstance(board, (list, tuple)):
    board = [board]
  assert valid.ndim == 4 and len(board) == valid.shape[2], "one board per slot of the table's board axis"
  board_points = [np.asarray(getattr(b, "points", b), dtype=np.float64) for b in board]
  out = struct(points1=[], points2=[], object_points=[], ids=[])
  for f in range(valid.shape[1]):
    for b in range(valid.shape[2]):
      ids = np.flatnonzero(valid[cam1, f, b] & valid[cam2, f, b])
      out.points1.append(pts[cam1, f, b, ids])
      out.points2.append(pts[cam2, f, b, ids])
      out.object_points.append(board_points[b][ids])
      out.ids.append(ids)
  return out


def stereo_calibrate(points, board, cameras, i, j, **kwargs):
  """tables.stereo_calibrate (tables.py:380-382): camera.stereo_calibrate of cameras i and j on their matching points; a pair of
  fisheye cameras goes to camera.stereo_calibrate_fisheye."""
  from . import camera
  matching = matching_points(points, board, i, j)
  fn = camera.stereo_calibrate_fisheye if _is_fisheye(cameras[i]) and _is_fisheye(cameras[j]) else camera.stereo_calibrate
  return fn((cameras[i], cameras[j]), matching, **kwargs)
