"""TEST INFRASTRUCTURE: synthetic rigs whose per-view inlier counts sit on every edge of the 64-observation chunks the per-view
kernels walk (k_linearize, k_residual, k_cost, k_lsmr_jv / jtu / fused / fused2), for each of the 42 view shapes the kernels are
instantiated for: 7 camera units x 3 motion models x {intrinsics optimised, fixed}.

The rigs come from synthetic.make_rig unchanged; the helpers below only REMOVE observations (they clear `valid` and `points` of
the slots behind the first k valid ones of a view), so the generator, the oracle and the device see ordinary detections."""
import functools

import numpy as np

from multical_amd import synthetic

# camera translation unit of the kernels -> distortion model(s) of the generator (mix14: pinhole AND fisheye cameras in one rig;
# 4 coefficients each, so that every camera block has 9 entries and the reference's own sparsity_matrix accepts the rig)
UNITS = dict(pin4="pin4", pin5="standard", pin8="rational", pin12="thin_prism", pin14="tilted", fish4="fisheye",
             mix14=["pin4", "fisheye"])
MOTIONS = ["static", "rolling", "hand_eye"]
SHAPES = [(u, m, k) for u in UNITS for m in MOTIONS for k in (True, False)]

# inlier counts of a view: below / at / above one and two chunks, the last lane groups of a chunk, three and four chunks (one MFMA
# step of four chunks, the even rounding of the step count) and the first observation of a fifth
COUNTS = [1, 2, 4, 5, 8, 9, 60, 61, 63, 64, 65, 68, 127, 128, 129, 192, 256, 257]
SMALL_COUNTS = [k for k in COUNTS if k <= 68]
# frame counts tried in turn: the first at which every count fits on both cameras is taken (at seed 71 with today's generator that is
# 31 for all 42 shapes; 30, 32 and 34 .. 41 lack a view of 256 / 257 points on some shape), so a change of the generator moves the
# choice instead of breaking the placement
FRAME_CHOICES = range(31, 49)
SEGMENT = 512        # LIN_MAX_POINTS of the kernels: a larger board is walked in segments of this many slots
BIG_PAIRS = [(0, 1), (0, 64), (0, 65), (1, 0), (64, 0), (64, 64), (65, 63), (128, 1), (256, 65), (1, 1)]
BIG_SHAPES = [("pin5", "static", True), ("pin8", "rolling", True), ("fish4", "hand_eye", False)]
BIG_FRAME_CHOICES = range(16, 33)   # (16 works for the three shapes at seed 71)


def shape_id(shape):
  unit, motion, optk = shape
  return f"{unit}-{motion}-{'free' if optk else 'fixed'}"


def _keep_first(rig, view, k, lo=0, hi=None):
  """Keep the first k valid slots of view[lo:hi]; clear `valid` and `points` of the others in that range."""
  v = rig.valid[view][lo:hi]
  drop = np.flatnonzero(v)[k:]
  v[drop] = False
  rig.points[view][lo:hi][drop] = 0.0


def _make(unit, motion, optk, boards, frames, seed):
  cfg = dict(cameras=2, frames=frames, boards=boards, motion=motion, model=UNITS[unit], optimize_cameras=bool(optk),
             layout="stereo", seed=seed)
  rig = synthetic.make_rig(cfg, outlier_frac=0.0)
  rig.name = f"planted_{unit}_{motion}_{'free' if optk else 'fixed'}"
  return rig


def _freeze(rig):
  """the rigs are cached and shared by every test of a process: an accidental write is an error, not a dependency between tests"""
  rig.valid.flags.writeable = False
  rig.points.flags.writeable = False
  return rig


def _plant(rig):
  """Place COUNTS on both cameras of the rig (in place); None when a count finds no view or fewer than two views are empty."""
  C, F, B, P = rig.valid.shape
  planted = {k: [] for k in COUNTS}
  for c in range(C):
    n = rig.valid[c, :, 0].sum(axis=-1)
    free = set(range(F))
    for k in sorted(COUNTS, reverse=True):
      fits = [f for f in free if n[f] >= k]
      if not fits:
        return None
      f = min(fits, key=lambda f: (n[f], f))
      _keep_first(rig, (c, f, 0), k)
      planted[k].append((c, f))
      free.discard(f)
    for i, f in enumerate(sorted(f for f in free if n[f] >= 68)):
      k = SMALL_COUNTS[(i + 5 * c) % len(SMALL_COUNTS)]
      _keep_first(rig, (c, f, 0), k)
      planted[k].append((c, f))
  return planted if (rig.valid[:, :, 0].sum(axis=-1) == 0).sum() >= 2 else None


@functools.lru_cache(maxsize=None)
def planted_rig(unit, motion, optk, seed=71):
  """(rig, {count: [(camera, frame), ...]}): 2 cameras x (the first of FRAME_CHOICES that works) frames of one 324-point aprilgrid whose
  views hold exactly the COUNTS above -- every count on BOTH cameras (in the mixed rig the projection family goes with the camera).
  The largest count is placed first, on the free view with the fewest points that still has enough; every view left over with 68
  points or more is cut to one of the counts up to 68 (about 6000 residuals per rig); the views the generator left empty stay empty.
  The result is cached and its tables are read-only."""
  for frames in FRAME_CHOICES:
    rig = _make(unit, motion, optk, ["aprilgrid_9x9"], frames, seed)
    planted = _plant(rig)
    if planted is not None:
      break
  assert planted is not None, f"{rig.name}: no frame count of {FRAME_CHOICES} places every count on both cameras next to two empty views"
  C = rig.valid.shape[0]
  counts = rig.valid[:, :, 0].sum(axis=-1)
  for k, views in planted.items():
    assert {c for c, _ in views} == set(range(C)), (rig.name, k)
    assert all(counts[v] == k for v in views)
  assert (counts == 0).sum() >= 2, rig.name
  return _freeze(rig), planted


def _plant_big(rig):
  """Place BIG_PAIRS on the views of board 0 (in place); None when a pair finds no view."""
  C, F, B, P = rig.valid.shape
  assert P > SEGMENT
  n0 = rig.valid[:, :, 0, :SEGMENT].sum(axis=-1)
  n1 = rig.valid[:, :, 0, SEGMENT:].sum(axis=-1)
  free = {(c, f) for c in range(C) for f in range(F) if n0[c, f] + n1[c, f] > 0}
  planted = {p: [] for p in BIG_PAIRS}

  def cut(view, pair):
    _keep_first(rig, view + (0,), pair[0], 0, SEGMENT)
    _keep_first(rig, view + (0,), pair[1], SEGMENT, P)
    planted[pair].append(view)
    free.discard(view)

  for pair in sorted(BIG_PAIRS, key=lambda p: (p[0] + p[1], p), reverse=True):
    fits = [v for v in free if n0[v] >= pair[0] and n1[v] >= pair[1]]
    if not fits:
      return None
    cut(min(fits, key=lambda v: (n0[v] + n1[v], v)), pair)
  for i, view in enumerate(sorted(free)):
    fits = [p for p in BIG_PAIRS if n0[view] >= p[0] and n1[view] >= p[1]]
    cut(view, fits[i % len(fits)])
  return planted


@functools.lru_cache(maxsize=None)
def planted_bigboard(unit, motion, optk, seed=71):
  """(rig, {(n0, n1): [(camera, frame), ...]}): an 816-point board (two segments of the kernels' walk) next to an 81-point one; the
  views of the big board hold n0 inliers in slots [0, 512) and n1 in [512, 816) for every pair of BIG_PAIRS: an empty first or second
  segment, full chunks on both sides, a tail on either.  Views of the big board that are left over are cut to the pairs in turn.
  Cached, read-only tables."""
  assert (unit, motion, optk) in BIG_SHAPES
  for frames in BIG_FRAME_CHOICES:
    rig = _make(unit, motion, optk, ["charuco_25x35", "charuco_10x10"], frames, seed)
    planted = _plant_big(rig)
    if planted is not None:
      break
  assert planted is not None, f"{rig.name}: no frame count of {BIG_FRAME_CHOICES} has a view for every pair"
  for pair, views in planted.items():
    assert views, (rig.name, pair)
    for v in views:
      assert (rig.valid[v][0][:SEGMENT].sum(), rig.valid[v][0][SEGMENT:].sum()) == pair
  return _freeze(rig), planted


def view_mask(rig, views, board=0):
  """Inlier mask [C, F, B, P] that keeps the valid observations of the given (camera, frame) views of one board only."""
  mask = np.zeros(rig.valid.shape, dtype=bool)
  for c, f in views:
    mask[c, f, board] = rig.valid[c, f, board]
  return mask
