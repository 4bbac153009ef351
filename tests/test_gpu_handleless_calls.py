"""The seven handle-less entry families (pose alignment, pose table, intrinsics, hand-eye start, undistortion, triangulation, rig
localisation) share one call scaffold (csrc/mcba_host.h: DeviceCall) and one resource cache: streams and buffers parked by one family
are taken by the next.  One process, one thread: every family twice, interleaved A .. G A .. G, at the smallest shapes -- the second
result of each is the first byte for byte, every family's timing count is its own, and a call refused at argument checking leaves
that family's message in mcba_last_error() and the next valid call returns the bytes it returned before.  (Every refusal here comes
before the call takes its stream: argument errors only, so the parking of a call that fails on the device is not exercised.)"""
import ctypes as C

import numpy as np
import pytest

import handeye_host_lib as hh
import intrinsic_host_lib as I
import localize_host_lib as lh
import pnp_host_lib as L
import triangulate_host_lib as th
import undistort_host_lib as uh
from multical_amd import _lib, localize, synthetic, tables, triangulate, undistort

pytestmark = pytest.mark.gpu

CAMERAS = uh.fixture_cameras()


def _alignment_problems():
  rng = np.random.default_rng(3)
  T = synthetic.to_matrix(np.array([0.3, -0.2, 0.5, 0.1, 0.2, -0.4]))
  problems = []
  for n in (9, 30, 200):
    a = synthetic.to_matrix(np.concatenate([rng.normal(0, 0.5, (n, 3)), rng.normal(0, 1.0, (n, 3))], axis=1))
    b = synthetic.perturb(T @ a, rng, 1e-3, 1e-3)
    problems.append((a, b, rng.random(n) < 0.85))
  return problems


def _count(getter, slots=4):
  return _lib.call_ms(getter, range(slots))[1]


def _bytes(arrays):
  return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def _last_error():
  return _lib.load().mcba_last_error().decode()


def test_seven_families_interleaved_through_one_cache():
  rig = L.golden_rig("tiny")
  irig = I.rig("tiny")
  ta, va, tb, vb, _, _ = hh.interleaved_problem(5, 6, n_rows=2)
  problems = _alignment_problems()
  rng = np.random.default_rng(11)
  X = np.concatenate([rng.uniform(-0.3, 0.3, (1000, 2)), rng.uniform(1.0, 2.0, (1000, 1))], axis=1)
  of = rng.integers(0, len(CAMERAS), 1000).astype(np.int32)
  image = uh.noise_image(5, (1, uh.IMAGE_SIZE[1], uh.IMAGE_SIZE[0]), np.uint8)
  trig = th.make_rig(2, 1, 65)                        # (65 points: across one 64-lane edge)
  lrig = lh.named_rig("1cam-2board-pin5-rolling")     # (4 frames)

  def align():
    out, valid, inliers = tables.align_transforms_robust_batch(problems)
    return _bytes([out, valid] + list(inliers))

  def view_poses():
    return _bytes(tables.view_poses(rig.points, rig.valid, rig.board_points, rig.truth.cameras))

  def intrinsics():
    out = tables.calibrate_intrinsics(I.table_of(irig), irig.board_points, irig.image_sizes, model=irig.models)
    return _bytes(out[k] for k in ("cameras", "poses", "sse", "n_used", "view_status", "camera_status", "lm_iterations"))

  def hand_eye():
    return _bytes(tables.hand_eye_batch(ta, va, tb, vb, [0, 1], [0, 1]))

  def undistortion():
    uv = undistort.project_points(CAMERAS, X, of)
    return _bytes([uv, undistort.undistort_images(CAMERAS, image, [0], image_size=(57, 5))])

  def triangulation():
    r = th.run(trig, "device")
    return _bytes(r[k] for k in ("points", "cov", "sse", "error", "n_views", "status"))

  def localisation():
    r = lh.run(lrig, "device")
    return _bytes(r[k] for k in ("poses", "poses_end", "cov", "sse", "n_obs", "iters", "error", "status"))

  families = [align, view_poses, intrinsics, hand_eye, undistortion, triangulation, localisation]
  first = [f() for f in families]
  second = [f() for f in families]
  for f, a, b in zip(families, first, second):
    assert len(a) > 0 and a == b, f.__name__

  # the timing state belongs to the family: each count is what that family's last call worked on
  status = tables.view_poses(rig.points, rig.valid, rig.board_points, rig.truth.cameras)[3]
  out = tables.calibrate_intrinsics(I.table_of(irig), irig.board_points, irig.image_sizes, model=irig.models)
  assert np.all(out.camera_status == tables.CAMERA_OK)
  idle = (tables.VIEW_MASKED, tables.VIEW_TOO_FEW)
  counts = dict(view_poses=int((~np.isin(status, idle)).sum()), intrinsics=int((~np.isin(out.view_status, idle)).sum()),
                hand_eye=2, undistortion=57 * 5, triangulation=65, localisation=4)
  assert len(set(counts.values())) == 6, counts          # (shapes chosen so that a mixed-up count shows)
  hand_eye()
  undistortion()
  triangulation()
  localisation()
  got = dict(view_poses=_count("view_poses"), intrinsics=_count("calibrate_intrinsics"), hand_eye=_count("hand_eye"),
             undistortion=_count("undistort"), triangulation=_count("triangulate"), localisation=_count("rig_poses", 5))
  assert got == counts

  # refused at argument checking: the family's own message, and the next valid call returns the bytes it returned before
  bumpy = np.asarray(rig.board_points[0], dtype=np.float64).copy()
  bumpy[::3, 2] += 0.005
  ibumpy = np.asarray(irig.board_points[0], dtype=np.float64).copy()
  ibumpy[::3, 2] += 0.005
  def null_points():           # (the raw call: the wrapper never leaves X out)
    p, out, keep = th.raw_problem(trig)
    _lib.check(_lib.load().mcba_triangulate(C.byref(p), None, None, None, None, None, _lib.up(out["status"])))

  def too_many_cameras():
    p, out, keep = lh.raw_problem(lrig, n_cameras=localize.MAX_CAMERAS + 1)
    _lib.check(lh.raw_call(_lib.load().mcba_rig_poses, p, out))

  refused = [
      (lambda: tables.align_transforms_robust_indexed(problems[2][0], np.full(200, 200), np.zeros(200, dtype=np.int64),
                                                      np.array([9, 30, 161])), "pose index out of range"),
      (lambda: tables.view_poses(rig.points, rig.valid, [bumpy] + list(rig.board_points[1:]), rig.truth.cameras),
       "mcba_view_poses: board 0 is not planar"),
      (lambda: tables.calibrate_intrinsics(I.table_of(irig), [ibumpy] + list(irig.board_points[1:]), irig.image_sizes, model=irig.models),
       "mcba_calibrate_intrinsics: board 0 is not planar"),
      (lambda: tables.hand_eye_batch(ta, va, tb, vb, [0, 2], [0, 1]), "mcba_hand_eye: problem 1: rows (2, 1) outside tables of 2 and 2 rows"),
      (lambda: undistort.remap(np.zeros((1, 4, 4, 2), dtype=np.uint8), np.zeros((4, 4, 2), dtype=np.float32)),
       "mcba_remap: images of 1 or 3 channels are served, not 2"),
      (null_points, "mcba_triangulate: null argument"),
      (too_many_cameras, "mcba_rig_poses: 65 cameras, at most 64 are served"),
  ]
  for (call, message), family, before in zip(refused, families, first):
    with pytest.raises(RuntimeError) as e:
      call()
    assert message in str(e.value) and message in _last_error(), (family.__name__, str(e.value), _last_error())
    assert family() == before, family.__name__
