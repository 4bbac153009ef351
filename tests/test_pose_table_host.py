"""Per-view board poses (tables.make_pose_table / mcba_view_poses): the mathematics of multical_amd/csrc/mcba_pnp.h built for the
host (tests/pnp_host), pinned by an independent numpy / scipy restatement (tests/pnp_reference.py), and the table conventions
of the Python layer with that host build standing in for the device call.

Tolerances are measured, not assumed:
  noise-free views   100 x the restatement's own worst recovery error on the same views, floor 1e-12 (rad, m);
  noisy views        max(1e-9, 100 x the distance between scipy's two end points) -- one started at the truth, one at the pose
                     under test -- for the pose (rad, m) and the sum of squared pixel distances.
MCBA_WRITE_PROFILES=1 writes the measured figures to profiles/pose_table_parity.txt.

Note on tiny_tilted and tiny_mixed (one tilted camera): synthetic._project, which synthesises the noise-free corners, carries no
sensor tilt while the product's projection does, so there the truth chain is not the optimum of either the header or the
restatement (both end 1.4e-2 / 1.9e-2 rad | m away from it, and agree with each other); the recovery bound on those two is the
restatement's own.  Measured on the other fixtures: header 7e-16 .. 4e-14, restatement 7e-16 .. 1.4e-14.
"""
import os
import pickle

import numpy as np
import pytest

import pnp_host_lib as L
import pnp_reference as ref
from multical_amd import board as mboard
from multical_amd import synthetic, tables
from multical_amd.structs import Table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_figures = []


def _record(line):
  _figures.append(line)
  print(line)


def _active_views(status):
  return [tuple(v) for v in np.argwhere(status == tables.VIEW_OK)]


def _perturbed(pose, k):
  rng = np.random.default_rng([977, k])
  return synthetic.to_matrix(np.concatenate([rng.normal(0, 1e-3, 3), rng.normal(0, 1e-3, 3)])) @ pose


@pytest.fixture(scope="module")
def noisy():
  cache = {}

  def get(name):
    if name not in cache:
      rig = L.golden_rig(name)
      cache[name] = (rig, L.view_poses(rig.points, rig.valid, rig.board_points, rig.truth.cameras))
    return cache[name]
  return get


@pytest.mark.parametrize("name", L.FIXTURES)
def test_noise_free_recovery(name):
  rig = L.golden_rig(name)
  chain = L.truth_chain(rig)
  points, ok = L.noise_free_points(rig)
  poses, sse, n_used, status, _ = L.view_poses(points, ok, rig.board_points, rig.truth.cameras)
  views = _active_views(status)
  assert len(views) > 0
  assert np.all((status == tables.VIEW_OK) | (status == tables.VIEW_TOO_FEW))
  assert np.array_equal(n_used[status == tables.VIEW_OK], ok.sum(axis=3)[status == tables.VIEW_OK])
  worst_ref, worst = 0.0, 0.0
  for k, (c, f, b) in enumerate(views):
    m = np.flatnonzero(ok[c, f, b])
    X = np.asarray(rig.board_points[b], dtype=np.float64)[m]
    r, _ = ref.solve(rig.truth.cameras[c], X, points[c, f, b][m], _perturbed(chain[c, f, b], k))
    worst_ref = max(worst_ref, *[float(v[0]) for v in L.pose_distance(r[None], chain[c, f, b][None])])
    worst = max(worst, *[float(v[0]) for v in L.pose_distance(poses[c, f, b][None], chain[c, f, b][None])])
  bound = max(1e-12, 100 * worst_ref)
  _record(f"noise-free {name}: {len(views)} views, recovery error of the header {worst:.3e}, of the scipy restatement "
          f"{worst_ref:.3e} (rad | m), bound {bound:.3e}")
  assert worst <= bound


@pytest.mark.parametrize("name", L.FIXTURES)
def test_noisy_optimum_is_the_restatements(name, noisy):
  rig, (poses, sse, n_used, status, iters) = noisy(name)
  chain = L.truth_chain(rig)
  views = _active_views(status)
  assert len(views) > 0
  worst = [0.0, 0.0, 0.0, 0.0]
  for c, f, b in views:
    m = np.flatnonzero(rig.valid[c, f, b])
    X = np.asarray(rig.board_points[b], dtype=np.float64)[m]
    r, r_sse, spread, spread_sse = ref.pin_view(rig.truth.cameras[c], X, rig.points[c, f, b][m], chain[c, f, b], poses[c, f, b])
    d = max(float(v[0]) for v in L.pose_distance(r[None], poses[c, f, b][None]))
    ds = abs(r_sse - sse[c, f, b])
    worst = [max(worst[0], d), max(worst[1], spread), max(worst[2], ds), max(worst[3], spread_sse)]
    assert d <= max(1e-9, 100 * spread), (c, f, b, d, spread)
    assert ds <= max(1e-9, 100 * spread_sse), (c, f, b, ds, spread_sse)
  _record(f"noisy {name}: {len(views)} views, pose difference to scipy {worst[0]:.3e} (scipy's own two end points {worst[1]:.3e}) "
          f"rad | m, sse difference {worst[2]:.3e} (scipy's own {worst[3]:.3e}) px^2, LM linearisations mean "
          f"{iters[status == 0].mean():.1f} max {iters[status == 0].max()}")


def test_reduction_orders_agree(noisy):
  """table order against the device's order (64 lane partials + xor butterfly): the same optimum to rounding, same counts"""
  rig, a = noisy("tiny_bigboard")
  b = L.view_poses(rig.points, rig.valid, rig.board_points, rig.truth.cameras, pairwise=True)
  assert np.array_equal(a[3], b[3]) and np.array_equal(a[2], b[2])
  assert np.abs(a[0] - b[0]).max() < 1e-10 and np.abs(a[1] - b[1]).max() < 1e-8


def test_four_corners_and_three():
  rig = L.golden_rig("tiny")
  chain = L.truth_chain(rig)
  points, ok = L.noise_free_points(rig)
  c, f, b = _active_views(L.view_poses(points, ok, rig.board_points, rig.truth.cameras)[3])[0]
  ids = np.flatnonzero(ok[c, f, b])
  keep4 = ids[[0, 3, len(ids) // 2, len(ids) - 1]]      # (the first and last rows of the grid: not collinear)
  for keep, want in ((keep4, tables.VIEW_OK), (keep4[:3], tables.VIEW_TOO_FEW)):
    v = np.zeros_like(ok)
    v[c, f, b, keep] = True
    poses, sse, n_used, status, _ = L.view_poses(points, v, rig.board_points, rig.truth.cameras)
    assert status[c, f, b] == want
    assert (np.delete(status.ravel(), np.ravel_multi_index((c, f, b), status.shape)) == tables.VIEW_TOO_FEW).all()
    if want == tables.VIEW_OK:
      assert n_used[c, f, b] == 4
      m = keep
      r, _ = ref.solve(rig.truth.cameras[c], np.asarray(rig.board_points[b], dtype=np.float64)[m], points[c, f, b][m],
                       _perturbed(chain[c, f, b], 0))
      bound = max(1e-12, 100 * max(float(x[0]) for x in L.pose_distance(r[None], chain[c, f, b][None])))
      assert max(float(x[0]) for x in L.pose_distance(poses[c, f, b][None], chain[c, f, b][None])) <= bound
    else:
      assert np.array_equal(poses[c, f, b], np.eye(4)) and sse[c, f, b] == 0 and n_used[c, f, b] == 0


def test_collinear_corners_are_degenerate():
  rig = L.golden_rig("tiny")
  points, ok = L.noise_free_points(rig)
  c, f, b = _active_views(L.view_poses(points, ok, rig.board_points, rig.truth.cameras)[3])[0]
  ids = np.flatnonzero(ok[c, f, b])
  row = ids[ids // 9 == ids[len(ids) // 2] // 9]        # one row of the 9 x 9 corner grid
  assert len(row) >= 4
  v = np.zeros_like(ok)
  v[c, f, b, row] = True
  poses, sse, n_used, status, _ = L.view_poses(points, v, rig.board_points, rig.truth.cameras)
  assert status[c, f, b] == tables.VIEW_DEGENERATE and np.array_equal(poses[c, f, b], np.eye(4)) and n_used[c, f, b] == 0


@pytest.mark.parametrize("name", ["tiny", "tiny_pin4", "tiny_rational", "tiny_thin_prism", "tiny_tilted", "tiny_fisheye"])
def test_undistortion_inverts_the_projection(name):
  """Newton on the header's own distortion against the oracle's restatement of the OpenCV projection, tilt included"""
  rig = L.golden_rig(name)
  cam = rig.truth.cameras[0]
  rng = np.random.default_rng(5)
  lim = 1.2 if cam.model == 'fisheye' else 0.4
  q = rng.uniform(-lim, lim, (50, 2))
  from oracle import restate
  uv = restate.OracleCamera(cam.image_size, cam.intrinsic, cam.dist, model=cam.model).project(np.concatenate([q, np.ones((50, 1))], axis=1))
  got, ok = L.undistort(cam, uv)
  assert ok.all()
  assert np.abs(got - q).max() < 1e-12
  want, ok2 = ref.undistort(cam, uv)
  assert ok2.all() and np.abs(got - want).max() < 1e-12


def test_corner_outside_the_monotone_range_is_dropped():
  """a pixel the distortion cannot reach (beyond the fold of a strongly negative k1) does not converge: dropped, not a NaN"""
  cam = synthetic._make_camera("standard", np.random.default_rng(0))
  cam.dist = np.array([-0.5, 0.0, 0.0, 0.0, 0.0])
  got, ok = L.undistort(cam, np.array([[cam.intrinsic[0, 2] + 5000.0, cam.intrinsic[1, 2]]]))
  assert not ok[0]


# ---- has_min_detections ----------------------------------------------------------------------------------------------------
def _random_id_sets(n_points, rng, tags):
  sets = []
  for k in range(60):
    sets.append(np.sort(rng.choice(n_points, size=int(rng.integers(0, min(n_points, 50))), replace=False)))
  return sets


@pytest.mark.needs_reference
@pytest.mark.parametrize("kind", ["charuco", "aprilgrid"])
def test_min_detections_mask_is_the_references(kind):
  import importlib
  from oracle import refload
  refload.load()
  grid = importlib.import_module("multical.board.common").has_min_detections_grid
  rng = np.random.default_rng(3)
  if kind == "charuco":
    b = mboard.CharucoBoard(size=(10, 8), square_length=0.04, marker_length=0.03)
    cell = lambda ids: ids
    rows_only = np.arange(20)                       # 20 ids in rows 0 and 1 of the (h, w) = (8, 10) unravel: count passes, rows fail
    count_only = np.array([0, 11, 22, 33, 44, 55])  # three rows and columns and more, 6 < 20 ids
  else:
    b = mboard.AprilGrid(size=(6, 5), tag_length=0.06, tag_spacing=0.3)
    cell = lambda ids: ids // 4
    rows_only = np.arange(24)                       # the four corners of tags 0..5 = one row of tags: 24 >= 12 ids, one row
    count_only = np.array([0, 4 * 7, 4 * 14])       # three tags on the diagonal, 3 < 12 ids
  assert b.min_rows == (3 if kind == "charuco" else 2) and b.min_points == (20 if kind == "charuco" else 12)
  sets = _random_id_sets(b.num_points, rng, kind == "aprilgrid") + [rows_only, count_only, np.arange(b.num_points), np.zeros(0, dtype=int)]
  valid = np.zeros((1, len(sets), 1, b.num_points + 3), dtype=bool)      # (padded like a table that holds a larger board too)
  for f, ids in enumerate(sets):
    valid[0, f, 0, ids] = True
  got = tables.min_detections_mask(valid, [b])[0, :, 0]
  want = np.array([bool(grid(b.size, cell(ids), b.min_points, b.min_rows)) for ids in sets])
  assert np.array_equal(got, want)
  assert want.any() and not want.all()
  assert not got[len(sets) - 4] and not got[len(sets) - 3] and got[len(sets) - 2]


def test_min_detections_mask_without_grid_attributes_passes_everything():
  valid = np.zeros((2, 3, 1, 10), dtype=bool)
  assert tables.min_detections_mask(valid, [mboard.Board(np.zeros((10, 3)))]).all()


# ---- table conventions (the host build in place of the device call) -----------------------------------------------------
@pytest.fixture()
def host_backend(monkeypatch):
  monkeypatch.setattr(tables, "view_poses", L.view_poses)


def _make(rig, **k):
  from multical_amd.board import Board
  boards = [Board(p, name=f"board{i}") for i, p in enumerate(rig.board_points)]
  return tables.make_pose_table(Table.create(points=rig.points, valid=rig.valid), boards, rig.truth.cameras, return_info=True, **k)


@pytest.mark.parametrize("name", ["cfg5_40", "tiny_edge"])
def test_table_conventions(name, host_backend):
  rig = L.golden_rig(name)
  t, info = _make(rig)
  assert set(t.keys()) == {"poses", "valid", "num_points", "reprojection_error", "view_angles"}
  assert t.poses.shape == rig.valid.shape[:3] + (4, 4) and t.view_angles.shape == rig.valid.shape[:3] + (3,)
  bad = ~t.valid
  assert bad.any() and t.valid.any()
  assert np.array_equal(t.poses[bad], np.broadcast_to(np.eye(4), (bad.sum(), 4, 4)))
  assert (t.num_points[bad] == 0).all() and (t.reprojection_error[bad] == 0).all() and (t.view_angles[bad] == 0).all()
  assert np.array_equal(t.valid, (info.status == tables.VIEW_OK) & (info.error <= 1.0))
  assert np.array_equal(t.num_points[t.valid], rig.valid.sum(axis=3)[t.valid])
  assert np.array_equal(t.reprojection_error[t.valid], info.error[t.valid])
  # empty views (tiny_edge: invalid cameras, frames and boards hold none) are reported as too few corners
  assert (info.status[rig.valid.sum(axis=3) < 4] == tables.VIEW_TOO_FEW).all()
  from scipy.spatial.transform import Rotation
  want = Rotation.from_rotvec(Rotation.from_matrix(t.poses[t.valid][:, :3, :3]).as_rotvec()).as_euler('xyz', degrees=True)
  assert np.abs(t.view_angles[t.valid] - want).max() < 1e-9
  # both error norms differ by exactly sqrt(2); without exclusion every converged view stays
  t2, info2 = _make(rig, error_norm='coordinate', exclude_bad_poses=False)
  assert np.array_equal(t2.valid, info.status == tables.VIEW_OK)
  np.testing.assert_allclose(info.error[t2.valid], info2.error[t2.valid] * np.sqrt(2.0), rtol=4e-16, atol=0)
  if name == "cfg5_40":
    estimated = info.status == tables.VIEW_OK
    rejected = (estimated & ~t.valid).sum() / estimated.sum()
    _record(f"cfg5_40: {estimated.sum()} views estimated, {rejected:.3f} of them above the 1 px limit")
    assert 0.25 < rejected < 0.75          # "about half": every view that holds one of the fixture's 1 % gross corner outliers


def test_workspace_initialise_poses_builds_the_calibration(host_backend, monkeypatch):
  """the Python chain detections -> pose table -> initialisation -> Calibration, with the host build for the per-view poses and the
  oracle's numpy restatement of tables.initialise_poses for the pose graph (both are device calls in the product)"""
  from multical_amd import calibration
  from multical_amd.structs import struct
  from multical_amd.workspace import Workspace
  from oracle import restate_init

  def initialise(pose_table, camera_poses=None):
    r = restate_init.initialise_poses(restate_init.table(pose_table.poses, pose_table.valid), pose_table.num_points, camera_poses)
    return struct(**{k: Table.create(poses=v["poses"], valid=v["valid"]) for k, v in r.items()})
  monkeypatch.setattr(tables, "initialise_poses", initialise)
  rig = L.golden_rig("cfg5_40")
  own = calibration.from_rig(rig)
  ws = Workspace()
  init = ws.initialise_poses(own.point_table, list(own.boards), list(own.cameras))
  assert ws.initialisation is init and ws.pose_table.valid.any()
  assert init.camera_poses.pose_table.valid.all() and init.board_poses.pose_table.valid.all() and init.motion.valid.all()
  chain = (init.camera_poses.pose_table.poses[:, None, None] @ init.motion.pose_table.poses[None, :, None]
           @ init.board_poses.pose_table.poses[None, None, :])
  ang, d = L.pose_distance(chain[ws.pose_table.valid], L.truth_chain(rig)[ws.pose_table.valid])
  assert ang.max() < 0.1 and d.max() < 0.1          # a start the bundle adjustment converges from (measured: 0.031 rad, 0.043 m)
  assert init.enable(**rig.optimize).param_vec.size == own.param_vec.size


def test_error_norm_is_checked(host_backend):
  with pytest.raises(ValueError):
    _make(L.golden_rig("tiny"), error_norm='pixel')


def test_boards_pickled_before_the_keywords_still_load():
  old = dict(size=(10, 10), square_length=0.04, marker_length=0.03, adjusted_points=None, points=None, name="b")   # the former state
  b = mboard.CharucoBoard.__new__(mboard.CharucoBoard)
  b.__setstate__(dict(old))
  assert (b.min_rows, b.min_points) == (3, 20) and b.num_points == 81
  a = mboard.AprilGrid.__new__(mboard.AprilGrid)
  a.__setstate__(dict(size=(9, 9), tag_length=0.06, tag_spacing=0.3, adjusted_points=None, points=None, name="a"))
  assert (a.min_rows, a.min_points) == (2, 12) and a.num_points == 324
  c = pickle.loads(pickle.dumps(mboard.CharucoBoard(size=(10, 10), square_length=0.04, marker_length=0.03, min_rows=4, min_points=9)))
  assert (c.min_rows, c.min_points) == (4, 9)


def test_zz_write_profile():
  """(not a check) MCBA_WRITE_PROFILES=1: the figures the tests above measured go to profiles/pose_table_parity.txt"""
  if os.environ.get("MCBA_WRITE_PROFILES") and _figures:
    with open(os.path.join(ROOT, "profiles", "pose_table_parity.txt"), "w") as fh:
      fh.write("Per-view board poses: the host build of csrc/mcba_pnp.h against tests/pnp_reference.py (tests/test_pose_table_host.py)\n")
      fh.write("\n".join(_figures) + "\n")
