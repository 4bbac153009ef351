"""mcba_view_poses / k_view_pose on the MI355X: against the host build of the same header (tests/pnp_host) on every fixture,
repeatability, supplied start poses, non-planar boards, empty launches, and detections -> pose table -> initialisation ->
bundle adjustment end to end.

Tolerance of device against host: max(1e-10, 100 x the host build's own difference between its two reduction orders) -- corners
summed in table order against the device's order (64 lane partials folded by the xor butterfly).  What remains between the device
and the host build in the device's order is FMA contraction and libm.  (The host build's two orders differ by 3e-16 .. 3e-14 in the
poses and 1e-12 .. 5e-11 px^2 in sse on these fixtures, so the floor of 1e-10 decides nearly everywhere.  No figure of a hardware run is
recorded here yet.)"""
import ctypes as C

import numpy as np
import pytest

import pnp_host_lib as L
from multical_amd import _lib, calibration, synthetic, tables
from multical_amd.workspace import Workspace

pytestmark = pytest.mark.gpu


def _tolerances(rig, **k):
  """(host result in the device's order, pose tolerance, sse tolerance)"""
  a = L.view_poses(rig.points, rig.valid, rig.board_points, rig.truth.cameras, pairwise=False, **k)
  b = L.view_poses(rig.points, rig.valid, rig.board_points, rig.truth.cameras, pairwise=True, **k)
  assert np.array_equal(a[3], b[3]) and np.array_equal(a[2], b[2])
  return b, max(1e-10, 100 * np.abs(a[0] - b[0]).max()), max(1e-10, 100 * np.abs(a[1] - b[1]).max())


@pytest.fixture(scope="module")
def device():
  cache = {}

  def get(name):
    if name not in cache:
      rig = L.golden_rig(name)
      cache[name] = tables.view_poses(rig.points, rig.valid, rig.board_points, rig.truth.cameras)
    return cache[name]
  return get


@pytest.mark.parametrize("name", L.FIXTURES)
def test_device_matches_host_build(name, device):
  rig = L.golden_rig(name)
  host, tol_pose, tol_sse = _tolerances(rig)
  poses, sse, n_used, status, iters = device(name)
  print(f"{name}: |pose| {np.abs(poses - host[0]).max():.3e} (tolerance {tol_pose:.3e}), |sse| {np.abs(sse - host[1]).max():.3e} "
        f"(tolerance {tol_sse:.3e}), {int((status == 0).sum())} views, LM linearisations mean {iters[status == 0].mean():.1f}")
  assert np.array_equal(status, host[3])
  assert np.array_equal(n_used, host[2])
  assert (status == tables.VIEW_OK).any()
  assert np.abs(poses - host[0]).max() <= tol_pose
  assert np.abs(sse - host[1]).max() <= tol_sse


@pytest.mark.parametrize("name", ["tiny_fishmix", "tiny_bigboard"])
def test_two_calls_return_the_same_bits(name, device):
  rig = L.golden_rig(name)
  again = tables.view_poses(rig.points, rig.valid, rig.board_points, rig.truth.cameras)
  for a, b in zip(device(name), again):
    assert a.tobytes() == b.tobytes()


def test_supplied_start_poses_reach_the_same_optimum(device):
  rig = L.golden_rig("tiny_mixed")
  _, tol_pose, tol_sse = _tolerances(rig)
  first = device("tiny_mixed")
  poses, sse, n_used, status, iters = tables.view_poses(rig.points, rig.valid, rig.board_points, rig.truth.cameras, init_poses=first[0])
  assert np.array_equal(status, first[3]) and np.array_equal(n_used, first[2])
  assert np.abs(poses - first[0]).max() <= tol_pose and np.abs(sse - first[1]).max() <= tol_sse
  # started AT the optimum the refinement has nothing left to do (the homography start needs several linearisations)
  ok = status == tables.VIEW_OK
  assert iters[ok].max() <= 3 and first[4][ok].mean() > iters[ok].mean()


def _bumpy(rig):
  """the fixture's board with every third corner lifted 5 mm off the plane, and its noise-free detections"""
  pts = np.asarray(rig.board_points[0], dtype=np.float64).copy()
  pts[::3, 2] += 0.005
  bumpy = synthetic.rig_from_arrays(synthetic.rig_to_arrays(rig))
  bumpy.board_points = [pts] + list(rig.board_points[1:])
  return bumpy, L.noise_free_points(bumpy)


def test_non_planar_board_needs_start_poses():
  rig, (points, ok) = _bumpy(L.golden_rig("tiny"))
  with pytest.raises(_lib.McbaError, match="board 0 is not planar"):
    tables.view_poses(points, ok, rig.board_points, rig.truth.cameras)
  chain = L.truth_chain(rig)
  rng = np.random.default_rng(8)
  start = synthetic.perturb(chain, rng, 5e-3, 5e-3)
  poses, sse, n_used, status, _ = tables.view_poses(points, ok, rig.board_points, rig.truth.cameras, init_poses=start)
  good = status == tables.VIEW_OK
  assert good.any() and np.array_equal(good, ok.sum(axis=3) >= 4)
  ang, d = L.pose_distance(poses[good], chain[good])
  assert ang.max() < 1e-9 and d.max() < 1e-9 and sse.max() < 1e-12
  # ... and the library still works after the refused call
  flat = L.golden_rig("tiny")
  assert (tables.view_poses(flat.points, flat.valid, flat.board_points, flat.truth.cameras)[3] == tables.VIEW_OK).any()


def test_all_views_masked_launches_nothing():
  rig = L.golden_rig("tiny")
  mask = np.zeros(rig.valid.shape[:3], dtype=bool)
  poses, sse, n_used, status, iters = tables.view_poses(rig.points, rig.valid, rig.board_points, rig.truth.cameras, view_mask=mask)
  ms, n_active = (C.c_double * 4)(), C.c_int64(-1)
  _lib.check(_lib.load().mcba_debug_view_poses_ms(ms, C.byref(n_active)))
  assert n_active.value == 0 and ms[1] == 0.0 and ms[2] == 0.0          # no upload, no kernel
  assert np.array_equal(poses, np.broadcast_to(np.eye(4), poses.shape))
  assert (sse == 0).all() and (n_used == 0).all() and (status == tables.VIEW_MASKED).all() and (iters == 0).all()
  # a partial mask: masked views are identities, the others are untouched by the mask
  mask[0] = True
  part = tables.view_poses(rig.points, rig.valid, rig.board_points, rig.truth.cameras, view_mask=mask)
  full = tables.view_poses(rig.points, rig.valid, rig.board_points, rig.truth.cameras)
  assert (part[3][1:] == tables.VIEW_MASKED).all() and part[0][0].tobytes() == full[0][0].tobytes()


@pytest.mark.parametrize("name,exclude_bad_poses", [("cfg1", False), ("cfg5_40", True)])
def test_detections_to_bundle_adjustment(name, exclude_bad_poses):
  """detections -> make_pose_table -> initialise_poses -> Calibration -> bundle_adjust reaches the optimum the fixture's own
  initial guess reaches (the optimum does not depend on the start): RMS within 1e-9 px, the project's residual-parity unit.
  cfg1 keeps every converged view (its 315-corner views nearly all hold one of the fixture's gross outlier corners and its cameras
  are the fixture's perturbed ones, held fixed: one view of 27 is below 1 px); cfg5_40 runs the reference's default rejection at
  1 px, which drops about half of its views, and initialises from the rest."""
  rig = L.golden_rig(name)
  own = calibration.from_rig(rig)                     # the fixture's x0: cameras, optimise flags, perturbed poses
  tight = dict(tolerance=1e-15, xtol=1e-15, gtol=1e-15, max_iterations=300, solver="native")
  want = own.bundle_adjust(**tight)
  ws = Workspace()
  init = ws.initialise_poses(own.point_table, list(own.boards), list(own.cameras), exclude_bad_poses=exclude_bad_poses,
                             pose_error_limit=1.0)
  assert ws.calibrations["initialisation"] is init
  table = ws.pose_table
  estimated = table.valid.sum()
  assert estimated > 0 and (not exclude_bad_poses or estimated < (rig.valid.sum(axis=3) >= 4).sum())   # (the rejection path ran)
  got = init.enable(**rig.optimize).bundle_adjust(**tight)
  rms = lambda c: float(np.sqrt(np.mean(np.square(c.reprojection_error))))
  print(f"{name}: {int(estimated)} of {int((rig.valid.sum(axis=3) >= 4).sum())} views in the pose table, rms from the estimated table "
        f"{rms(got):.12f} px, from the fixture's x0 {rms(want):.12f} px, at the initialisation {rms(init):.3f} px")
  assert abs(rms(got) - rms(want)) < 1e-9
