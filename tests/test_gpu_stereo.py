"""mcba_stereo_calibrate / k_stereo_pair on the MI355X: against the host build of the same header (tests/stereo_host) run in the
device's summation order, bit-reproducibility, the call that has nothing to do, and -- end to end -- the two-camera bundle adjustment
whose cost is the same function, and Calibration.pairwise_extrinsics pointing at a displaced camera.

Shapes (synthetic.make_rig): tiny (16 frames) 1 pair of 8 views, 81 slots = one full chunk + 17; tiny_pin4 (16) 5 views: one wave
takes two, three take one; tiny_mixed (16) 6 pairs of 7 .. 12 views in one launch, mixed families inside a pair; tiny_fishmix (16, two
boards) 6 pairs of 10 .. 18 views, pinhole with fisheye (device against host build only: the data are rolling); tiny_bigboard (8)
7 views of 816 slots = 13 chunks beside an 81-slot board; masks leave pairs of 3 views (an idle wave), 1 view (three idle waves) and 0
views (not launched)."""
from types import SimpleNamespace

import numpy as np
import pytest

import stereo_host_lib as sh
from multical_amd import calibration, stereo

pytestmark = pytest.mark.gpu

RIGS = [("tiny", 16, 1, (8, 8)), ("tiny_pin4", 16, 1, (5, 5)), ("tiny_mixed", 16, 6, (7, 12)), ("tiny_fishmix", 16, 6, (10, 18)),
        ("tiny_bigboard", 8, 1, (7, 7))]
KEYS = ("T", "cov", "sse", "view_poses", "view_sse")
_cache, _launched = {}, {}


def solved(name, frames):
  """(case, device result, host build in table order, host build in the device's order), computed once.  _launched[name]: the
  pairs the device call launched."""
  if name not in _cache:
    case = sh.make_case(name, frames=frames)
    dev = sh.run(case, backend="device")
    _launched[name] = stereo.last_call_ms()[1]
    _cache[name] = (case, dev, sh.run(case), sh.run(case, order=True))
  return _cache[name]


def tolerance(a, b):
  """max(1e-10, 100 x the host build's own difference between its two summation orders)."""
  return max(1e-10, 100 * float(np.abs(np.asarray(a) - np.asarray(b)).max()))


def assert_device_equals_host(dev, host, serial, what):
  for key in ("status", "n_views", "n_points", "iterations"):
    assert np.array_equal(dev[key], host[key]), (what, key)
  for key in KEYS:
    d, tol = float(np.nanmax(np.abs(dev[key] - host[key]))), tolerance(host[key], serial[key])
    print(f"{what} {key}: device - host {d:.3e}, bound {tol:.3e}")
    assert np.array_equal(np.isnan(dev[key]), np.isnan(host[key])) and d <= tol, (what, key)


@pytest.mark.parametrize("name,frames,n_pairs,views", RIGS)
def test_device_equals_host_build(name, frames, n_pairs, views):
  case, dev, serial, host = solved(name, frames)
  assert len(dev.pairs) == n_pairs and (dev.n_views.min(), dev.n_views.max()) == views
  assert (dev.status == stereo.OK).all()
  print(f"{name}: views {list(dev.n_views)}, points {list(dev.n_points)}, passes {list(dev.iterations)}, rms {list(np.round(dev.rms, 4))}")
  assert_device_equals_host(dev, host, serial, name)
  assert _launched[name] == n_pairs


def test_two_calls_return_the_same_bits():
  case, dev, _, _ = solved("tiny_mixed", 16)
  again = sh.run(case, backend="device")
  for key in KEYS + ("status", "n_views", "n_points", "iterations", "rms"):
    assert np.array_equal(dev[key], again[key], equal_nan=True), key


def test_idle_waves_and_a_pair_that_is_not_launched():
  """pairs of 3 views, 1 view and no view in one call"""
  case = sh.make_case("tiny_mixed", frames=16)
  both = lambda i, j: np.argwhere(case.view_valid[i] & case.view_valid[j] & ((case.valid[i] & case.valid[j]).sum(axis=-1) >= 4))
  keep01 = [tuple(s) for s in both(0, 1)[:3]]
  keep23 = [tuple(s) for s in both(2, 3) if tuple(s) not in keep01][:1]
  view_valid = case.view_valid.copy()
  for c, keep in ((0, keep01), (2, keep23)):
    view_valid[c] = False
    for f, b in keep:
      view_valid[c, f, b] = True
  masked = sh.with_tables(case, view_valid=view_valid)
  pairs = [(0, 1), (2, 3), (0, 2)]
  dev, serial, host = sh.run(masked, pairs, backend="device"), sh.run(masked, pairs), sh.run(masked, pairs, order=True)
  ms, launched = stereo.last_call_ms()
  assert list(dev.n_views) == [3, 1, 0] and list(dev.status) == [stereo.OK, stereo.OK, stereo.TOO_FEW] and launched == 2
  assert_device_equals_host(dev, host, serial, "masks")


def test_a_launched_pair_without_a_finite_cost_is_degenerate():
  """start poses of the left camera that are not finite: the pair is launched, its first cost is not finite -- the loop's own
  DEGENERATE exit -- and it returns what a pair without a result returns, beside a pair that is solved"""
  case = sh.make_case("tiny_mixed", frames=16)
  poses = case.view_poses.copy()
  poses[0] = np.nan
  bad = sh.with_tables(case, view_poses=poses)
  pairs = [(0, 1), (2, 3)]
  dev, serial, host = sh.run(bad, pairs, backend="device"), sh.run(bad, pairs), sh.run(bad, pairs, order=True)
  assert stereo.last_call_ms()[1] == 2
  assert list(dev.status) == [stereo.DEGENERATE, stereo.OK] and dev.iterations[0] == 1 and dev.n_views[0] > 0
  assert np.array_equal(dev.T[0], np.eye(4)) and np.isnan(dev.cov[0]).all() and dev.sse[0] == 0
  assert (dev.view_poses[0] == np.eye(4)).all() and (dev.view_sse[0] == 0).all()
  assert_device_equals_host(dev, host, serial, "not finite")


def test_nothing_to_do_touches_nothing():
  for case in (sh.make_case("tiny_fisheye"), sh.with_tables(sh.make_case("tiny", frames=16),
                                                             view_valid=np.zeros((2, 16, 1), dtype=bool))):
    res = sh.run(case, backend="device")
    ms, launched = stereo.last_call_ms()
    assert (res.status == stereo.TOO_FEW).all() and np.isnan(res.cov).all() and (res.T == np.eye(4)).all()
    assert launched == 0 and ms["upload"] == 0.0 and ms["kernel"] == 0.0 and ms["download"] == 0.0
  none = sh.run(sh.make_case("tiny", frames=16), pairs=np.zeros((0, 2), dtype=np.int32), backend="device")
  assert len(none.status) == 0 and stereo.last_call_ms()[1] == 0


# ---- end to end: the two-camera bundle adjustment is the same cost function ---------------------------------------------------------
def pair_sub_rig(case, i, j):
  """the rig of cameras (i, j) alone, `valid` reduced to the common corners of the pair's views, frames without a view invalid"""
  rig = case.rig
  n = (case.valid[i] & case.valid[j]).sum(axis=-1)
  views = case.view_valid[i] & case.view_valid[j] & (n >= 4)
  common = case.valid[i] & case.valid[j] & views[..., None]
  valid = np.stack([common, common])
  t = rig.truth
  # (the start: the truth cameras, which stay held, and the truth poses)
  src = SimpleNamespace(cameras=[t.cameras[i], t.cameras[j]], camera_poses=t.camera_poses[[i, j]], board_poses=t.board_poses,
                        rig=t.rig, rig_end=None, hand_eye=None)
  return SimpleNamespace(name=rig.name, cfg=rig.cfg, truth=src, init=src, board_points=rig.board_points,
                         points=np.where(valid[..., None], rig.points[[i, j]], 0.0), valid=valid, camera_valid=np.ones(2, dtype=bool),
                         board_valid=rig.board_valid, frame_valid=views.any(axis=1),
                         optimize=dict(cameras=False, boards=False, camera_poses=True, board_poses=False, motion=True))


@pytest.mark.parametrize("name,i,j", [("tiny", 0, 1), ("tiny_mixed", 0, 1), ("tiny_mixed", 1, 3)])
def test_pair_rms_equals_the_two_camera_bundle_adjustment(name, i, j):
  """one-board rigs: with cameras and the board held and camera poses and frame poses free, bundle_adjust over the pair's common
  corners minimises the same function of the same data; its RMS equals the pair's within 1e-9 px, the project's residual-parity
  unit"""
  case, dev, _, _ = solved(name, 16)
  k = int(np.flatnonzero((dev.pairs[:, 0] == i) & (dev.pairs[:, 1] == j))[0])
  calib = calibration.from_rig(pair_sub_rig(case, i, j), which='truth')
  tight = dict(tolerance=1e-15, xtol=1e-15, gtol=1e-15, max_iterations=300, solver="native")
  adjusted = calib.bundle_adjust(**tight)
  err = np.asarray(adjusted.reprojection_error)
  rms = float(np.sqrt(np.mean(np.square(err))))
  print(f"{name} ({i}, {j}): pair rms {dev.rms[k]:.12f} px over {2 * dev.n_points[k]} image points, two-camera bundle adjustment "
        f"{rms:.12f} px over {err.size}")
  assert err.size == 2 * dev.n_points[k]
  assert abs(dev.rms[k] - rms) <= 1e-9


# ---- the diagnostic ------------------------------------------------------------------------------------------------------------
def test_pairwise_extrinsics_points_at_a_displaced_camera():
  """a calibration at its optimum (cameras held at the truth), then camera 1's pose rotated by a planted 5 mrad: the three pairs of
  camera 1 lead the ranking"""
  from scipy.spatial.transform import Rotation
  case = sh.make_case("tiny_mixed", frames=16)
  calib = calibration.from_rig(case.rig, which='truth').enable(cameras=False, boards=False)
  calib = calib.bundle_adjust(tolerance=1e-12, max_iterations=100, solver="native")
  at_optimum = calib.pairwise_extrinsics()
  poses = np.asarray(calib.camera_poses.poses).copy()
  bump = np.eye(4)
  bump[:3, :3] = Rotation.from_rotvec([0.0, 5e-3, 0.0]).as_matrix()
  poses[1] = bump @ poses[1]
  bumped = calib.copy(camera_poses=calib.camera_poses._replace_poses(poses, keep_valid=True))
  r = bumped.report_pairwise_extrinsics("bumped")
  lead = [tuple(int(c) for c in r.pairs[k]) for k in r.ranking[:3]]
  print("at the optimum: scaled", np.round(at_optimum.scaled, 2), "; camera 1 displaced: pairs", [tuple(p) for p in r.pairs], "scaled",
        np.round(r.scaled, 2), "rotation mrad", np.round(r.rotation_mrad, 3), "ranking", list(r.ranking))
  assert len(r.pairs) == 6 and r.enough.all()
  assert all(1 in p for p in lead)
  # the pairs' own estimates do not depend on the rig's camera poses beyond the start of their views: what they report is the
  # planted 5 mrad, to within 3 mrad -- above three of the pairs' own standard deviations (0.4 .. 0.9 mrad at 0.2 px noise with 1 %
  # outliers of up to 50 px in these 16 frames)
  assert np.abs(r.rotation_mrad[[k for k, p in enumerate(r.pairs) if 1 in p]] - 5.0).max() <= 3.0
