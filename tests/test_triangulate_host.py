"""The triangulation mathematics (csrc/mcba_triangulate.h) in its g++ build, against an independent numpy restatement with a
central-difference Jacobian (triangulate_reference.py), and the Python layer on top of it (multical_amd.triangulate,
Calibration.triangulate / reconstruction_error) driven through that build.  No GPU."""
import functools
import logging

import numpy as np
import pytest

from multical_amd import triangulate

import host_build
import triangulate_host_lib as th
import triangulate_reference as tr
import undistort_host_lib as uh
import undistort_reference as ref

SHAPES = list(range(len(th.SHAPES)))
SIGMA = th.NOISE_PX


@functools.lru_cache(maxsize=None)
def solved(i):
  """shape i once for every test: the rig, the host build's result (known sigma), the restatement's normal equations at the returned
  points and its own optimum from two starts"""
  C, F, M, rolling = th.SHAPES[i]
  rig = th.make_rig(C, F, M, rolling)
  got = th.run(rig, sigma=SIGMA)
  prob = th.reference_problem(rig)
  ok = (got.status == triangulate.OK).ravel()
  X = got.points.reshape(-1, 3)
  H, g, sse, r = prob.normal_equations(np.where(ok[:, None], X, 0.0))
  start, solvable = prob.linear_start()
  a = prob.refine(start)
  b = prob.refine(start + np.random.default_rng(5).normal(0.0, 1e-3, start.shape))
  return th.SimpleNamespace(rig=rig, got=got, prob=prob, ok=ok, X=X, H=H, g=g, sse=sse, r=r, optimum=a, second=b, solvable=solvable)


@pytest.mark.parametrize("i", SHAPES, ids=th.SHAPE_IDS)
def test_status_and_cap(i):
  """every point two cameras or more saw converges from the linear start within the default 20 linearisations (cap: 0 left out);
  every other point is TOO_FEW, with NaN, no covariance and zeros"""
  s = solved(i)
  n = s.rig.valid.sum(axis=0)
  assert np.array_equal(s.got.n_views, n) and np.array_equal(s.prob.n_views.reshape(n.shape), n)
  assert (n >= 2).sum() > 40
  print(f"{th.SHAPE_IDS[i]}: {(n >= 2).sum()} points seen twice, {(n < 2).sum()} not; statuses {np.bincount(s.got.status.ravel(), minlength=5)}")
  assert (s.got.status[n >= 2] == triangulate.OK).all()
  assert (s.got.status[n < 2] == triangulate.TOO_FEW).all()
  none = n < 2
  assert np.isnan(s.got.points[none]).all() and np.isnan(s.got.cov[none]).all() and (s.got.sse[none] == 0).all()
  assert (s.got.error[:, none] == 0).all() and np.isfinite(s.got.points[~none]).all() and np.isfinite(s.got.cov[~none]).all()
  assert (s.got.error[~s.rig.valid] == 0).all() and (s.got.error[s.rig.valid & ~none[None]] > 0).all()
  assert np.array_equal(s.solvable, (n >= 2).ravel())


@pytest.mark.parametrize("i", SHAPES, ids=th.SHAPE_IDS)
def test_every_ok_point_is_stationary(i):
  """|L^-1 g| <= 1e-8 px with H = L L^T and g of the restatement at the returned point: 40 x the 2.5e-10 px that the restatement's
  central differences leave at its own optimum with a step of 1e-6 m (1e-11 px with the 1e-5 m it uses)"""
  s = solved(i)
  w = tr.whitened_gradient(s.H[s.ok], s.g[s.ok])
  own = tr.whitened_gradient(*s.prob.subset(np.nonzero(s.ok)[0]).normal_equations(s.optimum[s.ok])[:2])
  print(f"{th.SHAPE_IDS[i]}: whitened gradient at the returned points {w.max():.2e} px, at the restatement's own optimum {own.max():.2e} px, "
        f"cond(H) {np.linalg.cond(s.H[s.ok]).max():.1e}")
  assert w.max() <= 1e-8


@pytest.mark.parametrize("i", SHAPES, ids=th.SHAPE_IDS)
def test_distance_to_the_restatements_optimum(i):
  s = solved(i)
  spread = tr.whitened_norm(s.H[s.ok], (s.optimum - s.second)[s.ok]).max()
  dist = tr.whitened_norm(s.H[s.ok], (s.X - s.optimum)[s.ok]).max()
  print(f"{th.SHAPE_IDS[i]}: whitened distance to the restatement's optimum {dist:.2e} px; its spread between two starts {spread:.2e} px")
  assert dist <= max(1e-9, 100.0 * spread)


@pytest.mark.parametrize("i", SHAPES, ids=th.SHAPE_IDS)
def test_covariance_and_errors(i):
  s = solved(i)
  ok2 = s.ok.reshape(s.got.status.shape)
  inv = np.linalg.inv(s.H[s.ok])
  cov = s.got.cov.reshape(-1, 3, 3)[s.ok]
  scale = np.abs(inv).max(axis=(1, 2))

  def relative(c, sigma2):
    return (np.abs(c - sigma2[:, None, None] * inv).max(axis=(1, 2)) / (sigma2 * scale)).max()
  assert np.array_equal(cov, np.swapaxes(cov, 1, 2))
  known = relative(cov, np.full(len(inv), SIGMA ** 2))
  sse = s.got.sse.ravel()[s.ok]
  err = np.moveaxis(s.got.error, 0, 2).reshape(-1, s.prob.C)[s.ok]
  want_err = np.linalg.norm(s.r[s.ok], axis=-1)
  d_sse, d_err = np.abs(sse - s.sse[s.ok]).max(), np.abs(err - want_err).max()
  # the automatic sigma: the point's own sse / (2 n - 3), everything else unchanged
  auto = th.run(s.rig)
  assert np.array_equal(auto.points[ok2], s.got.points[ok2]) and np.array_equal(auto.sse, s.got.sse) and np.array_equal(auto.status, s.got.status)
  n = s.got.n_views.ravel()[s.ok]
  sigma2 = sse / (2 * n - 3)
  ratio = auto.cov.reshape(-1, 3, 3)[s.ok] / cov
  own = np.abs(ratio * SIGMA ** 2 / sigma2[:, None, None] - 1.0).max()
  automatic = relative(auto.cov.reshape(-1, 3, 3)[s.ok], sigma2)
  print(f"{th.SHAPE_IDS[i]}: cov vs sigma^2 inv(H) {known:.2e} (known sigma) {automatic:.2e} (automatic) relative; sse {d_sse:.2e} px^2, "
        f"err {d_err:.2e} px; cov_auto / cov_known vs sse / (2n - 3) / sigma^2: {own:.2e}")
  assert known <= 1e-6 and automatic <= 1e-6 and own <= 1e-12
  assert d_sse <= 1e-9 and d_err <= 1e-9


@pytest.mark.parametrize("i", SHAPES, ids=th.SHAPE_IDS)
def test_noise_free_observations_give_the_truth(i):
  rig = solved(i).rig
  got = th.run(rig, points=rig.clean)
  n = rig.valid.sum(axis=0)
  assert (got.status[n >= 2] == triangulate.OK).all() and (got.status[n < 2] == triangulate.TOO_FEW).all()
  d = np.linalg.norm(got.points - rig.truth, axis=-1)[n >= 2]
  print(f"{th.SHAPE_IDS[i]}: |X - truth| <= {d.max():.2e} m, sse <= {got.sse.max():.2e} px^2")
  assert d.max() <= 1e-9


# ---- planted cases -------------------------------------------------------------------------------------------------------------
def planted(cameras, views, X):
  """one frame of points X [M, 3] seen by every camera, noise-free: (views [C,1,3,4], points [C,1,M,2], valid)"""
  views = np.asarray(views, dtype=np.float64)[:, None]
  pts = np.stack([ref.project(cam, X @ v[0, :, :3].T + v[0, :, 3]) for cam, v in zip(cameras, views)])[:, None]
  return views, pts, np.ones(pts.shape[:3], dtype=bool)


POINTS = np.array([[0.05, -0.03, 1.2], [-0.1, 0.06, 1.6], [0.0, 0.0, 0.9]])


def test_identical_views_are_degenerate():
  rig = th.make_rig(2, 1, 65)
  views, pts, valid = planted(rig.cameras, [rig.views[0, 0], rig.views[0, 0]], POINTS)
  got = th.on_host(triangulate.triangulate, rig.cameras, views, pts, valid)
  assert (got.status == triangulate.DEGENERATE).all() and (got.n_views == 2).all()
  assert np.isnan(got.points).all() and np.isnan(got.cov).all() and (got.sse == 0).all() and (got.error == 0).all()


def test_a_pixel_outside_the_model_drops_its_view():
  cams = uh.fixture_cameras()
  rig = th.make_rig(3, 3, 65)
  cameras = [cams[0], cams[5], cams[1]]                       # 5 coefficients, Kannala-Brandt, 4 coefficients
  assert ref.is_fisheye(cameras[1])
  views, pts, valid = planted(cameras, rig.views[:, 0], POINTS)
  pts[1] = [5000.0, 4000.0]                                   # a fisheye camera cannot have produced this pixel
  two = th.on_host(triangulate.triangulate, cameras[:2], views[:2], pts[:2], valid[:2])
  assert (two.status == triangulate.TOO_FEW).all() and (two.n_views == 1).all() and np.isnan(two.points).all()
  three = th.on_host(triangulate.triangulate, cameras, views, pts, valid)
  assert (three.status == triangulate.OK).all() and (three.n_views == 2).all()
  assert np.abs(three.points[0] - POINTS).max() <= 1e-9 and (three.error[1] == 0).all()
  pts[1, 0, 0] = [np.nan, 10.0]                               # not finite: dropped as well
  assert (th.on_host(triangulate.triangulate, cameras, views, pts, valid).n_views == 2).all()


def test_a_point_behind_the_cameras_is_flagged_and_returned():
  rig = th.make_rig(2, 1, 65)                                 # 5 and 4 Brown-Conrady coefficients
  X = POINTS * [1.0, 1.0, -1.0]
  views, pts, valid = planted(rig.cameras, rig.views[:, 0], X)
  assert ((X @ views[:, 0, 2, :3].T + views[:, 0, 2, 3]) < 0).all()
  got = th.on_host(triangulate.triangulate, rig.cameras, views, pts, valid)
  assert (got.status == triangulate.BEHIND).all()
  assert np.abs(got.points[0] - X).max() <= 1e-9 and np.isfinite(got.cov).all()


def test_one_linearisation_does_not_converge():
  rig = th.make_rig(3, 3, 65)
  got = th.run(rig, max_iterations=1)
  n = rig.valid.sum(axis=0)
  assert (got.status[n >= 2] == triangulate.NOT_CONVERGED).all() and (got.status[n < 2] == triangulate.TOO_FEW).all()
  start = th.reference_problem(rig).linear_start()[0].reshape(got.points.shape)      # the last iterate is the linear start
  assert np.abs(got.points - start)[n >= 2].max() <= 1e-9 and np.isfinite(got.cov[n >= 2]).all()
  # the cap is clamped to 100, 0 and below mean the default
  assert np.array_equal(th.run(rig, max_iterations=10 ** 6).points, th.run(rig, max_iterations=0).points, equal_nan=True)


def test_view_valid_masks_a_view():
  rig = th.make_rig(3, 3, 65)
  view_valid = np.ones((3, 3), dtype=bool)
  view_valid[2, 1] = view_valid[0, 2] = False
  got = th.run(rig, view_valid=view_valid)
  masked = rig.valid & view_valid[:, :, None]
  want = th.on_host(triangulate.triangulate, rig.cameras, rig.views, rig.points, masked)
  assert np.array_equal(got.n_views, masked.sum(axis=0)) and not np.array_equal(got.n_views, rig.valid.sum(axis=0))
  for k in ("points", "cov", "sse", "error", "status"):
    assert np.array_equal(got[k], want[k], equal_nan=True), k


def test_refused_calls_and_empty_tables():
  rig = th.make_rig(2, 1, 65)
  fn = th.lib().th_triangulate
  p, out, keep = th.raw_problem(rig, n_cameras=triangulate.MAX_CAMERAS + 1)
  assert th.raw_call(fn, p, out) == 1 and b"at most 64" in th.lib().th_last_error()
  p, out, keep = th.raw_problem(rig)
  p.views = None
  assert th.raw_call(fn, p, out) == 1 and b"null argument" in th.lib().th_last_error()
  p, out, keep = th.raw_problem(rig)
  p.views_end = p.views
  assert th.raw_call(fn, p, out) == 1 and b"image_heights" in th.lib().th_last_error()
  empty = th.on_host(triangulate.triangulate, rig.cameras, rig.views, np.zeros((2, 1, 0, 2)), np.zeros((2, 1, 0), dtype=bool))
  assert empty.points.shape == (1, 0, 3) and empty.cov.shape == (1, 0, 3, 3) and empty.error.shape == (2, 1, 0)
  # a [C, F, 4, 4] table of whole poses serves as views; triangulate_rig builds them
  whole = triangulate.rig_views(rig.camera_poses, rig.rig_poses)
  assert np.array_equal(whole, rig.views)
  a = th.on_host(triangulate.triangulate_rig, rig.cameras, rig.camera_poses, rig.rig_poses, rig.points, rig.valid)
  assert np.array_equal(a.points, th.run(rig).points, equal_nan=True)


def test_sanitized_stand_alone_run(tmp_path):
  """the host build inside a small program of its own under AddressSanitizer + UBSan (CPU only): exact-size heap tables, pixels that
  are not finite or far outside every model, masked views, optional outputs left out -- no observation is read and no error stored
  out of bounds"""
  r = host_build.sanitized_program("triangulate_host", "triangulate_sanitize_main.cpp", tmp_path)
  assert r.returncode == 0 and "triangulate sanitize run: ok" in r.stdout, r.stdout + r.stderr


# ---- Calibration.triangulate / reconstruction_error ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,twice,once", [("tiny", 119, 240), ("tiny_rolling", None, None)])
def test_reconstruction_error_at_the_truth(name, twice, once):
  """noise-free detections at the truth parameters: every corner two cameras saw comes back within 1e-9 m of where the rig chain
  puts it (the rolling fixture through its rolling chain); every other slot is invalid"""
  calib = th.truth_calibration(name)
  seen = calib.valid.sum(axis=0)
  if twice is not None:
    assert ((seen >= 2).sum(), (seen == 1).sum()) == (twice, once)
  with th.host_backend():
    t = calib.triangulate()
    r = calib.reconstruction_error()
  assert (seen >= 2).sum() > 50 and np.array_equal(t.valid, seen >= 2) and np.array_equal(r.valid, seen >= 2)
  assert t.points.shape == seen.shape + (3,) and t.cov.shape == seen.shape + (3, 3) and np.array_equal(t.n_views, seen)
  print(f"{name}: {int(r.valid.sum())} corners seen twice, largest distance {r.error.max():.2e} m")
  assert r.error[r.valid].max() <= 1e-9 and (r.error[~r.valid] == 0).all() and np.isnan(t.points[~t.valid]).all()
  assert r.overall.n == r.valid.sum() and len(r.boards) == calib.size.boards and sum(b.n for b in r.boards if b.rms > 0) == r.overall.n
  if name == "tiny_rolling":
    # its static start is NOT the chain that made the detections
    from multical_amd.motion import StaticFrames
    from multical_amd.structs import Table
    static = calib.copy(motion=StaticFrames(Table.create(poses=calib.motion.pose_start, valid=calib.motion.valid)))
    with th.host_backend():
      assert static.reconstruction_error().error.max() > 1e-6


def test_reconstruction_error_of_the_golden_detections(caplog):
  """the golden noisy detections of `tiny` at the truth parameters: a median below 2 mm (scipy.least_squares per point: 0.55 mm)"""
  calib = th.truth_calibration("tiny", noise_free=False)
  with th.host_backend(), caplog.at_level(logging.INFO, logger="calibration"):
    r = calib.reconstruction_error()
    calib.report_reconstruction("golden:")
  q = r.overall.quantiles
  print(f"tiny: n={r.overall.n} rms={1e3 * r.overall.rms:.3f} mm median={1e3 * q[2]:.3f} mm max={1e3 * q[4]:.3f} mm")
  assert r.overall.n > 100 and q[2] < 2e-3
  assert any("reconstruction RMS=" in m and "mm" in m and "corners seen by >= 2 cameras" in m for m in caplog.messages)
