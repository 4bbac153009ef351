"""mcba_projection_uncertainty on the device (k_projection_uncertainty) against the g++ build of the same header
(uncertainty_host_lib), Calibration.projection_uncertainty end to end, and the entry inside the one resource cache of the handle-less
families.  Device against host build, in whitened form |L^-1 (C_dev - C_host) L^-T| with L L^T = C_host: within 100 x what
contraction alone does -- the difference between two HOST builds of the header, -ffp-contract=off against -ffp-contract=fast, over
the same queries (measured here on the CPU, printed; profiles/projection_uncertainty_parity.txt)."""
import numpy as np
import pytest

from multical_amd import _lib, synthetic, tables, uncertainty

import pnp_host_lib as L
import uncertainty_host_lib as ul
from util import mirror

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def spread_pixels(n, seed=0):
  """n pixels over the image, the nine edge pixels first"""
  rng = np.random.default_rng(seed)
  px = np.concatenate([ul.edge_pixels(), rng.uniform([0, 0], [ul.W_IMG - 1, ul.H_IMG - 1], (max(n, 9), 2))])
  return np.ascontiguousarray(px[:n])


def compare(jobs, label, model=None):
  model = ul.rig() if model is None else model
  dev = ul.run(model, jobs, "device")
  host = ul.run(model, jobs)
  fast = ul.run(model, jobs, "fast")
  assert np.array_equal(dev[2], host[2]) and np.array_equal(fast[2], host[2]), label
  ok = host[2] == uncertainty.OK
  assert np.array_equal(np.isnan(dev[0]), np.isnan(host[0])) and np.isnan(dev[0][~ok]).all() and np.isnan(dev[1][~ok]).all(), label
  if not ok.any():
    return dev
  contraction = ul.whitened_difference(fast[0][ok], host[0][ok]).max()
  got = ul.whitened_difference(dev[0][ok], host[0][ok]).max()
  print(f"{label}: {int(ok.sum())} of {ok.size} queries OK; device - host whitened {got:.3g}, contraction alone (two host builds) "
        f"{contraction:.3g}")
  assert got <= 100.0 * contraction, label
  uu, uv, vv = dev[0][ok, 0], dev[0][ok, 1], dev[0][ok, 2]
  hs, hd = 0.5 * (uu + vv), 0.5 * (uu - vv)
  assert np.sqrt(np.maximum(hs + np.sqrt(hd * hd + uv * uv), 0.0)).tobytes() == dev[1][ok].tobytes(), label
  return dev


def job_of(b, a, distance, seed, **where):
  return uncertainty.Job(b, a, distance, ul.random_spd(ul.rig().stored_count(b, a), seed), **where)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_lists_at_lane_wave_and_workgroup_edges(n):
  compare([job_of(5, 0, 2.0, n, pixels=spread_pixels(n, n))], f"list of {n}")


@pytest.mark.parametrize("grid", [(1, 1), (1, 65), (17, 5)], ids=["1x1", "1x65", "17x5"])
def test_grids(grid):
  jobs = [job_of(3, None, 2.0, 1, grid=uncertainty.grid_of(ul.uh.IMAGE_SIZE, grid)),
          job_of(6, 7, np.inf, 2, grid=uncertainty.grid_of(ul.uh.IMAGE_SIZE, grid))]
  dev = compare(jobs, f"grid {grid}")
  as_list = [uncertainty.Job(j.camera, j.reference, np.inf if j.rho == 0 else 1.0 / j.rho, j.sigma, pixels=j.pixel_array()) for j in jobs]
  again = ul.run(ul.rig(), as_list, "device")
  assert all(x.tobytes() == y.tobytes() for x, y in zip(dev, again))


def test_two_jobs_of_different_width_share_a_call():
  """14 + 6 columns (the tilted camera against the rig frame) and 4 + 4 + 12 (pinhole-4 -> fisheye): 257 queries of the first end
  inside a tile, the second job starts on the next"""
  compare([job_of(4, None, 1.5, 3, pixels=spread_pixels(257, 3)), job_of(1, 5, 1.5, 4, pixels=spread_pixels(65, 4))], "K = 24 and K = 28")


def test_every_family_both_modes_near_and_at_infinity():
  jobs = []
  for b in range(9):
    for a in (None, b - 1 if b > 0 else 1):
      for distance in (np.inf, 0.5):
        jobs.append(job_of(b, a, distance, 10 + b, pixels=ul.edge_pixels()))
  dev = compare(jobs, "9 cameras x 2 modes x 2 distances")
  assert (dev[2] == uncertainty.OK).mean() > 0.9


def test_a_call_whose_queries_all_fail_and_repeatability():
  far = np.tile([[5000.0, 4000.0]], (70, 1))
  dev = compare([job_of(5, None, 1.0, 1, pixels=far), job_of(4, 5, 1.0, 2, pixels=far)], "outside the fisheye model")
  assert (dev[2] == uncertainty.NOT_CONVERGED).all()
  jobs = [job_of(2, 3, 0.7, 5, pixels=spread_pixels(300, 5)), job_of(8, None, 0.7, 6, grid=uncertainty.grid_of(ul.uh.IMAGE_SIZE, (16, 12)))]
  one, two = ul.run(ul.rig(), jobs, "device"), ul.run(ul.rig(), jobs, "device")
  assert all(x.tobytes() == y.tobytes() for x, y in zip(one, two))
  assert uncertainty.last_call_ms()[1] == 300 + 16 * 12


# ---- end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "tiny_fisheye", "tiny_rolling"])
@pytest.mark.parametrize("reference", [None, 1], ids=["rig", "transfer"])
def test_calibration_projection_uncertainty(name, reference):
  """Calibration.projection_uncertainty against J Sigma J^T in np.longdouble: Sigma the sub-block of the same calib.covariance(), J
  the header's row pair in its g++ build taken to the stored parameters (pinned to the numpy restatement's differences by
  test_projection_uncertainty_host.py); |dC| <= 1000 eps |J|_F^2 |Sigma|_2 as there"""
  c = mirror(synthetic.make_rig(name)).enable(cameras=True)
  cov = c.covariance()
  got = c.projection_uncertainty(reference=reference, distance=1.5, grid=(5, 4))
  assert got.cov.shape == (c.size.cameras, 4, 5, 2, 2) and got.sigma2 == cov.sigma2
  camera_index, pose_index = c._shared_layout()
  model = uncertainty.RigModel(list(c.cameras), np.asarray(c.camera_poses.poses), np.asarray(c.camera_poses.params).reshape(-1, 6))
  worst = 0.0
  for b in range(c.size.cameras):
    idx = [camera_index[b], pose_index[b]] + ([pose_index[reference], camera_index[reference]] if reference is not None else [])
    sigma, loose = uncertainty.stored_covariance(cov, np.concatenate(idx))
    J, status = ul.query_rows(model, b, reference, 1.0 / 1.5, got.pixels[b].reshape(-1, 2))
    assert (J[:, :, loose] == 0).all()              # (the skew: no residual depends on it, and neither does this prediction)
    assert np.array_equal(status, got.status[b].ravel())
    for i in np.flatnonzero(status == uncertainty.OK):
      Jl, Sl = J[i].astype(np.longdouble), sigma.astype(np.longdouble)
      want = (Jl @ Sl @ Jl.T).astype(np.float64)
      bound = 1000.0 * EPS * np.linalg.norm(J[i]) ** 2 * np.linalg.norm(sigma, 2)
      diff = np.abs(got.cov[b].reshape(-1, 2, 2)[i] - want).max()
      worst = max(worst, diff / bound)
      assert diff <= bound, (name, b, i, diff, bound)
    if reference == b:
      assert (got.cov[b] == 0).all()
  assert (got.status == uncertainty.OK).any()       # (the fisheye rig is a ring: most of what one camera sees lies behind the next)
  print(f"{name} reference {reference}: worst |dC| / bound {worst:.3g}; median std {np.nanmedian(got.std):.4f} px")


def test_held_camera_without_intrinsics_is_exactly_zero_and_the_report_runs():
  import logging
  c = mirror(synthetic.make_rig("tiny")).enable(cameras=False)
  got = c.projection_uncertainty(distance=2.0)
  assert got.std.shape == (c.size.cameras, 12, 16)
  assert (got.cov[0] == 0).all() and (got.std[0] == 0).all() and (got.status[0] == uncertainty.OK).all()
  assert (got.std[1:][got.status[1:] == uncertainty.OK] > 0).all()
  records = []
  handler = logging.Handler()
  handler.emit = records.append
  logging.getLogger("calibration").addHandler(handler)
  try:
    logging.getLogger("calibration").setLevel(logging.INFO)
    c.enable(cameras=True).report_projection_uncertainty("test", reference=0, distance=2.0)
  finally:
    logging.getLogger("calibration").removeHandler(handler)
  lines = [r.getMessage() for r in records if "projected std" in r.getMessage()]
  assert len(lines) == c.size.cameras and all("median=" in l and "below sigma" in l for l in lines), lines
  with pytest.raises(ValueError, match="boards"):
    c.enable(boards=True).projection_uncertainty()


# ---- one cache ------------------------------------------------------------------------------------------------------------
def test_between_two_calls_of_another_family():
  rig = L.golden_rig("tiny")

  def view_poses():
    out = tables.view_poses(rig.points, rig.valid, rig.board_points, rig.truth.cameras)
    return b"".join(np.ascontiguousarray(a).tobytes() for a in out), _lib.call_ms("view_poses", range(4))[1]

  jobs = [job_of(5, 0, 2.0, 7, pixels=spread_pixels(65, 7)), job_of(2, None, 2.0, 8, grid=uncertainty.grid_of(ul.uh.IMAGE_SIZE, (3, 2)))]

  def own():
    return b"".join(a.tobytes() for a in ul.run(ul.rig(), jobs, "device"))

  before = view_poses()
  first = own()
  assert uncertainty.last_call_ms()[1] == 71
  after = view_poses()
  assert before == after and _lib.call_ms("projection_uncertainty", range(4))[1] == 71
  assert own() == first
  with pytest.raises(RuntimeError) as e:
    ul.run(ul.rig(), [job_of(5, 0, -2.0, 7, pixels=spread_pixels(65, 7))], "device")
  message = "mcba_projection_uncertainty: job 0: inv_distance must be finite and >= 0"
  assert message in str(e.value) and message in _lib.load().mcba_last_error().decode()
  assert own() == first and view_poses() == before
