"""mcba_reconstruction_uncertainty on the device (k_reconstruction_uncertainty) against the g++ build of the same header
(reconstruction_uncertainty_host_lib), Calibration.reconstruction_uncertainty and triangulate(calibration_cov=True) end to end, and
the entry inside the one resource cache of the handle-less families.  Statuses, n_views and view masks are equal exactly.  The
covariances, in whitened form |L^-1 (C_dev - C_host) L^-T| with L L^T = C_host: within 100 x what contraction alone does -- the
difference between two HOST builds of the header, -ffp-contract=off against -ffp-contract=fast, over the same points (measured here
on the CPU, printed; profiles/reconstruction_uncertainty_parity.txt); a floor of 1e-13 only where those two return the same bytes."""
import numpy as np
import pytest

from multical_amd import _lib, reconstruction, synthetic, uncertainty

import reconstruction_uncertainty_host_lib as rl
import uncertainty_host_lib as ul
from util import mirror

pytestmark = pytest.mark.gpu
mats = reconstruction.covariance_matrices


def volume_points(n, seed=0, G=3):
  """n points in front of the group, the first of them on its axis; every 11th behind it and every 13th far to one side"""
  rng = np.random.default_rng(seed)
  pts = rng.uniform([-0.3, -0.25, 1.0 + 0.15 * G], [0.3, 0.25, 3.0 + 0.15 * G], (n, 3))
  pts[0] = [0.0, 0.0, 2.0]
  pts[10::11, 2] *= -1.0
  pts[12::13, 0] += 2.5
  return pts


def compare(model, jobs, label, sigma2=0.3, margin=0.0):
  dev = rl.run(model, jobs, sigma2, margin, "device")
  host = rl.run(model, jobs, sigma2, margin)
  fast = rl.run(model, jobs, sigma2, margin, "fast")
  for k in ("status", "n_views", "views"):
    assert np.array_equal(dev[k], host[k]) and np.array_equal(fast[k], host[k]), (label, k)
  ok = host.status == reconstruction.OK
  for k in ("cov_cal", "cov_noise"):
    assert np.array_equal(np.isnan(dev[k]), np.isnan(host[k])) and np.isnan(dev[k][~ok]).all(), (label, k)
    if not ok.any():
      continue
    contraction = rl.whitened_difference(mats(fast[k][ok]), mats(host[k][ok])).max()
    got = rl.whitened_difference(mats(dev[k][ok]), mats(host[k][ok])).max()
    same = fast[k].tobytes() == host[k].tobytes()
    print(f"{label} {k}: {int(ok.sum())} of {ok.size} points OK; device - host whitened {got:.3g}, contraction alone (two host builds) "
          f"{contraction:.3g}{' (the same bytes)' if same else ''}")
    assert got <= (1e-13 if same else 100.0 * contraction), (label, k)
  return dev


def job(model, ref, r, n, seed, masks=None):
  return rl.job_of(model, ref, rl.random_factors(model, r, seed)[0], volume_points(n, seed, len(model.cameras)), masks)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 257])
def test_point_counts_at_tile_and_wave_edges(n):
  m, _ = rl.group_rig(3, 3)
  dev = compare(m, [job(m, None if n % 2 else 1, 17, n, n)], f"{n} points")
  assert dev.status[0] == reconstruction.OK and reconstruction.last_call_ms()[1] == n


@pytest.mark.parametrize("r", [0, 1, 15, 16, 17, 33, 128])
def test_factor_widths_at_column_tile_edges(r):
  m, _ = rl.group_rig(5, 3)
  for ref in (None, 2):
    dev = compare(m, [job(m, ref, r, 33, r)], f"r = {r} reference {ref}")
    if r == 0:
      assert (dev.cov_cal[dev.status == reconstruction.OK] == 0).all()


@pytest.mark.parametrize("G", [2, 3, 4, 5, 8])
@pytest.mark.parametrize("ref", [None, "last"], ids=["rig", "camera"])
def test_group_sizes_with_mixed_families(G, ref):
  m, _ = rl.group_rig(G % 9, G)
  dev = compare(m, [job(m, None if ref is None else G - 1, 20, 40, G)], f"G = {G} reference {ref}")
  assert (dev.status == reconstruction.OK).mean() > 0.7 and dev.n_views.max() == G


def test_masks_that_remove_the_first_the_last_and_a_middle_slot():
  m, _ = rl.group_rig(1, 5)
  n = 48
  masks = np.array([0b11110, 0b01111, 0b11011, 0b00001, 0b10001, 0][:6] * 8, dtype=np.uint64)
  dev = compare(m, [job(m, 4, 30, n, 2, masks)], "masked slots")
  assert ((dev.views & ~masks) == 0).all() and (dev.status[3::6] == reconstruction.TOO_FEW).all() and (dev.n_views[5::6] == 0).all()
  assert (dev.status == reconstruction.OK).sum() > 20


def test_two_jobs_of_different_group_and_width_share_a_call():
  """G = 8 with r = 40 over 37 points (its last tile holds 5) and G = 2 with r = 7 over 18: the second job starts on a tile of its
  own, and the call takes the wide stage"""
  big, _ = rl.group_rig(0, 8)
  maps, rng = rl.stored_maps(big), np.random.default_rng(5)
  pair = reconstruction.Job([6, 2], 2, [(maps[c] @ (1e-4 * rng.normal(size=(maps[c].shape[1], 7))), False) for c in (6, 2)],
                            volume_points(18, 6, 2), np.array([3] * 17 + [1], dtype=np.uint64))
  dev = compare(big, [job(big, None, 40, 37, 4), pair], "G = 8 | G = 2")
  assert dev.n_views[:37].max() == 8 and dev.n_views[37:].max() == 2 and dev.status[-1] == reconstruction.TOO_FEW
  alone = rl.run(big, [pair], 0.3, 0.0, "device")
  assert all(alone[k].tobytes() == dev[k][37:].tobytes() for k in ("cov_cal", "cov_noise", "n_views", "views", "status"))


def test_a_call_whose_points_all_fail():
  m, _ = rl.group_rig(3, 3)
  pts = np.tile([[0.0, 0.0, -2.0]], (70, 1))
  dev = compare(m, [rl.job_of(m, None, rl.random_factors(m, 9, 1)[0], pts), rl.job_of(m, 1, rl.random_factors(m, 9, 1)[0], pts[:3] + [5.0, 0, 4.0])],
                "behind | to one side")
  assert (dev.status == reconstruction.TOO_FEW).all() and np.isnan(dev.cov_cal).all() and np.isnan(dev.cov_noise).all()


def test_layout_a_single_column_and_points_that_differ_pairwise():
  """W has one non-zero column (in the first and in the second column tile in turn): cov_cal = z z^T of that column alone, and a
  transposed or permuted MFMA tile would hand a point the z of another point (or nothing).  Every point against the host's value
  for THAT point; the points' values differ pairwise by far more than the tolerance."""
  m, _ = rl.group_rig(2, 4)
  pts = volume_points(16, 9, 4)
  pts[10], pts[12] = [0.1, 0.2, 1.7], [-0.2, 0.1, 2.6]        # (all 16 in front: one full tile)
  for column, r in ((5, 16), (19, 33)):
    factors = []
    for W, loose in rl.random_factors(m, r, 3, scale=1e-3)[0]:
      one = np.zeros_like(W)
      one[:, column] = W[:, column]
      factors.append((one, loose))
    for ref in (None, 1):
      dev = rl.run(m, [rl.job_of(m, ref, factors, pts)], 1.0, 0.0, "device")
      host = rl.run(m, [rl.job_of(m, ref, factors, pts)], 1.0, 0.0)
      assert (host.status == reconstruction.OK).all() and np.array_equal(dev.status, host.status)
      scale = np.abs(host.cov_cal).max(axis=1)
      assert (np.abs(dev.cov_cal - host.cov_cal).max(axis=1) <= 1e-9 * scale).all(), (column, ref)
      apart = np.abs(host.cov_cal[:, None] - host.cov_cal[None]).max(axis=2) / np.maximum(scale[:, None], scale[None])
      assert apart[~np.eye(16, dtype=bool)].min() > 1e-3, (column, ref)


def test_range_grows_with_the_square_of_the_distance_and_lateral_with_the_distance():
  m, factors, pts, ref = rl.meaning_case()
  out = rl.run(m, [rl.job_of(m, ref, factors, pts)], backend="device")
  assert (out.status == reconstruction.OK).all()
  rng, lat = rl.range_lateral(m, ref, out, pts)
  print(f"range_std {rng}, ratio {rng[1] / rng[0]:.3f}; lateral_std {lat}, ratio {lat[1] / lat[0]:.3f}")
  assert rng[1] > 3.0 * rng[0] and lat[1] < 3.0 * lat[0]


# ---- one cache, the same bytes ---------------------------------------------------------------------------------------------
def test_repeatable_and_between_two_calls_of_another_entry_point():
  m, _ = rl.group_rig(4, 5)
  jobs = [job(m, 2, 50, 100, 7), job(m, None, 9, 20, 8)]

  def own():
    out = rl.run(m, jobs, 0.3, 0.0, "device")
    return b"".join(out[k].tobytes() for k in ("cov_cal", "cov_noise", "n_views", "views", "status"))

  other_jobs = [uncertainty.Job(5, 0, 2.0, ul.random_spd(ul.rig().stored_count(5, 0), 7), pixels=ul.edge_pixels())]

  def other():
    return b"".join(a.tobytes() for a in ul.run(ul.rig(), other_jobs, "device"))

  first = own()
  assert own() == first and reconstruction.last_call_ms()[1] == 120
  before = other()
  assert own() == first
  assert other() == before and _lib.call_ms("reconstruction_uncertainty", range(4))[1] == 120
  with pytest.raises(RuntimeError) as e:
    rl.run(m, [reconstruction.Job([0, 1, 0], None, rl.random_factors(m, 3, 1)[0][:3], volume_points(4))], 0.3, 0.0, "device")
  message = "mcba_reconstruction_uncertainty: job 0: cameras[2] = 0 is repeated"
  assert message in str(e.value) and message in _lib.load().mcba_last_error().decode()
  assert own() == first


# ---- end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reference", [None, 1], ids=["rig", "camera"])
def test_calibration_reconstruction_uncertainty(reference):
  """on the tiny golden rig: the grid form, against a direct call on the same points through the g++ build of the header with the
  factors of the same covariance"""
  from multical_amd import guidance
  c = mirror(synthetic.make_rig("tiny")).enable(cameras=True)
  got = c.reconstruction_uncertainty(reference=reference, grid=(5, 4))
  D = len(got.distances)
  assert D == 5 and got.cov_cal.shape == (D, 4, 5, 3, 3) and got.status.shape == (D, 4, 5) and got.sigma2 == c.covariance().sigma2
  ok = got.status == reconstruction.OK
  assert ok.any() and np.isnan(got.cov_cal[~ok]).all()
  assert (got.range_std_cal[ok] > 0).all() and (got.range_std_noise[ok] > 0).all() and (got.lateral_std_cal[ok] > 0).all()
  assert np.array_equal(got.cov_total[ok], got.cov_cal[ok] + got.cov_noise[ok])
  lam = np.linalg.eigvalsh(got.cov_cal[ok])
  assert (lam[:, 0] >= -1e-12 * lam[:, 2]).all()
  model = uncertainty.RigModel(list(c.cameras), np.asarray(c.camera_poses.poses), np.asarray(c.camera_poses.params).reshape(-1, 6))
  camera_index, pose_index = c._shared_layout()
  factors, r = guidance.rig_factors(model, c.covariance(), camera_index, pose_index)
  assert r == got.r
  host = rl.run(model, [rl.job_of(model, reference, factors, got.points.reshape(-1, 3))], sigma2=got.sigma2)
  assert np.array_equal(host.status, got.status.ravel())
  worst = rl.whitened_difference(got.cov_cal.reshape(-1, 3, 3)[ok.ravel()], mats(host.cov_cal)[ok.ravel()]).max()
  print(f"tiny reference {reference}: r = {r}, {int(ok.sum())} of {ok.size} cells OK, device - host whitened {worst:.3g}; median range std "
        f"calibration {np.nanmedian(got.range_std_cal):.3g} noise {np.nanmedian(got.range_std_noise):.3g}")
  assert worst <= 1e-9
  as_list = c.reconstruction_uncertainty(reference=reference, points=got.points.reshape(-1, 3))
  assert as_list.cov_cal.tobytes() == got.cov_cal.tobytes() and as_list.status.tobytes() == got.status.tobytes()


def test_the_report_runs_and_boards_are_refused():
  import logging
  c = mirror(synthetic.make_rig("tiny")).enable(cameras=True)
  records = []
  handler = logging.Handler()
  handler.emit = records.append
  logging.getLogger("calibration").addHandler(handler)
  try:
    logging.getLogger("calibration").setLevel(logging.INFO)
    c.report_reconstruction_uncertainty("test", reference=0)
  finally:
    logging.getLogger("calibration").removeHandler(handler)
  lines = [r.getMessage() for r in records if "range" in r.getMessage()]
  print("\\n".join(lines))
  assert len(lines) == c.size.cameras - 1 and any("calibration/noise" in l for l in lines), lines
  with pytest.raises(ValueError, match="boards"):
    c.enable(boards=True).reconstruction_uncertainty()


def test_triangulate_with_the_calibration_covariance():
  """cov_cal of triangulate(calibration_cov=True) is a direct call on the same points and views, turned into the frame of `cov`; every
  other field is byte-identical with and without the flag"""
  c = mirror(synthetic.make_rig("tiny")).enable(cameras=True)
  plain, with_cal = c.triangulate(), c.triangulate(calibration_cov=True)
  assert set(with_cal.keys()) == set(plain.keys()) | {"cov_cal"}
  for k in plain.keys():
    assert np.asarray(plain[k]).tobytes() == np.asarray(with_cal[k]).tobytes(), k
  assert with_cal.cov_cal.shape == plain.cov.shape and with_cal.valid.any()
  assert np.isnan(with_cal.cov_cal[~with_cal.valid]).all()
  f, b, p = np.nonzero(with_cal.valid)
  start, _ = c._rig_poses()
  R, t = start[f, :3, :3], start[f, :3, 3]
  X = np.einsum("nij,nj->ni", R, with_cal.points[f, b, p]) + t
  Cn = c.size.cameras
  view_valid = np.asarray(c.camera_poses.valid)[:, None] & np.asarray(c.motion.valid)[None, :]
  offered = c.inliers & view_valid[:, :, None, None]
  masks = (offered[:, f, b, p].astype(np.uint64) << np.arange(Cn, dtype=np.uint64)[:, None]).sum(axis=0).astype(np.uint64)
  direct = c._reconstruction_uncertainty(c.covariance(), None, None, X, masks, margin=1e9)
  want = np.einsum("nji,njk,nkl->nil", R, direct.cov_cal, R)
  assert np.allclose(want, with_cal.cov_cal[f, b, p], rtol=1e-9, atol=0.0, equal_nan=True)
  ok = direct.status == reconstruction.OK
  assert ok.mean() > 0.9 and (direct.n_views[ok] == with_cal.n_views[f, b, p][ok]).all()
  lam = np.linalg.eigvalsh(with_cal.cov_cal[f, b, p][ok])
  assert (lam[:, 2] > 0).all() and (lam[:, 0] >= -1e-12 * lam[:, 2]).all()
