"""mcba_projection_diff on the device (k_projdiff_fit, k_projdiff_map) against the g++ build of the same header (projdiff_host_lib),
Calibration.projection_diff end to end, and the entry inside the one resource cache of the handle-less families.  Statuses, n_fit and
fit statuses are equal; diff and landing agree within 1e-8 px (the bound tests/test_gpu_localize.py uses for the same stop rule: both
fits stop at a step of 1e-10 px, neither at the same one).  The fitted transforms are compared as the largest pixel displacement they
cause over the fit pixels, <= 1e-8 px: the fit jobs below carry their fit pixels as a second job's queries, so that displacement is
the difference of the two maps there.  Iteration counts are printed.  Measured: profiles/projection_diff_parity.txt."""
import logging

import numpy as np
import pytest

from multical_amd import _lib, calibration, compare, export, import_calib, synthetic, tables, uncertainty

import pnp_host_lib as L
import projdiff_host_lib as pl
from util import mirror

pytestmark = pytest.mark.gpu
BOUND = 1e-8
NAN_PIXEL = [np.nan, 10.0]


def compare_runs(jobs, label, pair=None):
  dev, host = pl.run(jobs, "device", pair), pl.run(jobs, None, pair)
  assert np.array_equal(dev.status, host.status), label
  assert np.array_equal(dev.fit_info[:, [0, 4]], host.fit_info[:, [0, 4]]), label
  for k in ("diff", "magnitude", "landing", "transform", "fit_info"):
    assert np.array_equal(np.isnan(dev[k]), np.isnan(host[k])), (label, k)
  ok = host.status == compare.OK
  assert np.isnan(dev.diff[~ok]).all() and np.isnan(dev.magnitude[~ok]).all() and np.isnan(dev.landing[~ok]).all(), label
  worst = 0.0
  if ok.any():
    worst = float(np.abs(dev.diff[ok] - host.diff[ok]).max())
    both = ok & ~np.isnan(host.landing[:, 0])
    if both.any():
      worst = max(worst, float(np.abs(dev.landing[both] - host.landing[both]).max()))
    assert dev.magnitude[ok].tobytes() == np.sqrt(dev.diff[ok, 0] * dev.diff[ok, 0] + dev.diff[ok, 1] * dev.diff[ok, 1]).tobytes(), label
  d_rms = np.abs(dev.fit_info[:, 2:4] - host.fit_info[:, 2:4])
  rms = float(np.nanmax(d_rms)) if np.isfinite(d_rms).any() else 0.0
  print(f"{label}: {int(ok.sum())} of {ok.size} queries OK; device - host |diff|, |landing| {worst:.3g} px, fit RMS {rms:.3g} px; "
        f"linearisations device {dev.fit_info[:, 1].astype(int).tolist()} host {host.fit_info[:, 1].astype(int).tolist()}")
  assert worst <= BOUND and rms <= BOUND, label
  return dev


def with_fit_pixels_as_queries(b, distance, mode, fit_pixels):
  """the job, once with a few queries and once with its fit pixels as queries (where the two transforms are compared)"""
  return [pl.fit_job(b, distance, mode, fit_pixels=fit_pixels, pixels=pl.spread_pixels(9)),
          pl.fit_job(b, distance, mode, fit_pixels=fit_pixels, pixels=np.ascontiguousarray(fit_pixels))]


# ---- the map kernel at its edges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_lists_at_lane_wave_and_workgroup_edges(n):
  compare_runs([compare.Job(5, 0, 2.0, pixels=pl.spread_pixels(n, n)),
                pl.fit_job(3, np.inf, compare.ROTATION, pixels=pl.spread_pixels(n, n + 1))], f"lists of {n}")


@pytest.mark.parametrize("grid", [(1, 1), (1, 65), (17, 5)], ids=["1x1", "1x65", "17x5"])
def test_grids(grid):
  g = uncertainty.grid_of(pl.IMAGE_SIZE, grid)
  jobs = [pl.fit_job(3, 2.0, compare.RIGID, grid=g), compare.Job(6, 7, np.inf, grid=g)]
  dev = compare_runs(jobs, f"grid {grid}")
  as_list = [pl.fit_job(3, 2.0, compare.RIGID, pixels=jobs[0].pixel_array()), compare.Job(6, 7, np.inf, pixels=jobs[1].pixel_array())]
  assert pl.bytes_of(pl.run(as_list, "device")) == pl.bytes_of(dev)


# ---- the fit kernel at its edges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025])
def test_fit_sets_at_mfma_wave_and_workgroup_edges(m):
  px = pl.inner_pixels(m, m)
  jobs = with_fit_pixels_as_queries(2, np.inf, compare.ROTATION, px)
  if m >= 3:
    jobs += with_fit_pixels_as_queries(4, 2.0, compare.RIGID, px)
  dev = compare_runs(jobs, f"fit set of {m}")
  assert (dev.fit_info[:, 0] == m).all() and (dev.fit_info[:, 4] == compare.FIT_OK).all()


@pytest.mark.parametrize("case", ["every_other", "last_chunk"])
def test_fit_sets_with_pixels_that_do_not_take_part(case):
  px = pl.inner_pixels(150, 5)
  if case == "every_other":
    px[1::2] = NAN_PIXEL                                   # 75 take part
  else:
    px[128:] = NAN_PIXEL                                   # chunks 0 and 1 take part, the short last chunk does not
  good = px[~np.isnan(px[:, 0])]
  jobs = [pl.fit_job(0, np.inf, compare.ROTATION, fit_pixels=px, pixels=good), pl.fit_job(5, 2.0, compare.RIGID, fit_pixels=px, pixels=good),
          pl.fit_job(0, np.inf, compare.ROTATION, fit_pixels=good, pixels=good)]
  dev = compare_runs(jobs, case)
  assert (dev.fit_info[:, 0] == len(good)).all() and (dev.fit_info[:, 4] == compare.FIT_OK).all()
  assert np.abs(dev.diff[:len(good)] - dev.diff[2 * len(good):]).max() <= BOUND


# ---- jobs sharing one call ---------------------------------------------------------------------------------------------------
def test_jobs_of_every_kind_share_a_call_and_a_failed_fit_leaves_its_neighbours_alone():
  px = pl.spread_pixels(300, 3)
  good = [compare.Job(5, 1, 1.5, pixels=px),                                        # pinhole-4 -> fisheye transfer
          pl.fit_job(4, 1.5, compare.RIGID, pixels=px[:257]),                         # the tilted camera, a rigid fit
          pl.fit_job(7, 1.5, compare.NONE, grid=uncertainty.grid_of(pl.IMAGE_SIZE, (16, 12)))]
  failed = pl.fit_job(2, np.inf, compare.ROTATION, fit_pixels=pl.inner_pixels(1), pixels=px[:70])
  without = compare_runs(good, "transfer, rigid and none in one call")
  mixed = compare_runs(good[:1] + [failed] + good[1:], "the same with a TOO_FEW job between them")
  assert mixed.fit_info[1, 4] == compare.FIT_TOO_FEW and (mixed.status[300:370] == compare.NO_FIT).all()
  assert np.isnan(mixed.diff[300:370]).all() and np.isnan(mixed.transform[1]).all()
  keep = np.r_[0:300, 370:len(mixed.status)]
  assert mixed.diff[keep].tobytes() == without.diff.tobytes() and mixed.landing[keep].tobytes() == without.landing.tobytes()
  assert mixed.status[keep].tobytes() == without.status.tobytes() and mixed.magnitude[keep].tobytes() == without.magnitude.tobytes()
  assert mixed.transform[[0, 2, 3]].tobytes() == without.transform.tobytes()
  assert mixed.fit_info[[0, 2, 3]].tobytes() == without.fit_info.tobytes()


def test_two_calls_return_the_same_bytes_and_the_query_count():
  jobs = [pl.fit_job(2, 0.7 ** -1, compare.RIGID, pixels=pl.spread_pixels(300, 5)), compare.Job(8, 3, np.inf, pixels=pl.spread_pixels(65, 6)),
          pl.fit_job(5, np.inf, compare.ROTATION)]
  one, two = pl.run(jobs, "device"), pl.run(jobs, "device")
  assert pl.bytes_of(one) == pl.bytes_of(two)
  ms, n = compare.last_call_ms()
  assert n == 300 + 65 + 16 * 12 and set(ms) == {"upload", "fit", "map", "download", "call"} and ms["fit"] > 0 and ms["map"] > 0
  pl.run([compare.Job(8, 3, np.inf, pixels=pl.spread_pixels(65, 6))], "device")              # no job fits: no fit kernel
  assert compare.last_call_ms()[1] == 65


def test_every_family_every_mode_near_and_at_infinity():
  jobs = []
  for b in range(9):
    jobs += [pl.fit_job(b, np.inf, compare.ROTATION, pixels=pl.ul.edge_pixels()), pl.fit_job(b, 0.5, compare.RIGID, pixels=pl.ul.edge_pixels()),
             compare.Job(b, (b + 1) % 9, 0.5, pixels=pl.ul.edge_pixels()), compare.Job(b, b, np.inf, pixels=pl.ul.edge_pixels())]
  dev = compare_runs(jobs, "9 cameras x (rotation, rigid, transfer, itself)")
  assert (dev.status == compare.OK).mean() > 0.8 and (dev.fit_info[:, 4] == compare.FIT_OK).all()
  same = dev.status.reshape(-1, 9)[3::4] == compare.OK
  assert (dev.diff.reshape(-1, 9, 2)[3::4][same] == 0).all()


# ---- end to end -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def adjusted():
  """{name: (truth, bundle-adjusted)} (computed once, unchanged)"""
  out = {}
  for name in ("tiny", "tiny_fisheye", "tiny_rolling"):
    rig = synthetic.make_rig(name)
    out[name] = (calibration.from_rig(rig, "truth"), mirror(rig).bundle_adjust())     # (the blocks the rig itself optimises)
  return out


@pytest.mark.parametrize("name", ["tiny", "tiny_fisheye", "tiny_rolling"])
@pytest.mark.parametrize("reference", [None, 1], ids=["intrinsics", "transfer"])
def test_calibration_projection_diff(adjusted, name, reference):
  truth, c = adjusted[name]
  kw = dict(reference=reference, distance=1.5, grid=(5, 4), fit_grid=(12, 9))
  dev = truth.projection_diff(c, **kw)
  host = pl.on_host(truth.projection_diff, c, **kw)
  C = truth.size.cameras
  assert dev.diff.shape == (C, 4, 5, 2) and dev.transform.shape == (C, 6) and dev.landing.shape == (C, 4, 5, 2)
  assert np.array_equal(dev.status, host.status) and np.array_equal(dev.fit.n_fit, host.fit.n_fit) and np.array_equal(dev.fit.status, host.fit.status)
  ok = host.status == compare.OK
  # (the fisheye rig is a ring: transfers mostly land behind)
  assert ok.any(), (np.bincount(host.status.ravel(), minlength=4).tolist(), host.fit.status.tolist(), host.fit.iterations.tolist())
  worst = float(np.abs(dev.diff[ok] - host.diff[ok]).max())
  if reference is not None:
    worst = max(worst, float(np.abs(dev.landing[ok] - host.landing[ok]).max()))
    assert (dev.diff[reference][dev.status[reference] == compare.OK] == 0).all() and (dev.transform == 0).all()
  else:
    assert (dev.fit.status == compare.FIT_OK).all() and (dev.fit.rms_after <= dev.fit.rms_before).all()
    assert np.abs(dev.fit.rms_after - host.fit.rms_after).max() <= BOUND
  print(f"{name} reference {reference}: device - host {worst:.3g} px; median |diff| {np.nanmedian(dev.magnitude):.4f} px, linearisations "
        f"{dev.fit.iterations.tolist()}")
  assert worst <= BOUND


def test_a_calibration_against_itself_its_own_export_sigmas_and_the_report(adjusted, tmp_path):
  truth, c = adjusted["tiny"]
  zero = c.projection_diff(c, distance=2.0)
  ok = zero.status == compare.OK
  assert ok.any() and zero.magnitude[ok].max() <= 1e-9 and np.abs(zero.transform).max() < 1e-12
  names = dict(camera=list(c.camera_poses.names))
  path = str(tmp_path / "calibration.json")
  export.export(path, c, names, [])
  loaded = import_calib.load_calibration(path)
  for kw in (dict(distance=2.0), dict(reference=0, distance=2.0)):
    a, b = truth.projection_diff(c, **kw), truth.projection_diff(loaded, **kw)
    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("diff", "magnitude", "landing", "status", "transform"))
  s = truth.projection_diff(c, reference=0, distance=2.0, grid=(5, 4), sigmas=True)
  both = np.isfinite(s.cov0).all(axis=(-1, -2)) & np.isfinite(s.cov1).all(axis=(-1, -2)) & (s.status == compare.OK)
  assert both[1:].any() and np.isfinite(s.d[1:][both[1:]]).all() and (s.d[1:][both[1:]] >= 0).all()
  with pytest.raises(ValueError, match="two Calibrations with observations"):
    truth.projection_diff(loaded, reference=0, sigmas=True)
  with pytest.raises(ValueError, match="needs a reference camera"):
    truth.projection_diff(c, sigmas=True)
  records = []
  handler = logging.Handler()
  handler.emit = records.append
  logging.getLogger("calibration").addHandler(handler)
  try:
    logging.getLogger("calibration").setLevel(logging.INFO)
    truth.report_projection_diff(c, "test", distance=2.0)
    truth.report_projection_diff(loaded, "test", reference=0)
  finally:
    logging.getLogger("calibration").removeHandler(handler)
  lines = [r.getMessage() for r in records if "projection difference" in r.getMessage()]
  assert len(lines) == 2 * c.size.cameras, lines
  assert all("median=" in l and "implied rotation=" in l and "translation=" in l and "->" in l for l in lines[:c.size.cameras]), lines
  assert all("median=" in l and "implied" not in l for l in lines[c.size.cameras:]), lines


# ---- one cache ------------------------------------------------------------------------------------------------------------
def test_between_two_calls_of_another_family():
  rig = L.golden_rig("tiny")

  def view_poses():
    out = tables.view_poses(rig.points, rig.valid, rig.board_points, rig.truth.cameras)
    return b"".join(np.ascontiguousarray(a).tobytes() for a in out), _lib.call_ms("view_poses", range(4))[1]

  jobs = [compare.Job(5, 0, 2.0, pixels=pl.spread_pixels(65, 7)), pl.fit_job(2, 2.0, compare.RIGID, grid=uncertainty.grid_of(pl.IMAGE_SIZE, (3, 2)))]

  def own():
    return pl.bytes_of(pl.run(jobs, "device"))

  before = view_poses()
  first = own()
  assert compare.last_call_ms()[1] == 71
  after = view_poses()
  assert before == after and _lib.call_ms("projection_diff", range(5))[1] == 71
  assert own() == first
  with pytest.raises(RuntimeError) as e:
    pl.run([compare.Job(5, 0, -2.0, pixels=pl.spread_pixels(65, 7))], "device")
  message = "mcba_projection_diff: job 0: inv_distance must be finite and >= 0"
  assert message in str(e.value) and message in _lib.load().mcba_last_error().decode()
  with pytest.raises(RuntimeError, match="a rigid fit needs a finite distance"):
    pl.run([pl.fit_job(2, np.inf, compare.RIGID)], "device")
  assert own() == first and view_poses() == before
