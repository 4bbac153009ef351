"""GPU (MI355X): the Gram matrices of the residual field (mcba_residual_gram) against the g++ build of the same
header (tests/residual_field), and Calibration.residual_field on top of them.

Handles come from the tiny goldens through util.mirror, at the fixture's start parameters.  The host side receives the device's own
projected points and valid mask (Handle.project / reprojection_error) next to the observed points and the inlier mask, so the
comparison pins that the residual is the one mcba_project returns.  Bound, per entry: |dG_ij| <= 4 n 2^-53 A_ij with n the rows
of the (camera, fold) slice and A the Gram matrix of the absolute rows -- the standard bound of two summation orders of the same
products; counts, outside counts and coverage maps must be equal.  Every comparison prints its worst |d| / bound before it asserts
(profiles/residual_field_parity.txt keeps a run).
"""
import functools
import logging

import numpy as np
import pytest

from multical_amd import residual_field as rf
from multical_amd.backend import Handle
from multical_amd._lib import McbaError
from util import load_golden, mirror

import residual_field_host_lib as hl

pytestmark = pytest.mark.gpu

ROWS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 257)


@functools.lru_cache(maxsize=None)
def _case(name):
  """(calibration, x, sizes, observed [C,F,B,P,2]) of a golden fixture"""
  c = mirror(load_golden(name)[1])
  x = np.array(c.param_vec, dtype=np.float64)
  sizes = [tuple(int(v) for v in cam.image_size) for cam in c.cameras]
  obs = np.array(c.point_table.points, dtype=np.float64)
  for a in (x, obs):
    a.setflags(write=False)
  return c, x, sizes, obs


@functools.lru_cache(maxsize=None)
def _device_tables(name):
  """(projected [C,F,B,P,2], valid [C,F,B,P]) of the device at the fixture's x, computed once"""
  c, x, _, _ = _case(name)
  with Handle(c) as h:
    proj = h.project(x)
    _, valid = h.reprojection_error(x)
  proj.setflags(write=False)
  valid.setflags(write=False)
  return proj, valid


def _host(name, inlier, nx=5, ny=4, n_folds=5, inliers_only=True, coverage=(16, 12), observed=None):
  _, _, sizes, obs = _case(name)
  proj, valid = _device_tables(name)
  return hl.gram(proj, obs if observed is None else observed, valid, inlier, sizes, nx, ny, n_folds, inliers_only, coverage)


def _compare(dev, host, what):
  ratio = hl.worst_ratio(dev.gram, host)
  print(f"  {what}: rows {int(host.count.sum())}, worst |d| / bound = {ratio:.3f}")
  assert np.array_equal(dev.count, host.count), what
  assert np.array_equal(dev.outside, host.outside), what
  if host.coverage is not None:
    assert np.array_equal(dev.coverage, host.coverage), what
  assert np.array_equal(dev.gram, np.swapaxes(dev.gram, -1, -2)), what
  assert ratio <= 1.0, what
  assert np.all(dev.gram[host.count == 0] == 0.0), what
  return ratio


def _slice_mask(name, camera, order, m, base):
  """`base` with exactly m inliers in `camera`: the first m valid slots of its frames taken in `order`"""
  _, valid = _device_tables(name)
  mask = base.copy()
  mask[camera] = False
  left = m
  for f in order:
    slots = np.argwhere(valid[camera, f])[:left]
    mask[camera, f, slots[:, 0], slots[:, 1]] = True
    left -= len(slots)
  assert left == 0 and mask[camera].sum() == m
  return mask


# ---- rows per slice -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", ROWS)
def test_rows_in_camera0_fold0(m):
  """exactly m inliers in camera 0, fold 0 (n_folds = 1: one frame per wavefront), filled from the camera's fullest frame (88 valid
  slots) down: m <= 5 the MFMA k-step of 4, 63 / 64 / 65 the 64-row chunk edge inside one wavefront, 127 .. 129 and 257 rows spread
  over two and four chunk partials.  The other cameras keep their inliers."""
  name = "tiny_rolling"
  c, x, sizes, _ = _case(name)
  _, valid = _device_tables(name)
  order = np.argsort(-valid[0].sum(axis=(1, 2)), kind="stable")
  mask = _slice_mask(name, 0, order, m, np.asarray(c.inliers, dtype=bool))
  with Handle(c) as h:
    h.set_inliers(mask)
    dev = h.residual_gram(x, sizes, n_folds=1)
  host = _host(name, mask, n_folds=1)
  assert host.count[0, 0] == m and (host.count[1:, 0] == np.asarray(c.inliers)[1:].sum(axis=(1, 2, 3))).all()
  _compare(dev, host, f"camera 0 with {m} rows")
  if m == 0:
    assert not dev.gram[0, 0].any()


@pytest.mark.parametrize("m", (127, 128, 129, 192, 253))
def test_rows_in_one_wavefront(m):
  """m rows in ONE frame (camera 2, frame 2 of tiny_rolling: 253 valid slots), so one wavefront runs two to four dense chunks"""
  name = "tiny_rolling"
  c, x, sizes, _ = _case(name)
  mask = _slice_mask(name, 2, [2], m, np.asarray(c.inliers, dtype=bool))
  with Handle(c) as h:
    h.set_inliers(mask)
    dev = h.residual_gram(x, sizes, n_folds=2)
  host = _host(name, mask, n_folds=2)
  assert host.count[2].tolist() == [m, 0]
  _compare(dev, host, f"one frame with {m} rows")


# ---- column tile edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", sorted(hl.GRIDS))
def test_column_tiles(grid):
  name = "tiny"
  c, x, sizes, _ = _case(name)
  nx, ny = grid
  with Handle(c) as h:
    dev = h.residual_gram(x, sizes, nx=nx, ny=ny, n_folds=5)
  nc = hl.GRIDS[grid]
  assert dev.gram.shape == (2, 5, nc, nc)
  _compare(dev, _host(name, np.asarray(c.inliers, dtype=bool), nx, ny, 5), f"{nx} x {ny}: NC = {nc}")


# ---- folds ------------------------------------------------------------------------------------------------------------------------
def test_folds():
  name = "tiny_handeye"
  c, x, sizes, _ = _case(name)
  inl = np.asarray(c.inliers, dtype=bool)
  F = inl.shape[1]
  assert F < 16
  with Handle(c) as h:
    dev = {k: h.residual_gram(x, sizes, n_folds=k) for k in (1, 2, 5, 16)}
  for k, d in dev.items():
    host = _host(name, inl, n_folds=k)
    _compare(d, host, f"{k} folds")
    assert not d.gram[:, F:].any() and not d.count[:, F:].any()          # folds without a frame
    one = _host(name, inl, n_folds=1)
    diff, lim = np.abs(d.gram.sum(axis=1) - dev[1].gram[:, 0]), hl.bound(one.absgram, one.count)[:, 0]
    assert (diff <= lim).all() and np.array_equal(d.count.sum(axis=1), dev[1].count[:, 0])


# ---- coverage, inliers_only, outside ------------------------------------------------------------------------------------------------
def test_coverage_inliers_only_and_outside():
  name = "tiny"
  c, x, sizes, obs = _case(name)
  _, valid = _device_tables(name)
  with Handle(c) as h:
    err, _ = h.reprojection_error(x)
    n_in, n_valid = h.reject_outliers(x, float(np.quantile(err[valid], 0.8)))
    inl = h.get_inliers()
    only, every = h.residual_gram(x, sizes, inliers_only=True), h.residual_gram(x, sizes, inliers_only=False)
  assert 0 < n_in < n_valid == valid.sum() and inl.sum() == n_in
  _compare(only, _host(name, inl, inliers_only=True), "inliers only after a rejection")
  _compare(every, _host(name, inl, inliers_only=False), "all valid slots after a rejection")
  assert only.count.sum() == n_in and every.count.sum() == n_valid
  assert np.array_equal(only.coverage, every.coverage)                   # the maps do not depend on inliers_only
  assert only.coverage[:, 0].sum() == n_in and only.coverage.sum() == n_valid
  # one observed pixel moved out of the image, through a modified table
  cam, f, b, p = np.argwhere(inl)[11]
  moved = obs.copy()
  moved[cam, f, b, p, 1] = sizes[cam][1] + 2.0
  c2 = c.copy(point_table=c.point_table._extend(points=moved))
  with Handle(c2) as h:
    h.set_inliers(inl)
    proj, valid2 = h.project(x), h.reprojection_error(x)[1]
    dev = h.residual_gram(x, sizes)
  host = hl.gram(proj, moved, valid2, inl, sizes)
  assert host.outside[cam] == 1 and host.outside.sum() == 1 and host.count.sum() == n_in - 1
  _compare(dev, host, "one observed pixel outside the image")


# ---- repeatability ------------------------------------------------------------------------------------------------------------------
def test_same_bytes_and_state_untouched():
  name = "tiny"
  c, x, sizes, _ = _case(name)
  with Handle(c) as h:
    a, b = h.residual_gram(x, sizes), h.residual_gram(x, sizes)
    assert a.gram.tobytes() == b.gram.tobytes() and np.array_equal(a.count, b.count) and np.array_equal(a.coverage, b.coverage)
    res = h.solve(x, tolerance=1e-10, max_iterations=50, tr_solver="exact", verbose=0)
    r_before = h.residuals(res.x)
    after = h.residual_gram(res.x, sizes)
    assert h.residuals(res.x).tobytes() == r_before.tobytes()
    proj, valid = h.project(res.x), h.reprojection_error(res.x)[1]
    again = h.residual_gram(x, sizes)
  host = hl.gram(proj, _case(name)[3], valid, np.asarray(c.inliers, dtype=bool), sizes)
  _compare(after, host, "after a solve on the same handle")
  assert after.gram[..., -1, -1].sum() < a.gram[..., -1, -1].sum()       # the solve lowered r_y^T r_y
  assert again.gram.tobytes() == a.gram.tobytes()


# ---- motion and camera families -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hl.FIXTURES)
def test_families(name):
  c, x, sizes, _ = _case(name)
  inl = np.asarray(c.inliers, dtype=bool)
  with Handle(c) as h:
    dev = h.residual_gram(x, sizes, n_folds=3, inliers_only=False)
  _compare(dev, _host(name, inl, n_folds=3, inliers_only=False), name)


def test_boards_optimised_handle():
  name = "tiny"
  c, x0, sizes, _ = _case(name)
  cb = c.enable(boards=True)
  xb = np.array(cb.param_vec, dtype=np.float64)
  with Handle(cb) as h:
    dev = h.residual_gram(xb, sizes)
    proj, valid = h.project(xb), h.reprojection_error(xb)[1]
  _compare(dev, hl.gram(proj, _case(name)[3], valid, np.asarray(cb.inliers, dtype=bool), sizes), "boards optimised")


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_calibration_residual_field(caplog):
  name = "tiny"
  c, x, sizes, _ = _case(name)
  inl = np.asarray(c.inliers, dtype=bool)
  sigma2 = 0.37
  out = c.residual_field(sigma2=sigma2)
  host = _host(name, inl)
  want = rf.analyse(host.gram, host.count, host.outside, host.coverage, sizes, 5, 4, sigma2)
  for key in ("coefficients", "field", "field_std", "rms", "systematic_rms", "explained", "cv_gain", "T", "nu", "z"):
    a, b = np.asarray(getattr(out, key)), np.asarray(getattr(want, key))
    err = np.abs(a - b).max() / np.abs(b).max()
    print(f"  {key}: {err:.2e}")
    assert err <= 1e-9, key
  assert np.array_equal(out.n, want.n) and np.array_equal(out.coverage, want.coverage) and np.array_equal(out.outside, want.outside)
  assert out.field.shape == (2, 12, 16, 2)
  default = c.residual_field()                                           # sigma2 from the covariance chain
  assert default.sigma2 == pytest.approx(c.covariance().sigma2, rel=1e-12)
  with caplog.at_level(logging.INFO, logger="calibration"):
    c.report_residual_field("end", sigma2=sigma2)
  lines = [r.getMessage() for r in caplog.records if "residual field" in r.getMessage()]
  assert len(lines) == 2 and all(line.startswith("end ") and "cv_gain=" in line and " z=" in line for line in lines)
  ms, n_rows = rf.last_call_ms()
  assert n_rows == int(want.n.sum()) and ms["gram"] > 0.0 and ms["call"] >= ms["gram"]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals():
  name = "tiny"
  c, x, sizes, _ = _case(name)
  with Handle(c) as h:
    for kwargs, message in ((dict(nx=6, ny=4), "need more than 64 columns"), (dict(nx=0), "nx and ny must be at least 1"),
                            (dict(ny=0), "nx and ny must be at least 1"), (dict(n_folds=0), "n_folds must be at least 1"),
                            (dict(n_folds=17), "at most 16 folds"), (dict(coverage=(64, 64)), "coverage map has between 1 and 512 cells")):
      with pytest.raises(McbaError, match=message):
        h.residual_gram(x, sizes, **kwargs)
    for bad in ([(0, 1216), sizes[1]], [sizes[0], (1936, -1)]):
      with pytest.raises(McbaError, match="image size of camera . is not positive"):
        h.residual_gram(x, bad)
    assert h.residual_gram(x, sizes).count.sum() == np.asarray(c.inliers).sum()    # the handle still works
  F = c.size.rig_poses
  with Handle(c, frame_range=(0, F // 2)) as h:
    with pytest.raises(McbaError, match="residual field: a frame-sharded handle is not supported"):
      h.residual_gram(x, sizes)
