"""GPU (MI355X): parameter covariance of the Gauss-Newton problem (mcba_covariance).

  * exact against numpy on small rigs (every motion / camera model, ragged cameras, the cameras block disabled, invalid and
    unobserved parameters) and at the full-size BASELINE configurations 8 x 500 x 2 rolling shutter and 16 x 1000 x 5;
  * gauge invariance of the intrinsics block, statistical meaning over 64 noise draws, the error paths, and no change to the
    solvers of the same handle.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.linalg

from multical_amd import synthetic, gauge
from multical_amd.backend import Handle
from multical_amd._lib import McbaError
from util import load_golden, mirror

pytestmark = pytest.mark.gpu


def _solve(h, x0):
  return h.solve(x0, tolerance=1e-12, max_iterations=200, tr_solver="exact").x


def _reference_columns(H, free, sigma2, cols):
  """sigma2 (H_free)^-1 restricted to columns `cols` (indices into x; zero where not free), through the same Jacobi scaling
  as the device route, with scipy's dense Cholesky."""
  Hf = H[np.ix_(free, free)]
  d = 1.0 / np.sqrt(np.diag(Hf))
  cf = scipy.linalg.cho_factor(Hf * d[:, None] * d[None, :], lower=True)
  pos = np.full(H.shape[0], -1)
  pos[free] = np.arange(free.size)
  live = np.flatnonzero(pos[cols] >= 0)
  E = np.zeros((free.size, live.size))
  E[pos[cols[live]], np.arange(live.size)] = 1.0
  X = scipy.linalg.cho_solve(cf, E) * d[:, None] * d[pos[cols[live]]][None, :]
  out = np.zeros((H.shape[0], len(cols)))
  out[np.ix_(free, live)] = sigma2 * X
  return out


def _check_block(dev, ref, var_rows, var_cols, tol, ratios=None):
  """|dSigma_ij| / sqrt(Sigma_ii Sigma_jj) <= tol; rows / columns with zero variance must be exactly zero.  ratios (a list): receives
  the largest error / tolerance ratio of the block."""
  scale = np.sqrt(np.outer(var_rows, var_cols))
  live = scale > 0
  assert np.all(dev[~live] == 0.0)
  if live.any():
    err = np.abs(dev - ref)[live] / scale[live]
    if ratios is not None:
      ratios.append(float(err.max()) / tol)
    assert err.max() <= tol, err.max()


def _compare(h, x, hold, H, m, cost2, tol, frames=None, cross=True, sigma2=None, ratios=None):
  """sigma2: the residual variance handed to the device (None: the device's own estimate cost2 / dof, which is checked)"""
  cov = h.covariance(x, hold=hold, cross=cross, sigma2=sigma2)
  n = h.n_params
  diag = np.diag(H)
  free = np.flatnonzero(~hold & (diag > 0))
  dof = m - free.size
  sigma2 = cost2 / dof if sigma2 is None else sigma2
  assert cov.dof == dof
  assert abs(cov.sigma2 - sigma2) <= 1e-12 * sigma2
  var = np.zeros(n)
  sh = cov.shared_index
  fi = cov.frame_index
  F = fi.shape[0]
  sel = np.arange(F) if frames is None else np.asarray(frames)
  cols = np.concatenate([sh, fi[sel].ravel()]).astype(np.int64)
  R = _reference_columns(H, free, cov.sigma2, cols)
  var[cols] = R[cols, np.arange(cols.size)]
  ns = sh.size
  _check_block(cov.shared, R[sh][:, :ns], var[sh], var[sh], tol, ratios)
  DF = fi.shape[1]
  for q, f in enumerate(sel):
    c0 = ns + q * DF
    _check_block(cov.frames[f], R[fi[f]][:, c0:c0 + DF], var[fi[f]], var[fi[f]], tol, ratios)
    if cross:
      _check_block(cov.frame_shared[f], R[fi[f]][:, :ns], var[fi[f]], var[sh], tol, ratios)
  # std: held exactly 0, unobserved NaN, free sqrt of the diagonal
  assert np.all(cov.std[hold] == 0.0)
  unobs = ~hold & (diag <= 0)
  assert np.all(np.isnan(cov.std[unobs]))
  chk = np.intersect1d(free, cols)
  if ratios is not None and chk.size:
    ratios.append(float((np.abs(cov.std[chk] - np.sqrt(var[chk])) / np.sqrt(var[chk])).max()) / tol)
  assert np.allclose(cov.std[chk], np.sqrt(var[chk]), rtol=tol, atol=0)
  return cov


def _hold_distortion(c, hold):
  """hold + every distortion coefficient: the rational / thin-prism terms of the ragged tiny rigs are determined to pivots of
  ~1e-11 only (the covariance is then refused, rightly); the ragged caller layout is exercised all the same."""
  hold = hold.copy()
  pos = sum(parameters_count(c, k) for k in ("camera_poses", "board_poses", "motion") if c.optimize[k] is True)
  for cam in c.cameras:
    n = np.asarray(cam.param_vec).size
    hold[pos + 5:pos + n] = True
    pos += n
  return hold


SMALL = [("tiny", False), ("tiny_rolling", False), ("tiny_fisheye", False), ("tiny_handeye", False), ("tiny_fishmix", False),
         ("tiny_mixed", False), ("tiny_fishmix5", False), ("tiny_fixintr", True), ("tiny_edge", True)]
RAGGED = ("tiny_mixed", "tiny_fishmix5")


@pytest.mark.parametrize("name,golden", SMALL)
def test_covariance_matches_numpy_on_small_rigs(name, golden):
  rig = load_golden(name)[1] if golden else synthetic.make_rig(name)
  c = mirror(rig)
  hold = gauge.default_hold(c)
  with Handle(c) as h:
    x = _solve(h, c.param_vec)
    if name in RAGGED:
      with pytest.raises(McbaError, match=r"rank deficient at x\[\d+\] \(cameras\[\d\]\.dist\[\d+\]\)"):
        h.covariance(x, hold=hold)
      hold = _hold_distortion(c, hold)
    J = h.jacobian(x).toarray()
    r = h.residuals(x)
    H = J.T @ J
    cov = _compare(h, x, hold, H, r.size, float(r @ r), 1e-8)
    if name == "tiny_edge":   # the fixture exists to exercise every unobserved-parameter rule
      assert np.isnan(cov.std).sum() > 0


@pytest.mark.parametrize("cfg", ["cfg3", "cfg4"])
def test_covariance_matches_numpy_at_full_size(cfg):
  rig = synthetic.make_rig(cfg)
  c = mirror(rig)
  hold = gauge.default_hold(c)
  with Handle(c) as h:
    x = _solve(h, c.param_vec)
    cost, _, _ = h.normal_equations(x)
    H = h.dense_hessian()
    F = rig.valid.shape[1]
    frames = np.unique(np.linspace(0, F - 1, 24).astype(int))
    _compare(h, x, hold, H, h.n_residuals, 2.0 * cost, 1e-7, frames=frames, cross=True)


def test_covariance_intrinsics_do_not_depend_on_the_gauge():
  c = mirror(synthetic.make_rig("tiny"))
  with Handle(c) as h:
    x = _solve(h, c.param_vec)
    first = gauge.default_hold(c)
    last = first.copy()
    last[:6] = False
    C = c.size.cameras
    last[6 * (C - 1):6 * C] = True
    a, b = h.covariance(x, hold=first), h.covariance(x, hold=last)
  intr = np.flatnonzero(np.isin(a.shared_index, np.arange(x.size - parameters_count(c, "cameras"), x.size)))
  A, B = a.shared[np.ix_(intr, intr)], b.shared[np.ix_(intr, intr)]
  s = np.sqrt(np.outer(np.diag(A), np.diag(A)))
  live = s > 0
  assert (np.abs(A - B)[live] / s[live]).max() <= 1e-8


def parameters_count(c, block):
  from multical_amd import parameters
  return parameters.count(c.params[block])


def _to_gauge(c):
  """c moved to the gauge of gauge.canonical: first valid camera and first valid board at the identity."""
  T0 = np.asarray(c.camera_poses.poses)[gauge._first_valid(c.camera_poses.valid)]
  S0 = np.asarray(c.board_poses.poses)[gauge._first_valid(c.board_poses.valid)]
  c = c.transform_views(T0)
  return c.copy(board_poses=c.board_poses.pre_transform(np.linalg.inv(S0)), motion=c.motion.post_transform(S0))


def test_covariance_predicts_the_spread_of_noisy_solves():
  rig = synthetic.make_rig("tiny", noise=0.0, outlier_frac=0.0)
  truth = _to_gauge(mirror(SimpleNamespace(**{**vars(rig), "init": rig.truth})))
  hold = gauge.default_hold(truth)
  pred = truth.covariance(sigma2=0.04)
  rng = np.random.default_rng(7)
  xs, s2 = [], []
  for _ in range(64):
    noisy = SimpleNamespace(**vars(rig))
    noisy.points = rig.points + rng.normal(0.0, 0.2, rig.points.shape) * rig.valid[..., None]
    noisy.init = rig.truth
    c = mirror(noisy)
    with Handle(c) as h:
      x = _solve(h, c.param_vec)
    solved = _to_gauge(c.with_param_vec(x))
    xs.append(solved.param_vec)
    s2.append(solved.covariance().sigma2)
  xs = np.array(xs)
  free = ~hold & np.isfinite(pred.std) & (pred.std > 0)
  ratio = xs[:, free].std(axis=0, ddof=1) / pred.std[free]
  assert 0.85 <= np.median(ratio) <= 1.15, np.median(ratio)
  assert ratio.min() >= 0.6 and ratio.max() <= 1.6, (ratio.min(), ratio.max())
  assert abs(np.mean(s2) / 0.04 - 1.0) <= 0.15, np.mean(s2)


def test_covariance_errors():
  c = mirror(synthetic.make_rig("tiny"))
  with Handle(c) as h:
    x = _solve(h, c.param_vec)
    with pytest.raises(McbaError, match=r"covariance: rank deficient at x\[\d+\] \(.+\); hold more parameters"):
      h.covariance(x, hold=np.zeros(x.size, dtype=bool))
    cov = h.covariance(x, hold=gauge.default_hold(c))   # the handle is still usable after the failure
    assert np.isfinite(cov.shared).all()
  with pytest.raises(ValueError, match="explicit hold"):
    c.enable(boards=True).covariance()
  # m <= p_free: keep the residuals of one view only
  sub = mirror(synthetic.make_rig("tiny"))
  mask = np.zeros(sub.point_table.valid.shape, dtype=bool)
  C0, F0, B0, P0 = np.argwhere(sub.valid)[0]
  pts = np.flatnonzero(sub.valid[C0, F0, B0])[:4]
  mask[C0, F0, B0, pts] = True          # 8 residuals against the frame's 6 pose parameters and 9 observed intrinsics
  few = sub.copy(inlier_mask=mask)
  with Handle(few) as h:
    with pytest.raises(McbaError, match="m <= p_free"):
      h.covariance(few.param_vec, hold=gauge.default_hold(few))


def test_covariance_leaves_the_solvers_alone():
  c = mirror(synthetic.make_rig("tiny_rolling"))
  x0 = c.param_vec
  with Handle(c) as h:
    before = [h.solve(x0, tr_solver=s).x for s in ("exact", "lsmr")]
    h.covariance(before[0], hold=gauge.default_hold(c), cross=True)
    after = [h.solve(x0, tr_solver=s).x for s in ("exact", "lsmr")]
  for a, b in zip(before, after):
    assert np.array_equal(a, b)


def test_calibration_covariance_api():
  c = mirror(synthetic.make_rig("tiny_mixed"))
  hold = _hold_distortion(c, gauge.default_hold(c))
  cov = c.covariance(hold=hold, cross=True)
  assert np.array_equal(cov.held, hold) and cov.frames.shape[1:] == (6, 6) and "frame_shared" in cov
  std = c.parameter_std(hold=hold)
  assert std["camera_poses"].shape == (4, 6) and np.all(std["camera_poses"][0] == 0)
  import logging
  records = []
  handler = logging.Handler()
  handler.emit = records.append
  logging.getLogger("calibration").addHandler(handler)
  try:
    logging.getLogger("calibration").setLevel(logging.INFO)
    c.report_uncertainty("test", hold=hold)
  finally:
    logging.getLogger("calibration").removeHandler(handler)
  lines = [r.getMessage() for r in records]
  assert len(lines) == 4 and all("fx=" in l and "deg" in l for l in lines), lines
  assert [a.size for a in std["cameras"]] == [np.asarray(cam.param_vec).size for cam in c.cameras]
  np.testing.assert_array_equal(np.concatenate([a.ravel() for a in std["cameras"]]),
                                cov.std[-sum(a.size for a in std["cameras"]):])
