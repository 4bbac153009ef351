"""GPU (MI355X): per-observation prediction covariance, leverage and studentised errors (mcba_observation_covariance,
DESIGN.md 3.7) against a QR computation on the device's own Jacobian.

Reference (built here, once per rig): J = h.jacobian(x) (pinned to the reference's finite differences elsewhere), thin QR of the
Jacobi-scaled free columns J_free D = Q R; H_ii = Q_i Q_i^T for inlier rows, z = R^-T D j for the valid rows that are not
inliers (rows of a second handle on c.copy(inlier_mask=None)).  Tolerance: NOT hard-coded -- the same blocks by numpy's
normal-equation route (Cholesky of (J D)^T (J D), whitened solve), tol = max(1e-9, 100 x max |normal-eq - QR| / sqrt(C_uu C_vv)).
Each test prints the measured device-vs-QR maxima before it asserts (profiles/obs_cov_parity.txt keeps a run of them).
"""
import functools
import logging

import numpy as np
import pytest
import scipy.linalg

from multical_amd import synthetic, gauge
from multical_amd.backend import Handle
from multical_amd._lib import McbaError
from util import load_golden, mirror
from test_observation_covariance_host import studentized, max_eig

pytestmark = pytest.mark.gpu

GOLDEN_ONLY = ("tiny_fixintr", "tiny_edge")
RAGGED = ("tiny_mixed", "tiny_fishmix5")


def _solve(h, x0):
  return h.solve(x0, tolerance=1e-12, max_iterations=200, tr_solver="exact").x


def _hold_distortion(c, hold):
  """hold + every distortion coefficient (the rational / thin-prism terms of the ragged tiny rigs are refused as rank deficient)"""
  from multical_amd import parameters
  hold = hold.copy()
  pos = sum(parameters.count(c.params[k]) for k in ("camera_poses", "board_poses", "motion") if c.optimize[k] is True)
  for cam in c.cameras:
    n = np.asarray(cam.param_vec).size
    hold[pos + 5:pos + n] = True
    pos += n
  return hold


def _blocks(Z):
  """rows 2i, 2i+1 of Z -> (uu, uv, vv) of Z_i Z_i^T"""
  a, b = Z[0::2], Z[1::2]
  return np.stack([np.einsum("ij,ij->i", a, a), np.einsum("ij,ij->i", a, b), np.einsum("ij,ij->i", b, b)], axis=-1)


def _reference(c, x, hold):
  """struct of the reference side: cov [C,F,B,P,3] (NaN / 0 by the rules), student, valid, inlier, sigma2, dof, p_free, tol"""
  with Handle(c) as h:
    Jin = h.jacobian(x).toarray()
    rin = h.residuals(x)
    _, valid = h.reprojection_error(x)
  inlier = np.asarray(c.inliers, dtype=bool)
  assert not (inlier & ~valid).any()
  if (inlier == valid).all():
    Jall, rall = Jin, rin
  else:
    with Handle(c.copy(inlier_mask=None)) as hv:
      Jall = hv.jacobian(x).toarray()
      rall = hv.residuals(x)
  assert Jin.shape[0] == 2 * inlier.sum() and Jall.shape[0] == 2 * valid.sum()
  diag = (Jin * Jin).sum(axis=0)
  free = np.flatnonzero(~hold & (diag > 0))
  unobs = np.flatnonzero(~hold & (diag <= 0))
  D = 1.0 / np.sqrt(diag[free])
  A = Jin[:, free] * D
  Q, R = np.linalg.qr(A)
  dof = Jin.shape[0] - free.size
  sigma2 = float(rin @ rin) / dof
  in_of_valid = inlier[valid]                       # rows are C-ordered: the inlier rows are a subset of the valid rows
  Aall = Jall[:, free] * D
  Zqr = scipy.linalg.solve_triangular(R.T, Aall.T, lower=True).T
  Hqr = _blocks(Zqr)
  Hqr[in_of_valid] = _blocks(Q)
  L = np.linalg.cholesky(A.T @ A)
  Hne = _blocks(scipy.linalg.solve_triangular(L, Aall.T, lower=True).T)
  nanrow = (Jall[:, unobs] != 0).any(axis=1).reshape(-1, 2).any(axis=1)
  scale = np.sqrt(Hqr[:, 0] * Hqr[:, 2])
  ok = ~nanrow & (scale > 0)
  spread = float((np.abs(Hne - Hqr)[ok].max(axis=1) / scale[ok]).max())
  tol = max(1e-9, 100.0 * spread)
  cov_v = sigma2 * Hqr
  cov_v[nanrow] = np.nan
  cov = np.zeros(valid.shape + (3,))
  cov[valid] = cov_v
  r = np.zeros(valid.shape + (2,))
  r[valid] = rall.reshape(-1, 2)
  stud = np.where(valid, studentized(cov, r, sigma2, inlier), 0.0)
  # printed only, never a bound: how far numpy's own normal-equation route is from QR in d_i (same slots, same formula)
  cov_ne = np.zeros(valid.shape + (3,))
  cov_ne[valid] = np.where(nanrow[:, None], np.nan, sigma2 * Hne)
  stud_ne = studentized(cov_ne, r, sigma2, inlier)
  fin = valid & np.isfinite(stud) & np.isfinite(stud_ne) & (stud > 0)
  spread_student = float((np.abs(stud_ne - stud)[fin] / stud[fin]).max())
  return dict(cov=cov, student=stud, valid=valid, inlier=inlier, sigma2=sigma2, dof=dof, p_free=free.size, tol=tol,
              spread=spread, spread_student=spread_student, cond=float(np.linalg.cond(R)))


def _errors(dev, ref):
  """(max |dC| / sqrt(C_uu C_vv), max relative student error) over the determined valid slots; the NaN / 0 / inf pattern must be
  exactly the reference's"""
  cov3 = dev.cov.reshape(dev.cov.shape[:-2] + (4,))[..., [0, 1, 3]]
  assert np.array_equal(dev.cov[..., 0, 1], dev.cov[..., 1, 0], equal_nan=True)
  refnan = np.isnan(ref["cov"][..., 0])
  assert np.array_equal(np.isnan(cov3).all(axis=-1), refnan) and np.array_equal(np.isnan(cov3).any(axis=-1), refnan)
  assert np.array_equal(np.isnan(dev.student), refnan)
  assert np.all(cov3[~ref["valid"]] == 0.0) and np.all(dev.student[~ref["valid"]] == 0.0)
  live = ref["valid"] & ~refnan
  scale = np.sqrt(ref["cov"][..., 0] * ref["cov"][..., 2])[live]
  e_cov = float((np.abs(cov3 - ref["cov"])[live].max(axis=1) / scale).max())
  ds, rs = dev.student[live], ref["student"][live]
  assert np.array_equal(np.isinf(ds), np.isinf(rs))
  fin = np.isfinite(rs)
  rel = np.abs(ds - rs)[fin] / rs[fin]
  e_st = float(rel.max())
  k = np.flatnonzero(fin)[int(rel.argmax())]
  idx = tuple(int(a[k]) for a in np.nonzero(live))
  print(f"  worst student slot {idx}: device {ds[k]!r} reference {rs[k]!r}; C device {cov3[idx]} reference {ref['cov'][idx]} "
        f"inlier {bool(ref['inlier'][idx])}")
  return e_cov, e_st


def _case(name, frames=None, reject=None):
  """(calibration at the solved x, x, hold, reference), computed once per rig and shared"""
  return _case_cached(name, frames, reject)


@functools.lru_cache(maxsize=None)
def _case_cached(name, frames, reject):
  rig = load_golden(name)[1] if name in GOLDEN_ONLY else synthetic.make_rig(name, frames=frames)
  c = mirror(rig)
  hold = gauge.default_hold(c)
  if name in RAGGED:
    hold = _hold_distortion(c, hold)
  with Handle(c) as h:
    x = _solve(h, c.param_vec)
  c = c.with_param_vec(x)
  if reject is not None:
    c = c.reject_outliers(float(np.quantile(c.reprojection_error, reject)))
  if name == "tiny_edge":
    # the fixture's invalid frames / cameras / boards carry no valid slot; take the inliers of its LAST valid frame away as well:
    # its valid points then depend on 6 parameters that are unobserved and not held -- the prediction there is unconstrained
    mask = np.array(c.valid)
    mask[:, np.flatnonzero(mask.any(axis=(0, 2, 3)))[-1]] = False
    c = c.copy(inlier_mask=mask)
  ref = _reference(c, x, hold)
  for v in ref.values():
    if isinstance(v, np.ndarray):
      v.setflags(write=False)
  return c, x, hold, ref


def _device(name, frames=None, reject=None):
  """the device's result of a case and its errors against the reference (once per case; printed before anything is asserted)"""
  return _device_cached(name, frames, reject)


@functools.lru_cache(maxsize=None)
def _device_cached(name, frames, reject):
  c, x, hold, ref = _case(name, frames, reject)
  with Handle(c) as h:
    dev = h.observation_covariance(x, hold=hold)
  e_cov, e_st = _errors(dev, ref)
  label = name + (f"/{frames}" if frames else "") + ("/rejected" if reject else "")
  print(f"obs_cov_parity {label}: device-vs-QR cov {e_cov:.3e} student {e_st:.3e} | tol {ref['tol']:.3e} "
        f"(normal-eq vs QR {ref['spread']:.3e}, in d_i {ref['spread_student']:.3e}, cond(JD) {ref['cond']:.1f}) | trace {dev.trace!r} p_free {ref['p_free']} "
        f"sigma2 {dev.sigma2:.6g} dof {dev.dof}")
  return dev, e_cov, e_st


def _check_cov(record_property, name, frames=None, reject=None):
  ref = _case(name, frames, reject)[3]
  dev, e_cov, _ = _device(name, frames, reject)
  record_property("device_vs_qr_cov", e_cov)
  record_property("tol", ref["tol"])
  assert dev.dof == ref["dof"] and abs(dev.sigma2 - ref["sigma2"]) <= 1e-12 * ref["sigma2"]
  assert e_cov <= ref["tol"], (e_cov, ref["tol"])
  assert abs(dev.trace - ref["p_free"]) <= ref["tol"] * ref["p_free"], (dev.trace, ref["p_free"])
  return dev, ref


def _check_student(record_property, name, frames=None, reject=None):
  ref = _case(name, frames, reject)[3]
  _, _, e_st = _device(name, frames, reject)
  record_property("device_vs_qr_student", e_st)
  record_property("tol", ref["tol"])
  assert e_st <= ref["tol"], (e_st, ref["tol"])


SMALL = ["tiny", "tiny_rolling", "tiny_fisheye", "tiny_handeye", "tiny_fishmix", "tiny_fixintr", "tiny_mixed", "tiny_fishmix5",
         "tiny_edge", "tiny_bigboard", "tiny_manypairs"]


@pytest.mark.parametrize("name", SMALL)
def test_prediction_covariance_matches_qr(name, record_property):
  _, ref = _check_cov(record_property, name)
  if name == "tiny_edge":   # some valid slots are not constrained; that exactly the slots the rule names are NaN: _errors
    nan = np.isnan(ref["cov"][..., 0])
    assert nan.sum() > 0 and (ref["valid"] & ~nan).sum() > 0


@pytest.mark.parametrize("name", SMALL)
def test_studentized_error_matches_qr(name, record_property):
  """Relative error of d_i against the QR reference under the tolerance of the covariance blocks.  tiny_mixed and tiny_fishmix5
  each hold an inlier whose H_ii has its larger eigenvalue at about 1 - 1e-5 / 1 - 2.4e-4: d_i needs 1 - h there, which only the
  whitened route (a sum of squares per point) delivers -- the Sigma-route missed these two cases by 2.4e-5 / 8.6e-9."""
  _check_student(record_property, name)


@pytest.mark.parametrize("name", ["tiny_rolling", "tiny_handeye", "tiny_fixintr", "tiny_edge", "tiny_mixed"])
def test_sigma_route_fallback_meets_the_tolerance_of_the_blocks(name, record_property):
  """The fallback of systems whose whitened panel does not fit LDS (G = That Sigma_view That^T per view), forced here: the blocks,
  the NaN / 0 pattern and the trace hold to the same tolerance; the studentised error is only printed (it loses 1 - h at near-unit
  leverage: 2.4e-5 on tiny_mixed)."""
  c, x, hold, ref = _case(name)
  with Handle(c) as h:
    h.set_observation_covariance_route(True)
    dev = h.observation_covariance(x, hold=hold)
  e_cov, e_st = _errors(dev, ref)
  print(f"obs_cov_parity {name}/sigma-route: device-vs-QR cov {e_cov:.3e} student {e_st:.3e} | tol {ref['tol']:.3e}")
  record_property("device_vs_qr_cov", e_cov)
  assert e_cov <= ref["tol"], (e_cov, ref["tol"])
  assert abs(dev.trace - ref["p_free"]) <= ref["tol"] * ref["p_free"], (dev.trace, ref["p_free"])


def test_inliers_and_rejected_points_use_their_own_covariance(record_property):
  c, x, hold, ref = _case("tiny_rolling", reject=0.9)
  out = ref["valid"] & ~ref["inlier"]
  assert out.any() and ref["inlier"].any()          # the handle's inlier set is a strict subset of valid
  dev, _ = _check_cov(record_property, "tiny_rolling", reject=0.9)
  _check_student(record_property, "tiny_rolling", reject=0.9)
  cov3 = dev.cov.reshape(dev.cov.shape[:-2] + (4,))[..., [0, 1, 3]]
  with Handle(c) as h:
    r = np.zeros(ref["valid"].shape + (2,))
    r[ref["valid"]] = (h.project(x) - np.asarray(c.point_table.points))[ref["valid"]]
  # the device's own C_i with the two signs: sigma2 I + C outside the inlier set, sigma2 I - C inside
  for mask, inl in ((out, False), (ref["inlier"], True)):
    want = studentized(cov3[mask], r[mask], dev.sigma2, np.full(mask.sum(), inl))
    assert np.allclose(dev.student[mask], want, rtol=1e-9, atol=0)
    other = studentized(cov3[mask], r[mask], dev.sigma2, np.full(mask.sum(), not inl))
    assert not np.allclose(dev.student[mask], other, rtol=1e-6, atol=0)


@pytest.mark.parametrize("cfg", ["cfg3", "cfg4"])
def test_mid_size_rigs(cfg, record_property):
  """cfg3 x 12 frames: 8 x 12 x 2 rolling shutter, NV = 22; cfg4 x 12 frames: 16 x 12 x 5, ns = 286 > 256, 80 pairs per frame"""
  dev, ref = _check_cov(record_property, cfg, frames=12)
  _check_student(record_property, cfg, frames=12)
  uu, uv, vv = dev.cov[..., 0, 0], dev.cov[..., 0, 1], dev.cov[..., 1, 1]
  with np.errstate(invalid="ignore"):
    std = np.sqrt(np.maximum(max_eig(uu, uv, vv), 0.0))
  std = np.where(ref["valid"] & ~np.isnan(std), std, 0.0)
  assert np.array_equal(dev.cam_max_std, std.reshape(std.shape[0], -1).max(axis=1))


def test_repeatable_and_isolated():
  c, x, hold, _ = _case("tiny_rolling")
  x0 = mirror(synthetic.make_rig("tiny_rolling")).param_vec
  with Handle(c) as h:
    solves = [h.solve(x0, tr_solver=s).x for s in ("exact", "lsmr")]
    cov0 = h.covariance(x, hold=hold, cross=True)
    a = h.observation_covariance(x, hold=hold)
    b = h.observation_covariance(x, hold=hold)
    cov1 = h.covariance(x, hold=hold, cross=True)
    again = [h.solve(x0, tr_solver=s).x for s in ("exact", "lsmr")]
  for k in ("cov", "student", "cam_max_std"):
    assert np.array_equal(a[k], b[k], equal_nan=True), k
  assert a.trace == b.trace and a.sigma2 == b.sigma2
  for k in ("shared", "frames", "frame_shared", "std"):
    assert np.array_equal(cov0[k], cov1[k], equal_nan=True), k
  for p, q in zip(solves, again):
    assert np.array_equal(p, q)


def test_errors_leave_the_handle_usable():
  c, x, hold, _ = _case("tiny")
  with Handle(c) as h:
    with pytest.raises(McbaError, match=r"covariance: rank deficient at x\[\d+\] \(.+\); hold more parameters"):
      h.observation_covariance(x, hold=np.zeros(x.size, dtype=bool))
    assert np.isfinite(h.observation_covariance(x, hold=hold).trace)
  F = c.size.rig_poses
  with Handle(c, frame_range=(0, F // 2)) as h:
    with pytest.raises(McbaError, match="frame-sharded handle is not supported"):
      h.observation_covariance(x, hold=hold)
    assert h.n_residuals > 0 and h.device_info().startswith("gfx950")
  mask = np.zeros(c.valid.shape, dtype=bool)
  C0, F0, B0, _ = np.argwhere(c.valid)[0]
  mask[C0, F0, B0, np.flatnonzero(c.valid[C0, F0, B0])[:4]] = True   # 8 residuals against 6 pose parameters + the intrinsics
  few = c.copy(inlier_mask=mask)
  with Handle(few) as h:
    with pytest.raises(McbaError, match="m <= p_free"):
      h.observation_covariance(x, hold=hold)
    h.set_inliers(None)
    assert np.isfinite(h.observation_covariance(x, hold=hold).trace)


def test_calibration_api():
  c, x, hold, ref = _case("tiny_mixed")
  shape = c.valid.shape
  pc = c.prediction_covariance(hold=hold)
  assert pc.cov.shape == shape + (2, 2) and np.array_equal(pc.valid, c.valid) and pc.dof == ref["dof"]
  assert np.array_equal(pc.cov[..., 0, 1], pc.cov[..., 1, 0], equal_nan=True)
  st = c.studentized_error(hold=hold)
  assert st.error.shape == shape and np.array_equal(st.valid, c.valid)
  kept = c.reject_outliers_studentized(3.0, hold=hold)
  assert kept.inlier_mask.shape == shape and not (kept.inlier_mask & ~c.valid).any() and kept.inlier_mask.any()
  assert np.array_equal(kept.inlier_mask, (st.error < 3.0) & c.valid)
  records = []
  handler = logging.Handler()
  handler.emit = records.append
  logging.getLogger("calibration").addHandler(handler)
  try:
    logging.getLogger("calibration").setLevel(logging.INFO)
    c.report_prediction_uncertainty("test", hold=hold)
  finally:
    logging.getLogger("calibration").removeHandler(handler)
  lines = [r.getMessage() for r in records]
  assert len(lines) == c.size.cameras and all("predicted std" in l and "leverage" in l for l in lines), lines
