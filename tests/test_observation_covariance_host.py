"""No GPU: the boundary of the per-observation prediction covariance (mcba_observation_covariance) -- the symbol,
the refusal that needs no device, and the numpy statement of the studentised error the GPU tests compare against."""
import os

import numpy as np
import pytest

from multical_amd import _lib, synthetic
from util import mirror

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT_FIT = 1e-9


def max_eig(uu, uv, vv):
  """larger eigenvalue of (uu uv; uv vv): the five operations include/mcba.h states, each rounded once"""
  return 0.5 * (uu + vv) + np.sqrt((0.5 * (uu - vv)) ** 2 + uv ** 2)


def studentized(cov, r, sigma2, inlier):
  """d = sqrt(r^T Omega^-1 r), Omega = sigma2 I - C (inlier) / sigma2 I + C (not an inlier); +inf where the larger eigenvalue of
  an inlier's C / sigma2 is >= 1 - 1e-9; NaN where C is NaN.  cov [..., 3] = (uu, uv, vv), r [..., 2], inlier [...] bool."""
  cov, r, inlier = np.asarray(cov, dtype=np.float64), np.asarray(r, dtype=np.float64), np.asarray(inlier, dtype=bool)
  uu, uv, vv = cov[..., 0], cov[..., 1], cov[..., 2]
  sg = np.where(inlier, -1.0, 1.0)
  with np.errstate(invalid="ignore", divide="ignore"):
    a, b, c = sigma2 + sg * uu, sg * uv, sigma2 + sg * vv
    d2 = (c * r[..., 0] ** 2 - 2.0 * b * r[..., 0] * r[..., 1] + a * r[..., 1] ** 2) / (a * c - b * b)
    d = np.sqrt(np.maximum(d2, 0.0))
    d = np.where(inlier & (max_eig(uu, uv, vv) >= (1.0 - EXACT_FIT) * sigma2), np.inf, d)
  return np.where(np.isnan(uu) | np.isnan(uv) | np.isnan(vv), np.nan, d)


def test_symbol_is_declared():
  names = [s[0] for s in _lib.SYMBOLS]
  assert "mcba_observation_covariance" in names
  sig = dict((s[0], s) for s in _lib.SYMBOLS)["mcba_observation_covariance"]
  assert len(sig[2]) == 10
  header = open(os.path.join(ROOT, "include", "mcba.h")).read()
  assert "int32_t mcba_observation_covariance(mcba_handle h, const double* x, const uint8_t* hold, double sigma2," in header
  assert _lib.MCBA_VERSION == 3   # no struct changes with the new entry point


def test_boards_block_asks_for_an_explicit_hold_before_any_device_work(monkeypatch):
  c = mirror(synthetic.make_rig("tiny")).enable(boards=True)
  from multical_amd import calibration

  def no_handle(*a, **k):
    raise AssertionError("device work before the refusal")
  monkeypatch.setattr(calibration.Calibration, "_handle", no_handle)
  for call in (c.prediction_covariance, c.studentized_error, lambda: c.reject_outliers_studentized(3.0),
               c.report_prediction_uncertainty):
    with pytest.raises(ValueError, match="explicit hold"):
      call()


def test_studentized_error_of_hand_made_blocks():
  s2 = 2.0
  # no prediction uncertainty: the plain error in units of sigma, inlier or not
  for inl in (True, False):
    assert studentized([0.0, 0.0, 0.0], [3.0, 4.0], s2, inl) == pytest.approx(5.0 / np.sqrt(2.0), rel=1e-15)
  # diagonal C: inliers divide by sigma2 - C, the others by sigma2 + C
  C = [0.5, 0.0, 1.0]
  assert studentized(C, [3.0, 4.0], s2, True) == pytest.approx(np.sqrt(9.0 / 1.5 + 16.0 / 1.0), rel=1e-15)
  assert studentized(C, [3.0, 4.0], s2, False) == pytest.approx(np.sqrt(9.0 / 2.5 + 16.0 / 3.0), rel=1e-15)
  # a full block against numpy's inverse
  C = np.array([0.6, -0.3, 0.9])
  r = np.array([0.7, -1.1])
  M = np.array([[C[0], C[1]], [C[1], C[2]]])
  for inl, Om in ((True, s2 * np.eye(2) - M), (False, s2 * np.eye(2) + M)):
    assert studentized(C, r, s2, inl) == pytest.approx(np.sqrt(r @ np.linalg.solve(Om, r)), rel=1e-13)
  # the +inf rule: larger eigenvalue of H = C / sigma2 at 1 (fitted exactly) -- for inliers only
  assert studentized([s2, 0.0, 0.1], [0.1, 0.1], s2, True) == np.inf
  assert studentized([s2 * (1.0 - 5e-10), 0.0, 0.1], [0.1, 0.1], s2, True) == np.inf
  assert np.isfinite(studentized([s2 * (1.0 - 1e-8), 0.0, 0.1], [0.1, 0.1], s2, True))
  assert np.isfinite(studentized([s2, 0.0, 0.1], [0.1, 0.1], s2, False))
  # an eigenvalue at 1 off the axes
  assert studentized([0.5 * s2, 0.5 * s2, 0.5 * s2], [1.0, 0.0], s2, True) == np.inf
  # the NaN rule, and arrays
  assert np.isnan(studentized([np.nan, np.nan, np.nan], [1.0, 1.0], s2, True))
  out = studentized([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [s2, 0.0, 0.0]], [[1.0, 0.0]] * 3, s2, [True, False, True])
  assert out[0] == pytest.approx(1.0 / np.sqrt(2.0)) and np.isnan(out[1]) and out[2] == np.inf


def test_max_eig_is_the_larger_eigenvalue():
  rng = np.random.default_rng(3)
  for _ in range(20):
    A = rng.normal(size=(2, 3))
    M = A @ A.T
    assert max_eig(M[0, 0], M[0, 1], M[1, 1]) == pytest.approx(np.linalg.eigvalsh(M)[1], rel=1e-13)
