"""CPU: the oracle (oracle/restate.py) against the golden fixtures produced by the REAL reference."""
import numpy as np
import pytest

from oracle import restate
from util import ALL_CASES, load_golden, oracle, golden_jacobian


@pytest.mark.parametrize("name", ALL_CASES)
def test_oracle_matches_reference_fixtures(name):
  g, rig = load_golden(name)
  oc = oracle(rig)
  assert np.array_equal(oc.param_vec, g["x0"])                      # parameter packing, bit-exact
  assert np.array_equal(oc.inliers, g["inliers0"])
  r0 = oc.evaluate(g["x0"])
  assert np.array_equal(r0, g["r0"])                                # same numpy/scipy arithmetic -> bit-exact
  assert np.array_equal(oc.reprojection_error, g["err0"])
  assert restate.error_stats(oc.reprojection_error).rms == pytest.approx(float(g["rms0"]), rel=0, abs=0)


@pytest.mark.parametrize("name", ["tiny", "tiny_handeye", "tiny_edge"])
def test_oracle_bundle_adjust_matches_reference(name):
  g, rig = load_golden(name)
  oc = oracle(rig)
  out, res = oc.bundle_adjust(return_result=True)
  assert res.nfev == int(g["ba_nfev"]) and res.status == int(g["ba_status"])
  assert np.array_equal(res.x, g["ba_x_raw"])
  assert np.array_equal(out.param_vec, g["ba_x"])
  assert restate.error_stats(out.reprojection_error).rms == float(g["ba_rms"])


def test_oracle_sparsity_matches_fd_pattern():
  g, rig = load_golden("tiny_rolling")
  oc = oracle(rig)
  S = oc.sparsity_matrix.tocsr()
  J = golden_jacobian(g)
  assert S.shape == J.shape
  # every finite-difference non-zero lies inside the reference's sparsity pattern
  assert (abs(J) > 0).multiply(S == 0).nnz == 0


def test_oracle_outlier_loop_matches_reference():
  g, rig = load_golden("tiny")
  oc = oracle(rig)
  ao = oc.adjust_outliers(num_adjustments=3, select_outliers=restate.select_threshold(0.75, 5.0),
                          loss='linear', tolerance=1e-4)
  assert np.array_equal(ao.inliers, g["ao_inliers"])
  assert np.array_equal(ao.param_vec, g["ao_x"])
  assert restate.error_stats(ao.reprojection_error).rms == float(g["ao_rms"])


def full_golden(name):
  """Evaluation-only golden of a BASELINE configuration at its stated size (oracle/make_golden.py: run_full_case) and
  the rig regenerated from its seed; the observation table's checksums tie the two together."""
  import os
  from multical_amd import synthetic
  from util import GOLDEN
  g = dict(np.load(os.path.join(GOLDEN, f"{name}_full.npz"), allow_pickle=False))
  rig = synthetic.make_rig(str(g["config"]))
  assert tuple(g["shape"]) == rig.valid.shape and int(g["valid_count"]) == int(rig.valid.sum())
  assert float(g["points_sum"]) == rig.points.sum() and float(g["points_abs_sum"]) == np.abs(rig.points).sum()
  return g, rig


def check_full_residuals(g, tag, r, tol):
  """residual vector r at point `tag` ("0": x0, "1": the perturbed point) against the reference's checksums"""
  assert r.size == int(g[f"r{tag}_size"])
  stride = int(g[f"r{tag}_stride"])
  assert np.abs(r[:64] - g[f"r{tag}_head"]).max() <= tol
  assert np.abs(r[::stride] - g[f"r{tag}_sample"]).max() <= tol
  assert abs(r.sum() - float(g[f"r{tag}_sum"])) <= tol * r.size
  assert abs(np.abs(r).sum() - float(g[f"r{tag}_abs_sum"])) <= tol * r.size
  assert abs(r @ r - float(g[f"r{tag}_sq"])) <= 1e-12 * float(g[f"r{tag}_sq"]) + tol
  assert abs(np.dot(r, np.cos(np.arange(r.size) * 0.001)) - float(g[f"r{tag}_wsum"])) <= tol * r.size


@pytest.mark.parametrize("name", ["cfg3", "cfg4", "cfg5", "cfg5_handeye"])
def test_oracle_matches_reference_at_full_size(name):
  """BASELINE configs[2..4] at their stated size (8x500x2 rolling, 16x1000x5, 6x400x5 fisheye) and the 6x400x5 rig under the
  hand-eye motion model: the oracle's whole residual vector and error statistics against the real reference's checksums, at x0
  and at a perturbed point."""
  g, rig = full_golden(name)
  oc = oracle(rig)
  assert np.array_equal(oc.param_vec, g["x0"])
  for tag in ("0", "1"):
    x = g[f"x{tag}"]
    check_full_residuals(g, tag, oc.evaluate(x), 0.0 if tag == "0" else 1e-12)
    es = restate.error_stats(oc.with_param_vec(x).reprojection_error)
    assert es.n == int(g[f"n{tag}"])
    assert es.rms == pytest.approx(float(g[f"rms{tag}"]), rel=1e-14)
    assert np.allclose(es.quantiles, g[f"quantiles{tag}"], rtol=1e-13, atol=0)


@pytest.mark.parametrize("name", ["tiny_mixed", "tiny_fishmix5"])
def test_oracle_on_a_mixed_model_rig_matches_the_reference_including_its_failure(name):
  """Cameras of different distortion models in one rig (5 / 8 / 14 / 4 coefficients): the reference evaluates residuals
  and errors, but its bundle_adjust raises -- sparsity_matrix reshapes the ragged cameras block (calibration.py:179).  The
  oracle reproduces both facts (tests/golden/tiny_mixed.npz records the reference's values and its exception)."""
  g, rig = load_golden(name)   # (tiny_fishmix5: 5- / 8-coefficient pinhole + fisheye cameras in one rig)
  oc = oracle(rig)
  assert np.array_equal(oc.param_vec, g["x0"]) and np.array_equal(oc.inliers, g["inliers0"])
  assert np.array_equal(oc.evaluate(g["x0"]), g["r0"])
  assert np.array_equal(oc.reprojection_error, g["err0"])
  assert str(g["ba_error"]).startswith("ValueError: cannot reshape array")
  with pytest.raises(ValueError, match="cannot reshape array"):
    oc.bundle_adjust()


def test_scipys_lsmr_step_is_not_reproducible_beyond_rounding_noise():
  """Why two implementations of the reference's solver cannot agree step by step: the trust-region step of scipy's TRF is
  lsmr(J_h, f, damp) stopped at atol = btol = 1e-6 or at min(m, n) iterations (trf.py:481).  On the reference's own (finite-
  difference) Jacobian of a small rig, perturbing the matrix entries by 1e-15 RELATIVE -- one rounding error -- moves scipy's own
  LSMR solution by more than 1e-5 relative (the Golub-Kahan vectors lose orthogonality; weakly determined components carry the
  difference).  The end point of the reference is therefore defined to its measured spread (`*_pert_*` of the fixtures), and
  the device LSMR mode is held to that, not to bit-level agreement with scipy's trajectory."""
  from scipy.sparse import diags
  from scipy.sparse.linalg import lsmr
  from util import golden_jacobian
  g, rig = load_golden("tiny_thin_prism")
  J = golden_jacobian(g).tocsr()
  s = np.sqrt(np.asarray(J.multiply(J).sum(axis=0)).ravel())
  s[s == 0] = 1
  A = J @ diags(1 / s)
  x0, istop0, itn0 = lsmr(A, g["r0"], damp=np.sqrt(3e-4))[:3]
  rng = np.random.default_rng(0)
  Ap = A.copy()
  Ap.data = Ap.data * (1 + 1e-15 * rng.standard_normal(Ap.data.size))
  x1, istop1, itn1 = lsmr(Ap, g["r0"], damp=np.sqrt(3e-4))[:3]
  assert (istop0, itn0) == (istop1, itn1)
  assert np.linalg.norm(x1 - x0) / np.linalg.norm(x0) > 1e-5
