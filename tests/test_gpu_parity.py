"""GPU (MI355X): parity of the HIP back-end, called through the C ABI (libmcba.so), against
  * the golden fixtures produced by the REAL reference (tests/golden/*.npz, oracle/make_golden.py),
  * the oracle (oracle/restate.py) on the same seeded inputs,
  * the product's own device functions compiled for the host (tests/hostmath) for kernel-structure checks.
Tolerances: residuals / errors 1e-9 px (north star), Jacobian vs the reference's finite differences 5e-5 relative
(FD truncation), normal equations 1e-12 relative, solved RMS see each test.
"""
import numpy as np
import pytest

from multical_amd import synthetic, calibration
from multical_amd.backend import Handle, mfma_probe
from oracle import restate
from hostmath_lib import HostMath
from util import SMALL_CASES, ALL_CASES, load_golden, mirror, oracle, golden_jacobian, rel_col_error

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _exact_step_solver():
  """This module pins the properties of the EXACT-step solver (solver = "native": converged optima, fused outlier loop, timing
  paths) unless a test names another one; the product default is "lsmr" (tests/test_gpu_lsmr.py, test_device_lsmr_mode_*)."""
  prev = calibration.set_solver("native")
  yield
  calibration.set_solver(prev)


def rms_of(h, x):
  e, v = h.reprojection_error(x)
  return float(np.sqrt(np.mean(e[v] ** 2)))


def test_device_is_gfx950_and_library_loaded():
  with Handle(mirror(synthetic.make_rig("tiny"))) as h:
    assert h.device_info().startswith("gfx950")


def test_mfma_f64_operand_layout():
  """v_mfma_f64_16x16x4_f64: lane l feeds A[l&15][l>>4], B[l>>4][l&15]; D row = (l>>4) + 4 reg, col = l&15."""
  rng = np.random.default_rng(0)
  V = rng.normal(size=(4, 32))          # asymmetric operand pair: a swapped row/col map cannot pass
  out = mfma_probe(V)
  assert np.abs(out - V[:, :16].T @ V[:, 16:]).max() < 1e-14


@pytest.mark.parametrize("name", ALL_CASES)
def test_residuals_match_reference(name):
  g, rig = load_golden(name)
  c = mirror(rig)
  with Handle(c) as h:
    assert h.n_params == g["x0"].size and h.n_residuals == g["r0"].size
    r = h.residuals(g["x0"])
    assert np.abs(r - g["r0"]).max() < 1e-9                       # bit-identical indexing, values to 1e-9 px
    err, valid = h.reprojection_error(g["x0"])
    assert valid.sum() == g["err0"].size
    assert np.abs(err[valid] - g["err0"]).max() < 1e-9
    # at the reference's solution, against the oracle evaluated at the same point
    oc = oracle(rig)
    assert np.abs(h.residuals(g["ba_x_raw"]) - oc.evaluate(g["ba_x_raw"])).max() < 1e-9
    assert abs(rms_of(h, g["ba_x_raw"]) - float(g["ba_rms"])) < 1e-9
    # projections of every slot (Calibration.reprojected)
    proj, _ = oc.with_param_vec(g["x0"]).reprojected()
    assert np.abs(h.project(g["x0"]) - proj)[valid].max() < 1e-9


@pytest.mark.parametrize("name", SMALL_CASES)
def test_jacobian_matches_reference_finite_differences(name):
  g, rig = load_golden(name)
  c = mirror(rig)
  with Handle(c) as h:
    J = h.jacobian(g["x0"])
  Jfd = golden_jacobian(g)
  assert J.shape == Jfd.shape
  assert rel_col_error(J, Jfd) < 5e-5
  Jh = HostMath(c).jacobian(g["x0"])
  assert np.abs((J - Jh)).max() <= 1e-11 * np.abs(Jh).max()
  S = oracle(rig).sparsity_matrix.tocsr()
  assert (abs(J) > 0).multiply(S == 0).nnz == 0                   # inside the reference's sparsity pattern


@pytest.mark.parametrize("mfma", [1, 0])
@pytest.mark.parametrize("name", ALL_CASES)
def test_fused_normal_equations(name, mfma):
  """k_linearize + assembly == J^T J, J^T f of evaluate(); MFMA and plain-FMA accumulation agree."""
  g, rig = load_golden(name)
  c = mirror(rig)
  hm = HostMath(c)
  Hh, gh, costh = hm.normal_equations(g["x0"])
  with Handle(c) as h:
    h.set_mfma(mfma)
    cost, grad, diag = h.normal_equations(g["x0"])
    H = h.dense_hessian()
  assert cost == pytest.approx(0.5 * g["r0"] @ g["r0"], rel=1e-12)
  assert np.abs(grad - gh).max() <= 1e-12 * np.abs(gh).max()
  assert np.abs(H - Hh).max() <= 1e-12 * np.abs(Hh).max()
  assert np.abs(diag - np.diag(Hh)).max() <= 1e-12 * np.abs(Hh).max()
  assert np.array_equal(H, H.T)


def test_device_resident_evaluation_equals_host_boundary_evaluation():
  """mcba_normal_equations_device (x, tables and results stay in HBM: the bench step and the solver's own evaluations)
  reproduces mcba_normal_equations bit for bit."""
  g, rig = load_golden("tiny_rolling")
  with Handle(mirror(rig)) as h:
    cost, grad, diag = h.normal_equations(g["x0"])
    H0 = h.dense_hessian()
    for _ in range(3):
      h.normal_equations_device()
    h.synchronize()
    H1 = h.dense_hessian()
    assert np.array_equal(H0, H1)
    gn0, gh0, _ = h.debug_gn_step(1e-3)
    cost2, grad2, diag2 = h.normal_equations(g["x0"])
    assert cost2 == cost and np.array_equal(grad2, grad) and np.array_equal(diag2, diag)


@pytest.mark.parametrize("loss,f_scale", [("soft_l1", 1.5), ("huber", 2.0), ("cauchy", 1.0), ("arctan", 3.0)])
def test_robust_loss_normal_equations(loss, f_scale):
  from scipy.optimize._lsq.least_squares import construct_loss_function
  from scipy.optimize._lsq.common import scale_for_robust_loss_function
  g, rig = load_golden("tiny_rolling")
  c = mirror(rig)
  with Handle(c) as h:
    J = h.jacobian(g["x0"]).toarray()
    f = h.residuals(g["x0"])
    cost, grad, diag = h.normal_equations(g["x0"], loss=loss, f_scale=f_scale)
    H = h.dense_hessian()
  rho = construct_loss_function(f.size, loss, f_scale)(f)
  Js, fs = scale_for_robust_loss_function(J.copy(), f.copy(), rho)
  assert cost == pytest.approx(0.5 * np.sum(rho[0]), rel=1e-12)
  assert np.abs(H - Js.T @ Js).max() <= 1e-11 * np.abs(H).max()
  assert np.abs(grad - Js.T @ fs).max() <= 1e-11 * np.abs(grad).max()


@pytest.mark.parametrize("name", ["tiny", "tiny_rolling", "tiny_handeye", "tiny_edge", "cfg1"])
def test_schur_cholesky_step(name):
  """(D H D + reg I)^-1 D g from the Schur / Cholesky kernels == dense numpy solve."""
  g, rig = load_golden(name)
  c = mirror(rig)
  hm = HostMath(c)
  Hh, gh, _ = hm.normal_equations(g["x0"])
  with Handle(c) as h:
    h.normal_equations(g["x0"])
    for reg in (1e-2, 1e-5):
      gn, ghs, si = h.debug_gn_step(reg)
      si_ref = np.sqrt(np.diag(Hh))
      si_ref[si_ref == 0] = 1
      d = 1 / si_ref
      ref = np.linalg.solve(Hh * d[:, None] * d[None, :] + reg * np.eye(h.n_params), d * gh)
      assert np.abs(si - si_ref).max() <= 1e-12 * si_ref.max()
      assert np.abs(gn - ref).max() <= 1e-8 * np.abs(ref).max()
      # the trust-region driver takes the quadratic forms of the 2-D subspace from (H_h + reg I) gn = g_h instead of
      # a second pass over H (mcba_solve): check the identities on the device step against the dense Hessian
      Hs = Hh * d[:, None] * d[None, :]
      q01, q11 = ghs @ Hs @ gn, gn @ Hs @ gn
      assert abs((ghs @ ghs - reg * (ghs @ gn)) - q01) <= 1e-9 * abs(q01)
      assert abs((ghs @ gn - reg * (gn @ gn)) - q11) <= 1e-9 * abs(q11)


@pytest.mark.parametrize("name", ["cfg1", "tiny_handeye", "tiny_fixintr"])
def test_bundle_adjust_matches_reference_rms(name):
  """Well-conditioned cases (BASELINE configs[0] = cfg1): final reprojection RMS within 1e-6 px of the reference at the
  reference's default tolerance, same number of function evaluations."""
  g, rig = load_golden(name)
  c = mirror(rig)
  out, res = c.bundle_adjust(return_result=True)
  rms = calibration.error_stats(out.reprojection_error).rms
  assert abs(rms - float(g["ba_rms"])) < 1e-6
  assert res.status == int(g["ba_status"]) and res.nfev == int(g["ba_nfev"])
  assert res.cost == pytest.approx(float(g["ba_cost"]), rel=1e-6)


@pytest.mark.parametrize("name", ["tiny", "tiny_rolling", "tiny_fisheye", "tiny_edge", "tiny_rational", "tiny_thin_prism",
                                  "tiny_tilted"])
def test_bundle_adjust_reaches_lower_or_equal_cost(name):
  """Free intrinsics + 1 % gross outliers: the reference's LSMR-truncated steps stop (ftol=1e-4) before convergence,
  so RMS parity at default tolerance is limited to ~1e-3 px; the exact normal-equation solve must not be worse."""
  g, rig = load_golden(name)
  c = mirror(rig)
  out, res = c.bundle_adjust(return_result=True)
  assert res.status in (0, 2, 3, 4)          # over-parameterised distortion models may keep improving until max_nfev
  assert res.cost <= float(g["ba_cost"]) * (1 + 1e-9)
  if name in ("tiny", "tiny_rolling", "tiny_fisheye", "tiny_edge"):
    assert abs(calibration.error_stats(out.reprojection_error).rms - float(g["ba_rms"])) < 5e-3


@pytest.mark.parametrize("name,noise,outliers,seed", [
    ("tiny", 0.5, 0.0, 11), ("tiny", 0.5, 0.0, 12), ("tiny", 0.1, 0.05, 13), ("tiny_rolling", 0.2, 0.03, 11),
    ("tiny_fisheye", 0.1, 0.01, 11), ("tiny_fisheye", 0.4, 0.0, 12), ("tiny_handeye", 0.3, 0.02, 11),
    ("tiny_handeye", 0.3, 0.02, 12), ("tiny_handeye", 1.0, 0.0, 13)])
def test_randomised_rigs_against_the_oracle(name, noise, outliers, seed):
  """Fresh synthetic rigs (seeds, noise levels and outlier fractions that no fixture uses): residuals at the start point
  within 1e-9 px of the oracle, analytic gradient == J^T r of the oracle's finite-difference-free check (3-point), and
  the HIP solve ends at a cost not above the oracle's (= the reference's) bundle_adjust on the same rig."""
  rig = synthetic.make_rig(name, seed=seed, noise=noise, outlier_frac=outliers)
  c = mirror(rig)
  oc = restate.from_rig(rig)
  x0 = c.param_vec
  assert np.array_equal(x0, oc.param_vec)
  with Handle(c) as h:
    r = h.residuals(x0)
    r_ref = oc.evaluate(x0)
    assert r.shape == r_ref.shape and np.abs(r - r_ref).max() < 1e-9
    cost, grad, _ = h.normal_equations(x0)
    assert cost == pytest.approx(0.5 * r_ref @ r_ref, rel=1e-12)
    # directional derivative of the oracle's cost along a random direction == grad . direction (central differences)
    rng = np.random.default_rng(seed)
    dvec = rng.normal(size=x0.size) * 1e-6
    f = lambda x: 0.5 * np.sum(oc.evaluate(x) ** 2)
    num = (f(x0 + dvec) - f(x0 - dvec)) / 2
    assert num == pytest.approx(grad @ dvec, rel=2e-5, abs=1e-9 * abs(cost))
    res = h.solve(x0)
  ref = oc.bundle_adjust()
  ref_cost = 0.5 * np.sum(ref.evaluate(ref.param_vec) ** 2)
  assert res.status in (0, 1, 2, 3, 4)   # 0: the reference exhausts its 100 evaluations on the same rig too (rolling, 3 % outliers)
  assert res.cost <= ref_cost * (1 + 1e-9)


@pytest.mark.parametrize("name", ["tiny_bigboard", "tiny_manypairs", "tiny_mixed", "tiny_fishmix5"])
def test_rigs_beyond_the_former_limits_against_the_oracle(name):
  """Rigs the reference accepts and earlier versions of mcba_create rejected: a board with more than 512 points (816-corner
  charuco next to an 81-corner one, rolling shutter), more than 128 (camera, board) pairs (16 cameras x 10 boards),
  cameras of different distortion models in one rig (5 / 8 / 14 / 4 coefficients: a ragged cameras block), and pinhole AND
  fisheye cameras in one rig (round 4; 5 / 8 coefficients + two fisheye cameras: ragged as well).  Against the
  oracle (pinned bit for bit to the reference): residuals, errors, the analytic Jacobian inside the reference's sparsity
  pattern and equal to 3-point differences of the oracle, the fused normal equations == J^T J / J^T r, and the solve."""
  from scipy.optimize._numdiff import approx_derivative, group_columns
  from scipy.sparse import csr_matrix
  rig = synthetic.make_rig(name)
  c = mirror(rig)
  oc = restate.from_rig(rig)
  x0 = c.param_vec
  assert np.array_equal(x0, oc.param_vec)
  with Handle(c) as h:
    assert h.n_params == x0.size
    r = h.residuals(x0)
    r_ref = oc.evaluate(x0)
    assert r.shape == r_ref.shape and np.abs(r - r_ref).max() < 1e-9
    err, valid = h.reprojection_error(x0)
    eo, vo = oc.reprojection_error_table()
    assert np.array_equal(valid, vo) and np.abs(err[vo] - eo[vo]).max() < 1e-9
    J = h.jacobian(x0)
    if name in ("tiny_mixed", "tiny_fishmix5"):
      # the reference's own sparsity_matrix reshapes the cameras block to [C, -1] (calibration.py:179) and therefore
      # RAISES for a ragged block -- its bundle_adjust cannot run on such a rig at all (the fixture records the exception);
      # the oracle restates that line.  What the reference CAN compute is pinned by the fixture: residuals, errors and a
      # dense 2-point Jacobian of its `evaluate`; the analytic Jacobian is also checked against dense 3-point differences.
      g, _ = load_golden(name)
      assert np.array_equal(x0, g["x0"]) and str(g["ba_error"]).startswith("ValueError")
      assert np.abs(r - g["r0"]).max() < 1e-9 and np.abs(err[valid] - g["err0"]).max() < 1e-9
      assert rel_col_error(J, csr_matrix(g["J_dense"])) < 5e-5
      with pytest.raises(ValueError):
        oc.sparsity_matrix
      J3 = csr_matrix(approx_derivative(oc.evaluate, x0, method='3-point'))
      assert J.shape == J3.shape and rel_col_error(J, J3) < 2e-7
    else:
      S = csr_matrix(oc.sparsity_matrix)
      assert J.shape == S.shape and (abs(J) > 0).multiply(S == 0).nnz == 0        # inside the reference's pattern
      if name != "tiny_manypairs":                                                 # (138 k x 376: minutes of oracle time)
        J3 = csr_matrix(approx_derivative(oc.evaluate, x0, method='3-point', sparsity=(S, group_columns(S))))
        assert rel_col_error(J, J3) < 2e-7
    cost, grad, diag = h.normal_equations(x0)
    assert cost == pytest.approx(0.5 * r_ref @ r_ref, rel=1e-12)
    assert np.abs(J.T @ r - grad).max() <= 1e-11 * np.abs(grad).max()
    assert np.abs(np.asarray(J.multiply(J).sum(axis=0)).ravel() - diag).max() <= 1e-11 * diag.max()
    if x0.size <= 600:
      H = h.dense_hessian()
      JtJ = (J.T @ J).toarray()
      assert np.abs(H - JtJ).max() <= 1e-11 * np.abs(JtJ).max()
    rng = np.random.default_rng(5)
    dvec = rng.normal(size=x0.size) * 1e-6
    f = lambda x: 0.5 * np.sum(oc.evaluate(x) ** 2)
    assert (f(x0 + dvec) - f(x0 - dvec)) / 2 == pytest.approx(grad @ dvec, rel=2e-5, abs=1e-9 * abs(cost))
    res = h.solve(x0)
    assert res.status in (1, 2, 3, 4) and res.cost < 0.05 * res.initial_cost
    # the solution evaluated by the oracle: same cost and RMS as the device reports
    ro = oc.evaluate(res.x)
    assert 0.5 * ro @ ro == pytest.approx(res.cost, rel=1e-10)
    assert abs(rms_of(h, res.x) - restate.error_stats(oc.with_param_vec(res.x).reprojection_error).rms) < 1e-9
    # first-order optimality (scaled gradient) at the solution (the mixed rig contains a `tilted` camera: a flat valley in
    # which ftol = 1e-4 stops early, like tests/test_gpu_protocol.py FLAT_VALLEY -- checked after a tight solve there)
    xs = res.x if name not in ("tiny_mixed", "tiny_fishmix5") else h.solve(res.x, tolerance=1e-13, xtol=1e-13, gtol=1e-13, max_iterations=300).x
    c2, g2, d2 = h.normal_equations(xs)
    si = np.sqrt(d2); si[si == 0] = 1
    assert np.abs(g2 / si).max() < 1e-3 * np.sqrt(2 * c2)
  # the complete outlier loop on the device ends at the noise level
  from multical_amd import Workspace
  out = Workspace(c).calibrate(cameras=True)
  assert 0.25 < out.error_statistics(True).rms < 0.32


@pytest.mark.parametrize("name", ["tiny", "tiny_rolling", "tiny_handeye", "tiny_fisheye", "tiny_edge", "cfg1"])
def test_outlier_loop_matches_reference(name):
  """Workspace.calibrate's sequence (3 x {reject at 5 x q75, bundle_adjust}, workspace.py:228-247):
  identical inlier masks after the three rounds, and a final reprojection RMS (all valid points AND inliers) within
  1e-6 px of the CONVERGED optimum of the reference's own residual function on that inlier set (`ao_tight_*`:
  scipy exact trust-region solver polishing the reference's result, oracle/make_golden.py).  The reference's own
  default-tolerance end point is itself 1e-7 ... 1e-4 px away from that optimum (LSMR steps + ftol=1e-4)."""
  g, rig = load_golden(name)
  c = mirror(rig)
  ao = c.adjust_outliers(num_adjustments=3, select_outliers=calibration.select_threshold(0.75, 5.0), loss='linear',
                         tolerance=1e-4)
  assert np.array_equal(ao.inliers, g["ao_inliers"])
  rms_all = calibration.error_stats(ao.reprojection_error).rms
  rms_inl = calibration.error_stats(ao.reprojection_inliers).rms
  assert abs(rms_inl - float(g["ao_tight_rms_inliers"])) < 1e-6
  assert abs(rms_all - float(g["ao_tight_rms"])) < 1e-6
  # distance to the reference's (not fully converged) default-tolerance result
  assert abs(rms_inl - float(g["ao_rms_inliers"])) < 1e-4
  assert abs(rms_all - float(g["ao_rms"])) < 1e-3
  tight = ao.bundle_adjust(tolerance=1e-13, xtol=1e-13, gtol=1e-13, max_iterations=300)
  assert abs(calibration.error_stats(tight.reprojection_inliers).rms - float(g["ao_tight_rms_inliers"])) < 1e-7
  assert abs(calibration.error_stats(tight.reprojection_error).rms - float(g["ao_tight_rms"])) < 1e-6


@pytest.mark.parametrize("name", ["tiny", "tiny_rolling", "tiny_handeye", "tiny_fisheye", "tiny_edge", "cfg1"])
def test_outlier_loop_matches_reference_under_the_default_solver(name):
  """The same loop (Calibration.adjust_outliers, calibration.py:254-268) under the PRODUCT DEFAULT, solver = "lsmr" -- scipy's TRF + LSMR steps
  restated on the device: the reference's inlier mask after three rounds (up to what the reference's own perturbed re-runs flip) and the
  reference's OWN default-tolerance end point (not the converged optimum the exact-step solver is held to above) within max(1e-6 px, 3 x the
  reference's spread)."""
  g, rig = load_golden(name)
  c = mirror(rig)
  prev = calibration.set_solver("lsmr")
  try:
    ao = c.adjust_outliers(num_adjustments=3, select_outliers=calibration.select_threshold(0.75, 5.0), loss='linear', tolerance=1e-4)
  finally:
    calibration.set_solver(prev)
  allowed = int(g["ao_pert_mask_diff"].max()) if "ao_pert_mask_diff" in g else 0
  diff = int((ao.inliers != g["ao_inliers"]).sum())
  assert diff <= allowed, (diff, allowed)
  spread = float(np.abs(g["ao_pert_rms_inliers"] - g["ao_rms_inliers"]).max())
  rms_inl = calibration.error_stats(ao.reprojection_inliers).rms
  assert abs(rms_inl - float(g["ao_rms_inliers"])) <= max(1e-6, 3 * spread), (rms_inl - float(g["ao_rms_inliers"]), spread)
  if spread < 3e-7:
    assert diff == 0


def test_workspace_calibrate_entry_point():
  from multical_amd import Workspace
  g, rig = load_golden("cfg1")
  ws = Workspace(mirror(rig))
  calib = ws.calibrate(cameras=False)
  assert ws.latest_calibration is calib
  assert abs(calibration.error_stats(calib.reprojection_error).rms - float(g["ao_rms"])) < 1e-6


def test_full_size_properties_cfg2():
  """BASELINE configs[1] at full size: size-independent properties (the oracle needs minutes there)."""
  rig = synthetic.make_rig("cfg2")
  c = mirror(rig)
  x0 = c.param_vec
  with Handle(c) as h:
    r = h.residuals(x0)
    cost, grad, diag = h.normal_equations(x0)
    assert cost == pytest.approx(0.5 * r @ r, rel=1e-12)                       # fused pass == residual pass
    J = h.jacobian(x0)
    assert np.abs(J.T @ r - grad).max() <= 1e-11 * np.abs(grad).max()          # J^T f
    assert np.abs(np.asarray(J.multiply(J).sum(axis=0)).ravel() - diag).max() <= 1e-11 * diag.max()
    # a subset of frames evaluated by the oracle
    oc = restate.from_rig(rig)
    sub = oc.evaluate(x0)
    assert np.abs(sub - r).max() < 1e-9
    res = h.solve(x0)
    assert res.status in (1, 2, 3, 4) and res.cost < 0.02 * res.initial_cost
    # gradient vanishes at the solution (first-order optimality in the scaled norm)
    _, g2, d2 = h.normal_equations(res.x)
    si = np.sqrt(d2); si[si == 0] = 1
    assert np.abs(g2 / si).max() < 1e-3 * np.sqrt(2 * res.cost)


@pytest.mark.parametrize("name", ["cfg3", "cfg4", "cfg5", "cfg5_handeye"])
def test_full_size_properties(name):
  """BASELINE configs[2..4] AT THEIR STATED SIZE (rolling shutter 8x500x2 = the rig bench.py measures, 16x1000x5,
  fisheye 6x400x5) and the 6x400x5 rig under the hand-eye motion model (no per-frame block), pinned to the real reference: tests/golden/<name>_full.npz holds checksums, a strided
  sample and the error statistics of the reference's `evaluate` / `reprojection_error` at x0 and at a perturbed point,
  and a central-difference directional derivative of its cost (oracle/make_golden.py: run_full_case).  The WHOLE
  residual vector and error table are additionally compared with the oracle (which reproduces the reference bit for
  bit at these sizes: tests/test_oracle.py::test_oracle_matches_reference_at_full_size)."""
  from test_oracle import full_golden, check_full_residuals
  g, rig = full_golden(name)
  c = mirror(rig)
  x0 = c.param_vec
  assert np.array_equal(x0, g["x0"])                                           # parameter packing at full size
  oc = restate.from_rig(rig)
  with Handle(c) as h:
    for tag in ("0", "1"):
      x = g[f"x{tag}"]
      r = h.residuals(x)
      check_full_residuals(g, tag, r, 1e-9)                                    # reference checksums + strided sample
      assert np.abs(r - oc.evaluate(x)).max() < 1e-9                           # every residual, reference order
      err, valid = h.reprojection_error(x)
      eo, vo = oc.with_param_vec(x).reprojection_error_table()
      assert np.array_equal(valid.astype(bool), vo)
      assert np.abs(err[vo] - eo[vo]).max() < 1e-9                             # every table slot
      mse, rms, q, n = h.error_stats(x)
      assert n == int(g[f"n{tag}"]) and abs(rms - float(g[f"rms{tag}"])) < 1e-9
      assert np.abs(q - g[f"quantiles{tag}"]).max() < 1e-9
    r = h.residuals(x0)
    cost, grad, diag = h.normal_equations(x0)
    assert cost == pytest.approx(0.5 * float(g["r0_sq"]), rel=1e-12)           # fused pass == the reference's cost
    # gradient of the fused pass against the reference's central-difference directional derivative of its cost
    assert grad @ g["v"] == pytest.approx(float(g["dd"]), rel=1e-6)
    J = h.jacobian(x0)
    assert np.abs(J.T @ r - grad).max() <= 1e-10 * np.abs(grad).max()          # J^T f
    assert np.abs(np.asarray(J.multiply(J).sum(axis=0)).ravel() - diag).max() <= 1e-10 * diag.max()
    res = h.solve(x0)
    assert res.status in (1, 2, 3, 4) and res.cost < 0.02 * res.initial_cost
    # gradient vanishes at the solution (first-order optimality in the scaled norm)
    _, g2, d2 = h.normal_equations(res.x)
    si = np.sqrt(d2); si[si == 0] = 1
    assert np.abs(g2 / si).max() < 1e-3 * np.sqrt(2 * res.cost)
    # the solution evaluated by the oracle: same RMS as the device reports
    e, v = h.reprojection_error(res.x)
    rms_dev = float(np.sqrt(np.mean(e[v] ** 2)))
    assert abs(rms_dev - restate.error_stats(oc.with_param_vec(res.x).reprojection_error).rms) < 1e-9
  # the whole Workspace.calibrate sequence (outlier loop on the device): the inlier RMS ends at the noise level
  from multical_amd import Workspace
  out = Workspace(c).calibrate(cameras=rig.optimize["cameras"], camera_poses=rig.optimize["camera_poses"])
  assert 0.27 < out.error_statistics(True).rms < 0.30                          # synthetic noise: 0.2 px per axis


def test_non_finite_start_raises_value_error():
  rig = synthetic.make_rig("tiny")
  c = mirror(rig)
  x0 = c.param_vec.copy()
  x0[0] = np.nan
  with Handle(c) as h:
    with pytest.raises(ValueError, match="not finite"):
      h.solve(x0)


def test_empty_inlier_set_and_ragged_boards():
  """edge cases: a frame without observations, an invalid camera / frame (identity pose, zero Jacobian columns),
  boards of different sizes padded to P, and an all-false inlier mask."""
  g, rig = load_golden("tiny_edge")
  c = mirror(rig)
  with Handle(c) as h:
    cost, grad, diag = h.normal_equations(g["x0"])
    F = rig.valid.shape[1]
    off = 6 * 3 + 6 * 2
    assert np.all(grad[off + 6 * 3: off + 6 * 4] == 0) and np.all(diag[off + 6 * 3: off + 6 * 4] == 0)   # invalid frame 3
    assert np.all(grad[off + 6 * 5: off + 6 * 6] == 0)                                                     # empty frame 5
    assert np.all(grad[12:18] == 0)                                                                        # invalid camera 2
    res = h.solve(g["x0"])
    assert np.array_equal(res.x[off + 18: off + 24], g["x0"][off + 18: off + 24])                          # zero step there
    h.set_inliers(np.zeros(rig.valid.shape, dtype=bool))
    assert h.n_residuals == 0
    assert h.residuals(g["x0"]).size == 0
  g2, rig2 = load_golden("tiny_rolling")     # charuco_10x10 (81 pts) + aprilgrid (324 pts): ragged boards
  with Handle(mirror(rig2)) as h:
    assert np.abs(h.residuals(g2["x0"]) - g2["r0"]).max() < 1e-9


@pytest.mark.parametrize("name", ["tiny_rolling", "tiny_edge", "cfg1"])
def test_device_outlier_statistics_match_numpy(name):
  """mcba_error_stats / mcba_reject_outliers (radix select on the device) == numpy on the downloaded error table:
  quantiles bit-for-bit (numpy 'linear' method), RMS to 1e-12 relative, identical inlier masks and residual order."""
  g, rig = load_golden(name)
  c = mirror(rig)
  x = g["ba_x_raw"]
  with Handle(c) as h:
    err, valid = h.reprojection_error(x)
    e = err[valid]
    qs = [0, 0.25, 0.5, 0.75, 1, 0.95, 0.123]
    mse, rms, q, n = h.error_stats(x, quantiles=qs)
    assert n == e.size
    assert np.array_equal(q, np.array([np.quantile(e, v) for v in qs]))
    assert mse == pytest.approx(np.square(e).mean(), rel=1e-12)
    thr = np.quantile(e, 0.75) * 5.0
    n_in, n_valid = h.reject_outliers(x, thr)
    mask = h.get_inliers()
    assert np.array_equal(mask, (err < thr) & valid)
    assert (n_in, n_valid) == (int(mask.sum()), int(valid.sum()))
    # inlier statistics and the residual ordering after a device-side rejection
    _, rms_i, q_i, n_i = h.error_stats(x, inliers_only=True)
    assert n_i == n_in and np.array_equal(q_i, np.array([np.quantile(err[mask], v) for v in [0, .25, .5, .75, 1]]))
    oc = oracle(rig).copy(inlier_mask=mask)
    assert np.abs(h.residuals(x) - oc.evaluate(x)).max() < 1e-9
    # the fused pass honours the new mask
    cost, _, _ = h.normal_equations(x)
    r = oc.evaluate(x)
    assert cost == pytest.approx(0.5 * r @ r, rel=1e-12)


def test_adjust_board_block():
  """optimize.boards=True (`adjust_board`, board/charuco.py:112-117): board-point columns of the Jacobian, their normal
  equation blocks (k_points), and a solve that reaches the reference's cost."""
  g, rig = load_golden("tiny_boards")
  c = mirror(rig)
  assert c.param_vec.size == g["x0"].size
  hm = HostMath(c)
  with Handle(c) as h:
    assert np.abs(h.residuals(g["x0"]) - g["r0"]).max() < 1e-9
    J = h.jacobian(g["x0"])
    assert rel_col_error(J, golden_jacobian(g)) < 5e-5
    assert np.abs((J - hm.jacobian(g["x0"]))).max() <= 1e-11 * abs(J).max()
    Jd = J.toarray()
    for mf in (1, 0):
      h.set_mfma(mf)
      cost, grad, diag = h.normal_equations(g["x0"])
      H = h.dense_hessian()
      assert np.abs(H - Jd.T @ Jd).max() <= 1e-12 * np.abs(H).max()
      assert np.abs(grad - Jd.T @ g["r0"]).max() <= 1e-12 * np.abs(grad).max()
      assert np.array_equal(H, H.T)
    res = h.solve(g["x0"])
    assert res.status in (2, 3, 4) and res.cost <= float(g["ba_cost"]) * (1 + 1e-9)
    # the reference's own solution evaluates identically
    oc = oracle(rig)
    assert np.abs(h.residuals(g["ba_x_raw"]) - oc.evaluate(g["ba_x_raw"])).max() < 1e-9
  out = c.bundle_adjust()
  assert out.boards[0].adjusted_points.shape == c.boards[0].adjusted_points.shape
  assert abs(calibration.error_stats(out.reprojection_error).rms - float(g["ba_rms"])) < 5e-2


def test_adjust_board_rolling_and_handeye_blocks():
  for name in ["tiny_rolling", "tiny_handeye", "tiny_fisheye"]:
    g, rig = load_golden(name)
    c = mirror(rig).enable(boards=True)
    x0 = c.param_vec
    with Handle(c) as h:
      J = h.jacobian(x0).toarray()
      r = h.residuals(x0)
      cost, grad, diag = h.normal_equations(x0)
      H = h.dense_hessian()
      assert np.abs(H - J.T @ J).max() <= 1e-12 * np.abs(H).max(), name
      assert np.abs(grad - J.T @ r).max() <= 1e-12 * np.abs(grad).max(), name
    oc = oracle(rig).enable(boards=True)
    assert np.abs(r - oc.evaluate(x0)).max() < 1e-9
    from scipy.optimize._numdiff import approx_derivative
    cols = np.arange(x0.size - 12, x0.size)          # spot-check the last board-point columns by finite differences
    for j in cols[::5]:
      e = np.zeros_like(x0); hstep = 1e-6; e[j] = hstep
      fd = (oc.evaluate(x0 + e) - oc.evaluate(x0 - e)) / (2 * hstep)
      assert np.abs(fd - J[:, j]).max() <= 1e-5 * max(np.abs(J[:, j]).max(), 1.0), (name, j)


@pytest.mark.parametrize("ns,blocked", [(5, 0), (16, 0), (18, 0), (31, 0), (32, 0), (40, 0), (40, 1), (140, 0),
                                        (159, 0), (160, 0), (190, 0), (286, 0), (700, 0), (1023, 1), (200, 0), (200, 1),
                                        (333, 1), (1500, 1),
                                        # 6: the multi-launch panel kernels k_cholp_* (automatic for 160 < ns + 1 <= 1024)
                                        (5, 6), (16, 6), (17, 6), (47, 6), (48, 6), (49, 6), (140, 6), (286, 6), (288, 6),
                                        (400, 6), (1023, 6), (1023, 0),
                                        (1, 0), (15, 0), (17, 0), (33, 0), (64, 0), (96, 0), (127, 0), (128, 0), (143, 0), (144, 0),
                                        (150, 0)])
def test_device_cholesky_paths(ns, blocked):
  """The three Cholesky paths of the reduced system vs numpy: LDS-resident tiles (0, ns + 1 <= 160), multi-launch panel
  kernels (6; automatic up to ns + 1 = 1024), multi-workgroup kernels (1; automatic beyond)."""
  rng = np.random.default_rng(ns)
  M = rng.normal(size=(ns + 20, ns))
  S = M.T @ M / ns + 0.1 * np.eye(ns)
  rhs = rng.normal(size=ns)
  with Handle(mirror(synthetic.make_rig("tiny"))) as h:
    p = h.debug_chol(S, rhs, reg=0.05, blocked=blocked)
  ref = np.linalg.solve(S + 0.05 * np.eye(ns), rhs)
  assert np.abs(p - ref).max() <= 1e-10 * np.abs(ref).max()


def test_adjust_board_large_reduced_system():
  """cfg1 with adjust_board: ns = 18 + 3 x 315 = 963 shared parameters -> multi-workgroup Cholesky inside the solve."""
  g, rig = load_golden("cfg1")
  c = mirror(rig).enable(boards=True)
  x0 = c.param_vec
  with Handle(c) as h:
    J = h.jacobian(x0)
    r = h.residuals(x0)
    cost, grad, diag = h.normal_equations(x0)
    assert np.abs(J.T @ r - grad).max() <= 1e-11 * np.abs(grad).max()
    assert np.abs(np.asarray(J.multiply(J).sum(axis=0)).ravel() - diag).max() <= 1e-11 * diag.max()
    reg = 1e-3
    gn, gh, si = h.debug_gn_step(reg)
    d = 1 / si
    Hs = (J.T @ J).toarray() * d[:, None] * d[None, :]
    ref = np.linalg.solve(Hs + reg * np.eye(x0.size), d * grad)
    assert np.abs(gn - ref).max() <= 1e-8 * np.abs(ref).max()
    res = h.solve(x0)
    assert res.status in (2, 3, 4) and res.cost < float(g["ba_cost"])      # more freedom than the fixed-board fit


def test_handle_cache_sees_a_changed_validity_mask_and_float32_tables():
  """the device-handle cache is keyed on the point table by identity AND content: a copy of the Calibration whose point
  table has another `valid` mask (same `points` object) must not hit the tables built for the old mask, and float32
  detection tables (widened into a copy on lowering) keep their identity alive inside the cache entry."""
  from multical_amd.structs import Table
  g, rig = load_golden("tiny")
  c = mirror(rig)
  calibration.handle_cache.clear()
  r_all = c.residuals()
  valid2 = c.point_table.valid.copy()
  valid2[0, 0] = False                                  # drop camera 0 / frame 0
  c2 = c.copy(point_table=Table.create(points=c.point_table.points, valid=valid2))
  r2 = c2.residuals()
  assert r2.size == 2 * int((c2.valid).sum()) and r2.size < r_all.size
  oc = oracle(rig)
  oc2 = oc.copy(valid=valid2)
  assert np.abs(r2 - oc2.evaluate(c2.param_vec)).max() < 1e-9
  assert np.abs(c.residuals() - r_all).max() == 0.0     # and back again
  # float32 detections: two different tables of the same shape in a loop never alias
  for seed in (31, 32, 33):
    rg = synthetic.make_rig("tiny", seed=seed)
    rg.points = rg.points.astype(np.float32)
    cm = mirror(rg)
    ocm = restate.from_rig(rg)
    assert np.abs(cm.residuals() - ocm.evaluate(cm.param_vec)).max() < 1e-9
  # a float32 table goes up as float32 (mcba_problem.points_f32) and is widened on the device: the same bits as the
  # widened copy uploaded as float64
  rg = synthetic.make_rig("tiny_rolling", seed=5)
  p32 = rg.points.astype(np.float32)
  rg.points = p32
  r32 = mirror(rg).residuals()
  rg.points = p32.astype(np.float64)
  r64 = mirror(rg).residuals()
  assert r32.size == r64.size and np.array_equal(r32, r64)


@pytest.mark.parametrize("switch", ["MCBA_FUSED=0", "MCBA_ASM_STAGE_KB=4", "MCBA_FUSED=0,MCBA_TMAT_GLOBAL=1",
                                    "MCBA_NCHUNK_TARGET=1024", "MCBA_SHARED_FINAL_BIG=1", "MCBA_LIN_COMPACT=0", "MCBA_SYRK3=1", "MCBA_SPLIT_Q00=1", "MCBA_SPEC_ACCEPT=0", "MCBA_SPEC_ACCEPT=0,MCBA_NO_PUBLISH=1"])
def test_alternative_linearisation_paths_match_the_default(switch):
  """Paths of the evaluation that the fixtures do not reach by themselves, each forced with its switch in a subprocess
  (mcba_debug_set_switch, once per process -- the product library reads no MCBA_* experiment switch from the environment); all must reproduce the normal equations of the default form to round-off,
  for every motion model, and the same solve:
    (default)                 table-fed fused form: pose entries from the pose table (k_prep / k_vec_step), chains and That
                              in k_linearize (no k_tmat, no That table)
    MCBA_FUSED=0              table form: k_tmat writes That and the chain matrices of every view, k_linearize reads them
    MCBA_SHARED_FINAL_BIG=1   the final sum of the shared part for rigs with more than 128 (camera, board) pairs
    MCBA_ASM_STAGE_KB=4       frame blocks of k_assemble stage their records in several groups (rigs with many views per frame)
    MCBA_TMAT_GLOBAL=1        k_tmat reads the global pose table (rigs whose cameras + boards exceed the local table)
    MCBA_NCHUNK_TARGET=1024   more chunk sums than the default split of the shared part
    MCBA_LIN_COMPACT=0        k_linearize over the masks + slot tables instead of the compacted observation tables"""
  import os, subprocess, sys, json
  code = r'''
import sys, json, os, numpy as np
sys.path.insert(0, "."); sys.path.insert(0, "tests")
from util import load_golden, mirror
from multical_amd.backend import Handle
from multical_amd import _lib
for kv in filter(None, os.environ.get("TEST_SWITCHES", "").split(",")):
  _lib.set_switch(*kv.split("="))
out = {}
for name in ["tiny", "tiny_rolling", "tiny_handeye", "tiny_fisheye", "tiny_edge", "tiny_pin4", "cfg1", "tiny_tilted"]:
  g, rig = load_golden(name)
  with Handle(mirror(rig)) as h:
    cost, grad, diag = h.normal_equations(g["x0"])
    H = h.dense_hessian()
    res = h.solve(g["x0"])
  out[name] = dict(cost=cost, grad=grad.tolist(), hsum=float(np.abs(H).sum()), H=H.ravel()[::7].tolist(), nfev=res.nfev,
                   final=res.cost)
from multical_amd import synthetic   # the hand-eye rig at full size (no per-frame block: chunk sums only, DF == 0 in k_shared_final)
c = mirror(synthetic.make_rig("cfg5_handeye"))
with Handle(c) as h:
  cost, grad, diag = h.normal_equations(c.param_vec)
  H = h.dense_hessian()
  res = h.solve(c.param_vec)
out["cfg5_handeye"] = dict(cost=cost, grad=grad.tolist(), hsum=float(np.abs(H).sum()), H=H.ravel()[::7].tolist(), nfev=res.nfev,
                           final=res.cost)
print("RESULT" + json.dumps(out))
'''
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  res = {}
  base = {k: v for k, v in os.environ.items() if not k.startswith("MCBA_") and k != "TEST_SWITCHES"}
  for fused, env in (("0", base), ("1", dict(base, TEST_SWITCHES=switch))):
    p = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    res[fused] = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT")][0][6:])
  for name, a in res["0"].items():
    b = res["1"][name]
    assert b["cost"] == pytest.approx(a["cost"], rel=1e-13), name
    ga, gb = np.array(a["grad"]), np.array(b["grad"])
    assert np.abs(ga - gb).max() <= 1e-11 * np.abs(ga).max(), name
    Ha, Hb = np.array(a["H"]), np.array(b["H"])
    assert np.abs(Ha - Hb).max() <= 1e-11 * np.abs(Ha).max(), name
    assert b["nfev"] == a["nfev"] and b["final"] == pytest.approx(a["final"], rel=1e-9), name


def test_linearize_observation_sources_agree():
  """k_linearize reads its observations from the compacted tables of the inlier set (LsmrCompact: form 3, the default) or from the masks +
  slot tables (form 2, MCBA_LIN_COMPACT=0).  Every observation sits in the same lane of the same 64-row chunk in both, so cost, gradient
  and H come out BIT-IDENTICAL -- on every motion / camera model, with empty views and after the inlier set changed (the compacted
  tables are rebuilt); a board with more than 512 points is walked in segments by form 2 only (chunk boundaries differ): round-off."""
  import os, subprocess, sys, json
  code = r"""
import sys, json, os, numpy as np
sys.path.insert(0, "."); sys.path.insert(0, "tests")
from util import load_golden, mirror
from multical_amd.backend import Handle
from multical_amd import _lib, synthetic, calibration
if os.environ.get("TEST_MASKS") == "1":
  _lib.set_switch("MCBA_LIN_COMPACT", "0")
out = {}
def record(key, h, x):
  cost, grad, diag = h.normal_equations(x)
  H = h.dense_hessian()
  out[key] = dict(cost=cost, grad=grad.tolist(), diag=diag.tolist(), H=H.ravel()[::5].tolist())
for name in ["tiny", "tiny_rolling", "tiny_handeye", "tiny_fisheye", "tiny_edge", "tiny_pin4", "cfg1", "tiny_tilted", "tiny_fixintr",
             "tiny_fishmix", "tiny_softl1", "tiny_bigboard"]:
  g, rig = load_golden(name)
  with Handle(mirror(rig)) as h:
    record(name, h, g["x0"])
    if name in ("tiny_rolling", "cfg1"):
      h.reject_outliers(g["x0"], 1.0)          # another inlier set: the compacted tables follow
      record(name + "/rejected", h, g["x0"])
c = calibration.from_rig(synthetic.make_rig("cfg3", frames=40))
with Handle(c) as h:
  record("cfg3_40", h, c.param_vec)
print("RESULT" + json.dumps(out))
"""
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  base = {k: v for k, v in os.environ.items() if not k.startswith("MCBA_")}
  res = {}
  for masks in ("0", "1"):
    p = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(base, TEST_MASKS=masks), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    res[masks] = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT")][0][6:])
  for key, a in res["0"].items():
    b = res["1"][key]
    if key == "tiny_bigboard":
      for q in ("grad", "diag", "H"):
        va, vb = np.array(a[q]), np.array(b[q])
        assert np.abs(va - vb).max() <= 1e-12 * np.abs(va).max(), (key, q)
      assert b["cost"] == pytest.approx(a["cost"], rel=1e-13)
    else:
      assert a == b, key


@pytest.mark.parametrize("name", ["tiny_rolling", "tiny", "tiny_handeye", "tiny_fisheye"])
def test_projected_matches_the_oracle(name):
  """mcba_project_model == Calibration.projected of the reference (oracle pinned to it in test_oracle_vs_reference):
  rolling shutter iterates the scan time from the projected row (t = 0.5, then 4 passes)."""
  g, rig = load_golden(name)
  c = mirror(rig)
  want, valid = oracle(rig).projected()
  seen = valid & rig.valid
  with Handle(c) as h:
    got = h.project_model(g["x0"])
    assert np.abs(got - want)[seen].max() < 1e-9
    # slots that no camera detected lie far outside the image, where the distortion polynomial is steep and the rolling-
    # shutter fixed point amplifies round-off (1e-13 -> 4e-6 px after four passes): relative tolerance there
    assert (np.abs(got - want)[valid] / (1.0 + np.abs(want[valid]))).max() < 1e-6
    if name == "tiny_rolling":     # differs from `reprojected` (scan time from the OBSERVED row) where both are defined
      assert np.abs(got - h.project(g["x0"]))[valid & rig.valid].max() > 1e-6
      assert np.abs(h.project_model(g["x0"], max_iterations=0) - oracle(rig).projected(max_iterations=0)[0])[valid].max() < 1e-9
  tab = c.projected
  assert np.array_equal(tab.valid, valid) and np.abs(tab.points - want)[seen].max() < 1e-9


@pytest.mark.parametrize("name", ["tiny_rolling", "tiny_edge", "tiny_handeye"])
def test_reprojection_tables_consumer(name):
  """the GUI's reprojection tables (interface/view_table.py:43-52) built from the back-end's `projected`
  (mcba_project_model) and the inlier mask after an outlier round: per overall / view / board-view / board / camera /
  frame the detected and outlier counts are identical, mse / rms / quantiles within 1e-9 px of the oracle's tables."""
  import warnings
  from multical_amd import view_table
  g, rig = load_golden(name)
  c = mirror(rig)
  c = c.reject_outliers_quantile(0.75, 5.0) if hasattr(c, "reject_outliers_quantile") else c
  oc = oracle(rig).copy(inlier_mask=c.inliers)
  for inlier_only in (False, True):
    with warnings.catch_warnings():
      warnings.simplefilter("ignore")                      # (all-NaN slices of views without detections)
      got = view_table.reprojection_tables(c, inlier_only=inlier_only)
    want = restate.reprojection_tables(oc, inlier_only=inlier_only)
    for axis_name, w in want.items():
      t = got[axis_name]
      assert np.array_equal(t.detected, w["detected"]) and np.array_equal(t.outliers, w["outliers"]), axis_name
      for k in ("mse", "rms", "min", "lower_q", "median", "upper_q", "max"):
        a, b = np.asarray(t[k], dtype=np.float64), np.asarray(w[k], dtype=np.float64)
        assert np.array_equal(np.isnan(a), np.isnan(b)), (axis_name, k)
        assert np.nanmax(np.abs(a - b), initial=0.0) < 1e-9 * max(1.0, np.nanmax(np.abs(b), initial=0.0)), (axis_name, k)


@pytest.mark.parametrize("name,frames,seed", [("tiny_rolling", None, 5), ("tiny_fisheye", None, 6), ("cfg4", 12, 5),
                                              ("cfg2", 60, 7), ("cfg3", 40, 8), ("cfg5", 40, 9)])
def test_initialise_poses_on_the_device_matches_the_oracle(name, frames, seed):
  """multical_amd.tables.initialise_poses (every matrix.align_transforms_robust of the reference's pose-graph
  initialisation as a device batch: relative poses, Ward-cluster robust mean, quartile outlier test) against the oracle
  restatement, which is pinned bit-identical to the unmodified reference (test_oracle_vs_reference).  cfg5: the pose table
  after the reference's outlier pose rejection (pose_error_limit, tables.py:44-56) -- about half of its views are invalid."""
  from multical_amd import tables as mtables
  from multical_amd.structs import Table
  from oracle import restate_init
  rig = synthetic.make_rig(name, frames=frames)
  pt = synthetic.make_pose_table(rig, seed=seed)
  want = restate_init.initialise_poses(restate_init.table(pt["poses"], pt["valid"]), pt["num_points"])
  got = mtables.initialise_poses(Table.create(poses=pt["poses"], valid=pt["valid"], num_points=pt["num_points"]))
  for k in ("camera", "board", "times"):
    assert np.array_equal(got[k].valid, want[k]["valid"]), k
    assert np.abs(got[k].poses - want[k]["poses"]).max() < 1e-9, (k, np.abs(got[k].poses - want[k]["poses"]).max())


def test_align_transforms_robust_batch_edge_cases():
  """single pair, two pairs (fewer points than clusters), an empty problem, masked entries, inlier masks."""
  from multical_amd import tables as mtables
  from oracle import restate_init
  rng = np.random.default_rng(3)
  def poses(n, sigma):
    return synthetic.to_matrix(np.concatenate([rng.normal(0, sigma, (n, 3)), rng.normal(0, 1.0, (n, 3))], axis=1))
  T = synthetic.to_matrix(np.array([0.3, -0.2, 0.5, 0.1, 0.2, -0.4]))
  problems = []
  for n in (1, 2, 3, 9, 10, 11, 29, 30, 31, 200, 2600):     # (2600: ranking -> radix select, clustering state in memory + LDS tiles)
    a = poses(n, 0.5)
    b = synthetic.perturb(T @ a, rng, 1e-3, 1e-3)
    if n > 8:
      b[::7] = poses(len(b[::7]), 1.0)         # gross outliers
    mask = rng.random(n) < 0.85 if n > 3 else None
    if mask is not None and not mask.any():
      mask[0] = True
    problems.append((a, b, mask))
  out, valid, inl = mtables.align_transforms_robust_batch(problems + [(np.zeros((0, 4, 4)), np.zeros((0, 4, 4)), None)])
  assert valid[:-1].all() and not valid[-1] and np.array_equal(out[-1], np.eye(4))
  for (a, b, m), o, il in zip(problems, out, inl):
    want, want_inl = restate_init.align_transforms_robust(a, b, valid=m)
    assert np.array_equal(il, want_inl)
    assert np.abs(o - want).max() < 1e-9


def test_align_poses_indexed_equals_the_gathered_batch():
  """mcba_align_poses_indexed (pairs as indices into one pose table) against mcba_align_poses_robust on the gathered copies:
  the same bits, with and without mask / inversion, for problems of different sizes (one of them empty)."""
  from multical_amd import tables as mtables
  rng = np.random.default_rng(17)
  table = synthetic.to_matrix(np.concatenate([rng.normal(0, 0.4, (300, 3)), rng.normal(0, 1.0, (300, 3))], axis=1))
  sizes = np.array([40, 0, 7, 120, 1, 33])
  total = int(sizes.sum())
  ia, ib = rng.integers(0, 300, total), rng.integers(0, 300, total)
  for mask in (None, rng.random(total) < 0.8):
    for invert in (False, True):
      o1, v1, i1 = mtables.align_transforms_robust_indexed(table, ia, ib, sizes, mask, invert=invert)
      o2, v2, i2 = mtables.align_transforms_robust_ragged(table[ia], table[ib], sizes, mask, invert=invert)
      assert np.array_equal(v1, v2) and np.array_equal(i1, i2) and np.array_equal(o1, o2)
      assert not v1[1] and v1[0]
  with pytest.raises(Exception, match="out of range"):
    mtables.align_transforms_robust_indexed(table, np.full(total, 300), ib, sizes)


def test_staged_alignment_batch_with_degenerate_members():
  """A batch whose largest problem sends it through the staged kernels (k_align_stage_*: more than 2 048 entries) together with
  an empty problem, a single pair, a fully masked one and small ones: every member against the oracle."""
  from multical_amd import tables as mtables
  from oracle import restate_init
  rng = np.random.default_rng(23)
  def poses(n, sigma):
    return synthetic.to_matrix(np.concatenate([rng.normal(0, sigma, (n, 3)), rng.normal(0, 1.0, (n, 3))], axis=1))
  T = synthetic.to_matrix(np.array([-0.2, 0.1, 0.4, 0.3, -0.1, 0.2]))
  problems = []
  for n, masked in ((2500, False), (0, False), (1, False), (7, False), (40, True), (300, False)):
    a = poses(n, 0.5)
    b = synthetic.perturb(T @ a, rng, 1e-3, 1e-3) if n else a
    if n > 8:
      b[::9] = poses(len(b[::9]), 1.0)
    mask = (np.zeros(n, dtype=bool) if masked else rng.random(n) < 0.9) if n > 1 else None
    problems.append((a, b, mask))
  for invert in (False, True):
    out, valid, inl = mtables.align_transforms_robust_batch(problems, invert=invert)
    for k, ((a, b, m), o, il) in enumerate(zip(problems, out, inl)):
      if len(a) == 0 or (m is not None and not m.any()):
        assert not valid[k] and np.array_equal(o, np.eye(4)) and not il.any()
        continue
      aa, bb = (np.linalg.inv(a), np.linalg.inv(b)) if invert else (a, b)
      want, want_inl = restate_init.align_transforms_robust(aa, bb, valid=m)
      if invert:
        want = np.linalg.inv(want)
      assert valid[k] and np.array_equal(il, want_inl), k
      assert np.abs(o - want).max() < 1e-9, (k, invert)


def test_align_transforms_robust_with_duplicated_poses():
  """Exact duplicates among the relative poses (repeated or noise-free detections) give zero-height merges that TIE at
  the dendrogram cut: scipy's fcluster(maxclust) applies every merge up to the threshold height, so fewer than t flat
  clusters come out and the 'most common' cluster differs from a cut after exactly n - t merges."""
  from multical_amd import tables as mtables
  from oracle import restate_init
  rng = np.random.default_rng(11)
  def poses(n, sigma):
    return synthetic.to_matrix(np.concatenate([rng.normal(0, sigma, (n, 3)), rng.normal(0, 1.0, (n, 3))], axis=1))
  T = synthetic.to_matrix(np.array([0.3, -0.2, 0.5, 0.1, 0.2, -0.4]))
  problems = []
  # (the last case is large enough for the staged kernels: nearest-neighbour caching and split scans with exact ties)
  for groups, reps, extra in ((4, 2, 0), (6, 3, 2), (3, 8, 5), (10, 4, 0), (1, 12, 3), (280, 8, 100)):
    a0 = poses(groups, 0.5)
    b0 = synthetic.perturb(T @ a0, rng, 2e-3, 2e-3)
    a = np.concatenate([np.repeat(a0, reps, axis=0), poses(extra, 0.5)])
    b = np.concatenate([np.repeat(b0, reps, axis=0), T @ a[groups * reps:]]) if extra else np.repeat(b0, reps, axis=0)
    if extra:
      b[groups * reps:] = synthetic.perturb(b[groups * reps:], rng, 2e-3, 2e-3)
    perm = rng.permutation(len(a))
    problems.append((a[perm], b[perm], None))
  out, valid, inl = mtables.align_transforms_robust_batch(problems)
  assert valid.all()
  for (a, b, m), o, il in zip(problems, out, inl):
    want, want_inl = restate_init.align_transforms_robust(a, b, valid=m)
    assert np.array_equal(il, want_inl)
    assert np.abs(o - want).max() < 1e-9


def test_resource_cache_reuses_buffers_of_closed_handles():
  """mcba_destroy parks buffers / stream, the next mcba_create of the same shape takes them back: identical results from
  recycled (dirty) memory, also after a handle of ANOTHER shape ran in between, and after the cache was emptied."""
  from multical_amd.backend import release_cached_memory
  g, rig = load_golden("tiny_rolling")
  g2, rig2 = load_golden("tiny")
  ref = None
  for k in range(4):
    with Handle(mirror(rig)) as h:
      cost, grad, diag = h.normal_equations(g["x0"])
      H = h.dense_hessian()
      res = h.solve(g["x0"])
      r = h.residuals(g["x0"])
    cur = (cost, grad.copy(), H.copy(), res.cost, res.nfev, r.copy())
    if ref is None:
      ref = cur
    else:
      assert cur[0] == ref[0] and np.array_equal(cur[1], ref[1]) and np.array_equal(cur[2], ref[2])
      assert cur[3] == ref[3] and cur[4] == ref[4] and np.array_equal(cur[5], ref[5])
    if k == 1:
      with Handle(mirror(rig2)) as h2:
        assert np.abs(h2.residuals(g2["x0"]) - g2["r0"]).max() < 1e-9
    if k == 2:
      release_cached_memory()


@pytest.mark.parametrize("name", ["tiny_rolling", "cfg1", "tiny_fishmix"])
def test_adjust_outliers_in_one_call_equals_the_step_by_step_loop(name, monkeypatch):
  """Calibration.adjust_outliers as ONE library call (mcba_adjust_outliers: the default) against the reference-shaped Python
  loop over report / reject_outliers / bundle_adjust on fresh Calibration objects (MULTICAL_AMD_FUSED_LOOP=0): same inlier
  masks, same log lines up to the printed digits, same result (the step-by-step loop canonicalises the rotation vectors between
  the rounds -- a change of 1e-16 in x -- the single call does not)."""
  import logging
  from multical_amd import Workspace
  g, rig = load_golden(name)

  def run():
    lines = []

    class Grab(logging.Handler):
      def emit(self, rec):
        lines.append(rec.getMessage())

    log = logging.getLogger("calibration")
    hd = Grab()
    log.addHandler(hd)
    log.setLevel(logging.INFO)
    try:
      out = Workspace(mirror(rig)).calibrate(cameras=rig.optimize["cameras"], camera_poses=rig.optimize["camera_poses"],
                                             auto_scale=2.0 if name == "tiny_rolling" else None,
                                             loss="soft_l1" if name == "tiny_rolling" else "linear")
    finally:
      log.removeHandler(hd)
    return out, lines

  fast, lf = run()
  monkeypatch.setenv("MULTICAL_AMD_FUSED_LOOP", "0")
  slow, ls = run()
  assert np.array_equal(fast.inliers, slow.inliers)
  assert fast.error_statistics(True).rms == pytest.approx(slow.error_statistics(True).rms, abs=1e-9)
  assert fast.error_statistics(False).rms == pytest.approx(slow.error_statistics(False).rms, abs=1e-9)
  assert np.abs(fast.param_vec - slow.param_vec).max() < 1e-6      # (the round-off of the canonicalisation, amplified by three solves)
  import re
  keep = lambda ls_: [l for l in ls_ if l.startswith(("Adjust_outliers", "Rejecting", "Auto scaling", "Beginning"))]
  number = re.compile(r"[-+]?\d+\.?\d*(?:[eE][-+]?\d+)?")
  assert len(keep(lf)) == len(keep(ls))
  for a, b in zip(keep(lf), keep(ls)):     # same text; numbers to the printed precision minus the last digit
    assert number.sub("#", a) == number.sub("#", b), (a, b)
    for u, v in zip(number.findall(a), number.findall(b)):
      assert float(u) == pytest.approx(float(v), rel=1e-6, abs=1e-9), (a, b)
  rows = lambda ls_: [l.split()[:3] for l in ls_ if l.strip() and l.split()[0].isdigit()]
  assert rows(lf) == rows(ls)          # iteration, nfev, cost of every solve
