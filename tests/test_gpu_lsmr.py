"""GPU (MI355X): the lsmr mode (mcba_options.tr_solver = MCBA_TR_LSMR) below and above the solver level.

  * kernel level: the matrix-free products J v / J^T u of k_lsmr_jv / k_lsmr_jtu / k_lsmr_gather against the analytic Jacobian
    mcba_jacobian returns (itself pinned to the reference's finite differences and to 3-point differences of the oracle:
    tests/test_gpu_parity.py, tests/test_gpu_protocol.py), on every motion / camera model and with boards=True;
  * END POINTS of the unmodified reference at the BASELINE configurations' STATED sizes (tests/golden/cfg*_endpoint.npz,
    oracle/make_endpoint.py: hours of one host core each): solver = "lsmr" reproduces them with identical nfev / status.
"""
import os

import numpy as np
import pytest

from multical_amd import synthetic, calibration
from multical_amd.backend import Handle
from util import load_golden, mirror, GOLDEN

pytestmark = pytest.mark.gpu

PRODUCT_CASES = ["tiny", "tiny_rolling", "tiny_fisheye", "tiny_handeye", "tiny_rational", "tiny_thin_prism", "tiny_tilted",
                 "tiny_edge", "tiny_fixintr", "tiny_pin4", "tiny_boards", "tiny_bigboard", "tiny_fishmix", "tiny_fishmix5", "cfg1"]


@pytest.mark.parametrize("name", PRODUCT_CASES)
def test_lsmr_products_against_the_jacobian(name):
  """J v and J^T u of the lsmr mode's kernels = h.jacobian(x) @ v and .T @ u to rounding (1e-12 of sum |J_ij| |v_j|): the row
  pairs, the That chain of the pose blocks, the per-view reduction, the gather over the views of every parameter (incl. the
  board-point block of boards=True and invalid / ragged blocks, whose columns must come back exactly zero)."""
  g, rig = load_golden(name)
  c = mirror(rig)
  rng = np.random.default_rng(5)
  for x in (c.param_vec, c.param_vec + 1e-3 * rng.normal(size=c.param_vec.size)):
    with Handle(c) as h:
      J = h.jacobian(x)
      v = rng.normal(size=h.n_params)
      u = rng.normal(size=h.n_residuals)
      jv, jtu = h.lsmr_products(x, v, u)
      jv_only, _ = h.lsmr_products(x, v, None)
      _, jtu_only = h.lsmr_products(x, None, u)
    A = abs(J)
    assert np.abs(jv - J @ v).max() <= 1e-12 * (A @ np.abs(v)).max()
    scale = A.T @ np.abs(u)
    assert np.abs(jtu - J.T @ u).max() <= 1e-12 * scale.max()
    assert np.all(jtu[scale == 0] == 0)                   # structurally zero columns (skew, invalid poses, fix_aspect)
    assert np.array_equal(jv, jv_only) and np.array_equal(jtu, jtu_only)


@pytest.mark.parametrize("name", PRODUCT_CASES)
def test_lsmr_two_launch_kernels_against_the_jacobian(name):
  """The kernels the DEFAULT solver iterates with -- k_lsmr_fused2 (both products of a Golub-Kahan step from one evaluation of the
  analytic rows) and k_lsmr_gather3 -- against the analytic Jacobian: J v to 1e-12, J^T (J v) to 1e-11 (of sum |J^T| |J v|)."""
  g, rig = load_golden(name)
  c = mirror(rig)
  rng = np.random.default_rng(8)
  x = c.param_vec + 1e-3 * rng.normal(size=c.param_vec.size)
  with Handle(c) as h:
    J = h.jacobian(x)
    v = rng.normal(size=h.n_params)
    h.set_lsmr_fused(2)          # the evaluating form (the default on rolling-shutter rigs and with boards=True)
    jv, w = h.lsmr_fused_products(x, v)
    jv2, w2 = h.lsmr_fused_products(x, v)
    h.set_lsmr_masks_form(True)  # ... reading the frame-major tables instead of the compacted ones
    jvm, wm = h.lsmr_fused_products(x, v)
    h.set_lsmr_masks_form(False)
    if name != "tiny_bigboard":
      assert np.array_equal(jv, jvm) and np.array_equal(w, wm), (np.abs(jv - jvm).max(), np.abs(w - wm).max())
    h.set_lsmr_fused(3)          # the same step with the per-observation state streamed back from the cache (CACHED = 2)
    jv3, w3 = h.lsmr_fused_products(x, v)
  assert np.array_equal(jv, jv3) and np.array_equal(w, w3), (np.abs(jv - jv3).max(), np.abs(w - w3).max())
  A = abs(J)
  ref = J @ v
  assert np.abs(jv - ref).max() <= 1e-12 * (A @ np.abs(v)).max()
  scale = A.T @ np.abs(ref)
  assert np.abs(w - J.T @ ref).max() <= 1e-11 * scale.max()
  assert np.all(w[scale == 0] == 0)
  assert np.array_equal(jv, jv2) and np.array_equal(w, w2)          # deterministic


def test_lsmr_products_after_an_outlier_rejection():
  """the products follow the CURRENT inlier set (view lists, residual order, obs_index of the board-point gather)"""
  g, rig = load_golden("tiny_boards")
  c = mirror(rig)
  x = c.param_vec
  rng = np.random.default_rng(6)
  with Handle(c) as h:
    e, valid = h.reprojection_error(x)
    h.reject_outliers(x, float(np.quantile(e[valid.astype(bool)], 0.9)))
    J = h.jacobian(x)
    assert J.shape[0] == h.n_residuals < g["r0"].size
    v, u = rng.normal(size=h.n_params), rng.normal(size=h.n_residuals)
    jv, jtu = h.lsmr_products(x, v, u)
  A = abs(J)
  assert np.abs(jv - J @ v).max() <= 1e-12 * (A @ np.abs(v)).max()
  assert np.abs(jtu - J.T @ u).max() <= 1e-12 * (A.T @ np.abs(u)).max()


def test_lsmr_mode_with_adjusted_board_points():
  """boards=True (board/charuco.py:112-117, sparsity calibration.py:188-190) under the lsmr mode: the reference's end point of
  `tiny_boards` within the reference's own spread, like every other fixture of test_device_lsmr_mode_*."""
  g, rig = load_golden("tiny_boards")
  with Handle(mirror(rig)) as h:
    res = h.solve(g["x0"], tr_solver="lsmr")
    e, v = h.reprojection_error(res.x)
    assert h.lsmr_iterations() > 0
  rms = float(np.sqrt(np.mean(e[v.astype(bool)] ** 2)))
  ref, spread = float(g["ba_rms"]), float(np.abs(g["ba_pert_rms"] - g["ba_rms"]).max())
  assert abs(rms - ref) <= max(1e-6, 3 * spread), (rms - ref, spread, res.nfev, int(g["ba_nfev"]))
  assert res.nfev <= 2 * int(g["ba_nfev"]) + 5


def load_endpoint(cfg):
  path = os.path.join(GOLDEN, f"{cfg}_endpoint.npz")
  if not os.path.exists(path):
    pytest.skip(f"{path} not generated (oracle/make_endpoint.py)")
  g = dict(np.load(path, allow_pickle=False))
  rig = synthetic.make_rig(str(g["config"]))
  assert tuple(g["shape"]) == rig.valid.shape and int(g["valid_count"]) == int(rig.valid.sum())
  assert float(g["points_sum"]) == pytest.approx(float(rig.points.sum()), rel=1e-13)
  return g, rig


def endpoint_spread(g):
  return float(np.abs(g["ba_pert_rms"] - g["ba_rms"]).max()) if "ba_pert_rms" in g else 0.0


@pytest.mark.parametrize("cfg", ["cfg3", "cfg5", "cfg4", "cfg5_handeye"])
def test_lsmr_mode_reproduces_the_reference_end_point_at_full_size(cfg, record_property):
  """BASELINE configs[2] (8 x 500 x 2 rolling shutter: the rig bench.py measures), configs[4] (6 x 400 x 5 fisheye) and configs[3]
  (16 x 1000 x 5) AT THEIR STATED SIZE: the unmodified reference's `Calibration.bundle_adjust()` end point (final RMS, nfev,
  status, cost) is reproduced by solver = "lsmr" within max(1e-6 px, the reference's own spread under 1e-12 px perturbations);
  the exact-step default solver's distance from that end point is reported beside it."""
  g, rig = load_endpoint(cfg)
  c = mirror(rig)
  assert np.array_equal(c.param_vec, g["x0"])
  out, res = c.bundle_adjust(solver="lsmr", return_result=True)
  rms = calibration.error_stats(out.reprojection_error).rms
  spread = endpoint_spread(g)
  native, nres = c.bundle_adjust(solver="native", return_result=True)
  rms_native = calibration.error_stats(native.reprojection_error).rms
  record_property("lsmr_minus_reference_px", rms - float(g["ba_rms"]))
  record_property("native_minus_reference_px", rms_native - float(g["ba_rms"]))
  record_property("reference_spread_px", spread)
  print(f"{cfg}: reference {float(g['ba_rms']):.9f} px (nfev {int(g['ba_nfev'])}, {float(g['ba_seconds']):.0f} s on one core), "
        f"lsmr {rms - float(g['ba_rms']):+.2e} px in {res.solve_seconds * 1e3:.1f} ms, native {rms_native - float(g['ba_rms']):+.2e} px "
        f"in {nres.solve_seconds * 1e3:.2f} ms, reference spread {spread:.1e}")
  assert abs(rms - float(g["ba_rms"])) <= max(1e-6, spread), (cfg, rms - float(g["ba_rms"]), spread)
  assert res.nfev == int(g["ba_nfev"]) and res.status == int(g["ba_status"])
  cost_spread = float(np.abs(g["ba_pert_cost"] - g["ba_cost"]).max()) if "ba_pert_cost" in g else 0.0
  assert abs(res.cost - float(g["ba_cost"])) <= max(2e-6 * float(g["ba_cost"]), cost_spread), (res.cost, float(g["ba_cost"]), cost_spread)
  # the exact solver ends at or below the reference's cost (converged optimum of the same function), never above its end point
  assert rms_native <= float(g["ba_rms"]) + max(1e-6, spread)


@pytest.mark.parametrize("cfg", ["cfg3", "cfg5", "cfg4", "cfg5_handeye"])
def test_workspace_calibrate_at_full_size_against_the_reference(cfg):
  """Workspace.calibrate's outlier loop (workspace.py:228-247 -> calibration.py:254-268) at the stated size under solver="lsmr":
  the reference's inlier mask after three rounds, bit for bit, and its inlier RMS."""
  from multical_amd import Workspace
  g, rig = load_endpoint(cfg)
  if "ao_inliers_packed" not in g:
    pytest.skip("adjust_outliers end point of the reference not generated")
  prev = calibration.set_solver("lsmr")
  try:
    ao = Workspace(mirror(rig)).calibrate(cameras=rig.optimize["cameras"], camera_poses=rig.optimize["camera_poses"])
  finally:
    calibration.set_solver(prev)
  ref_mask = np.unpackbits(g["ao_inliers_packed"])[:rig.valid.size].reshape(rig.valid.shape).astype(bool)
  diff = int(np.sum(ao.inliers != ref_mask))
  drms = ao.error_statistics(True).rms - float(g["ao_rms_inliers"])
  print(f"{cfg}: inlier mask after three rounds differs from the reference's in {diff} of {int(ref_mask.sum())} observations, "
        f"inlier RMS {drms:+.2e} px from the reference's")
  assert diff == 0, diff        # index-level work: the reference's mask bit for bit (measured: 0 at all three sizes)
  assert abs(drms) <= max(1e-6, endpoint_spread(g))


@pytest.mark.parametrize("name", ["cfg1", "tiny_handeye", "tiny_rolling", "tiny_fisheye", "tiny_boards", "tiny_edge", "tiny_fishmix"])
def test_lsmr_iteration_forms_agree(name):
  """The LSMR iteration exists in three forms -- two launches (default: k_lsmr_fused2 / k_lsmr_gather3), three (k_lsmr_fused) and the
  six launches of round 4 (one kernel per product + two scalar kernels): the same recurrences with different summation orders.
  They must take the same trust-region trajectory wherever the reference's end point is defined to 1e-6 px, and stay inside the
  reference's own spread elsewhere."""
  g, rig = load_golden(name)
  spread = float(np.abs(g["ba_pert_rms"] - g["ba_rms"]).max())
  out = {}
  with Handle(mirror(rig)) as h:
    for mode in (0, 1, 2, 3):
      h.set_lsmr_fused(mode)
      res = h.solve(g["x0"], tr_solver="lsmr")
      e, v = h.reprojection_error(res.x)
      out[mode] = (res.nfev, res.status, float(np.sqrt(np.mean(e[v] ** 2))), h.lsmr_iterations())
    xs = {}
    for mode in (2, 3):
      h.set_lsmr_fused(mode)
      xs[mode] = h.solve(g["x0"], tr_solver="lsmr").x
  assert np.array_equal(xs[2], xs[3]), np.abs(xs[2] - xs[3]).max()      # the cached-state form is the SAME arithmetic: same bits
  ref = float(g["ba_rms"])
  for mode in (0, 1, 2, 3):
    assert abs(out[mode][2] - ref) <= max(1e-6, 3 * spread), (name, mode, out)
  if spread < 3e-7:
    assert out[0][:2] == out[1][:2] == out[2][:2] == (int(g["ba_nfev"]), int(g["ba_status"])), (name, out)
    assert max(abs(out[m][2] - out[0][2]) for m in (1, 2)) <= 1e-6, (name, out)


@pytest.mark.parametrize("name", ["cfg1", "tiny_rolling", "tiny_fisheye", "tiny_handeye", "tiny_edge", "tiny_fishmix", "tiny_bigboard", "tiny_softl1"])
def test_lsmr_observation_sources_agree(name):
  """k_lsmr_fused2 reads its observations from the COMPACTED tables (residual order, built once per inlier set: one round trip per view) --
  or, with boards=True, from the frame-major tables with the mask bytes compacted per view in LDS (the only form until round 6,
  mcba_debug_set_lsmr_masks_form).  Same arithmetic, same lane for every observation: the two solves return the SAME bits (a board of
  more than 512 points is walked in segments by the masks form and deals its observations to other lanes: rounding-level differences
  there), also after an outlier rejection has changed the inlier set."""
  import json
  g, rig = load_golden(name)
  kw = json.loads(str(g["ba_kwargs_json"])) if "ba_kwargs_json" in g else {}
  opts = dict(tr_solver="lsmr", loss=kw.get("loss", "linear"), f_scale=kw.get("f_scale", 1.0))
  with Handle(mirror(rig)) as h:
    out = {}
    for masks in (False, True, False):
      h.set_lsmr_masks_form(masks)
      res = h.solve(g["x0"], **opts)
      out.setdefault(masks, []).append((res.x, res.nfev, res.status, res.cost, h.lsmr_iterations()))
    e, valid = h.reprojection_error(out[False][0][0])
    h.reject_outliers(out[False][0][0], float(np.quantile(e[valid.astype(bool)], 0.9)))
    after = {}
    for masks in (True, False):
      h.set_lsmr_masks_form(masks)
      after[masks] = h.solve(g["x0"], **opts)
  a, a2, b = out[False][0], out[False][1], out[True][0]
  assert np.array_equal(a[0], a2[0]) and a[1:] == a2[1:]
  if name == "tiny_bigboard":
    spread = float(np.abs(g["ba_pert_rms"] - g["ba_rms"]).max())
    assert abs(a[3] - b[3]) <= max(1e-9, 10 * spread) * a[3]
  else:
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], (float(np.abs(a[0] - b[0]).max()), a[1:], b[1:])
    assert np.array_equal(after[True].x, after[False].x) and after[True].nfev == after[False].nfev


@pytest.mark.parametrize("name", ["tiny_rolling", "tiny_boards", "cfg1"])
def test_lsmr_solve_is_bit_repeatable(name):
  """No atomics and no order-dependent reductions anywhere in the lsmr route: every workgroup folds partial sums in a fixed order
  and the scalar recurrences are bit-identical in all of them, so two solves of the same problem return the SAME bits -- also
  across handles -- although thousands of LSMR iterations amplify any rounding difference to the 1e-6 px level."""
  g, rig = load_golden(name)
  c = mirror(rig)
  xs, its = [], []
  for _ in range(2):
    with Handle(c) as h:
      for _ in range(2):
        res = h.solve(g["x0"], tr_solver="lsmr")
        xs.append(res.x)
        its.append((res.nfev, res.status, h.lsmr_iterations(), res.cost))
  assert all(np.array_equal(xs[0], x) for x in xs[1:]), [float(np.abs(xs[0] - x).max()) for x in xs[1:]]
  assert all(it == its[0] for it in its), its


@pytest.mark.parametrize("name", ["tiny_autoscale", "tiny_autoscale_huber", "tiny", "tiny_rolling", "tiny_handeye", "tiny_edge"])
def test_workspace_calibrate_under_the_default_solver(name):
  """Workspace.calibrate (workspace.py:228-247: enable -> 3 x {report, auto-scale, reject, bundle_adjust} -> report) under the DEFAULT
  solver -- robust losses with `auto_scale` included -- against the reference's own run of the same loop: the inlier mask after three
  rounds (up to the mask differences the reference's own perturbed re-runs show) and the inlier RMS within the reference's spread."""
  import json
  from multical_amd import Workspace
  g, rig = load_golden(name)
  kw = json.loads(str(g["ao_kwargs_json"])) if "ao_kwargs_json" in g else {}
  assert calibration.get_solver() == "lsmr"
  out = Workspace(mirror(rig)).calibrate(cameras=rig.optimize["cameras"], camera_poses=rig.optimize["camera_poses"],
                                         loss=kw.get("loss", "linear"), auto_scale=kw.get("auto_scale", None))
  allowed = int(g["ao_pert_mask_diff"].max()) if "ao_pert_mask_diff" in g else 0
  assert int((out.inliers != g["ao_inliers"]).sum()) <= allowed, (int((out.inliers != g["ao_inliers"]).sum()), allowed)
  spread = float(np.abs(g["ao_pert_rms_inliers"] - g["ao_rms_inliers"]).max())
  rms_inl = out.error_statistics(True).rms
  assert abs(rms_inl - float(g["ao_rms_inliers"])) <= max(1e-6, 3 * spread), (rms_inl, float(g["ao_rms_inliers"]), spread)


@pytest.mark.parametrize("cfg", ["cfg5", "cfg3", "cfg5_handeye"])
def test_workspace_calibrate_with_a_robust_loss_at_full_size(cfg):
  """Workspace.calibrate(loss='soft_l1', auto_scale=2.0) (workspace.py:239-244: the soft margin re-derived from the error quantile in
  every round) at the stated size under the default solver, against the unmodified reference's run of the same loop."""
  import json
  from multical_amd import Workspace
  g, rig = load_endpoint(cfg)
  if "aor_inliers_packed" not in g:
    pytest.skip("robust outlier loop of the reference not generated (oracle/make_endpoint.py aor)")
  kw = json.loads(str(g["aor_kwargs_json"]))
  out = Workspace(mirror(rig)).calibrate(cameras=rig.optimize["cameras"], camera_poses=rig.optimize["camera_poses"],
                                         loss=kw["loss"], auto_scale=kw["auto_scale"])
  ref_mask = np.unpackbits(g["aor_inliers_packed"])[:rig.valid.size].reshape(rig.valid.shape).astype(bool)
  allowed = int(g["aor_pert_mask_diff"].max()) if "aor_pert_mask_diff" in g else 0     # (what the reference's own perturbed re-runs flip)
  diff = int(np.sum(out.inliers != ref_mask))
  print(f"{cfg}: robust loop: inlier mask differs from the reference's in {diff} observations (reference's own re-runs: up to {allowed})")
  assert diff <= allowed, (diff, allowed)
  spread = float(np.abs(g["aor_pert_rms_inliers"] - g["aor_rms_inliers"]).max()) if "aor_pert_rms_inliers" in g else 0.0
  rms_inl = out.error_statistics(True).rms
  print(f"{cfg}: reference inlier RMS {float(g['aor_rms_inliers']):.9f} (nfev {g['aor_nfev']}, {float(g['aor_seconds']):.0f} s), "
        f"here {rms_inl - float(g['aor_rms_inliers']):+.2e}, reference spread {spread:.1e}")
  assert abs(rms_inl - float(g["aor_rms_inliers"])) <= max(1e-6, 3 * spread)


# ---------------------------------------------------------------------------------------------------------------------------------
# The device's LSMR at the level of ONE lsmr() call (scipy/sparse/linalg/_isolve/lsmr.py:300-420, called at _lsq/trf.py:481)
# ---------------------------------------------------------------------------------------------------------------------------------
CALL_CASES = ["cfg1", "tiny_handeye", "tiny_fixintr", "tiny_rolling", "tiny_fisheye", "tiny_boards", "cfg2", "cfg3_40", "cfg4_40", "cfg5_40",
              "manypairs", "cfg5_handeye"]
# the iteration forms of the LSMR call (Handle.set_lsmr_fused): -1 = automatic (3 on static / hand-eye rigs, 2 with rolling shutter or
# boards=True), 3 = two launches with the per-observation state cached, 2 = two launches, 1 = three, 0 = six
LSMR_FORMS = (-1, 3, 2, 1, 0)


def _load_any(name):
  if name == "cfg5_handeye":                # (full size: the rig is regenerated from its seed, the fixture holds the end points)
    return load_endpoint(name)
  if name in ("cfg2", "cfg3_40", "cfg4_40", "cfg5_40", "manypairs"):
    g = dict(np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False))
    return g, synthetic.make_rig(str(g["config"]))
  return load_golden(name)


def _first_iterate(h, x0):
  """what scipy's trf_no_bounds hands to lsmr in its first iteration (trf.py:420-481): J_h = J diag(d), f, damp"""
  from scipy.optimize._lsq.common import minimize_quadratic_1d
  J, f = h.jacobian(x0), h.residuals(x0)
  si = np.asarray(J.power(2).sum(axis=0)).ravel() ** 0.5
  si[si == 0] = 1
  d = 1 / si
  g_h = d * (J.T @ f)
  Jg = J @ (d * g_h)
  Delta = np.linalg.norm(x0 * si) or 1.0
  ag = minimize_quadratic_1d(0.5 * np.dot(Jg, Jg), -np.dot(g_h, g_h), 0, Delta / np.linalg.norm(g_h))[1]
  return J, f, d, float((-ag / Delta ** 2) ** 0.5)


@pytest.mark.parametrize("name", CALL_CASES)
def test_device_lsmr_first_steps_equal_scipys(name):
  """lsmr(J_h, f, damp, maxiter = k) for the first Golub-Kahan steps, device (mcba_debug_lsmr_solve: lsmr_solve itself, every
  iteration form) against scipy on mcba_jacobian's matrix: the WHOLE return tuple (istop, itn, normr, normar, normA, condA, normx) and
  the solution to 1e-10.  (Only the first steps can be compared that tightly: the bidiagonalisation of these Jacobians loses
  orthogonality after 20 - 40 steps and any two roundings of it -- scipy against scipy with a permuted summation order -- drift apart
  in the third digit of normA; profiles/r06_lsmr_sign.md.)"""
  from scipy.sparse.linalg import lsmr
  from lsmr_emulation import scaled_operator
  g, rig = _load_any(name)
  with Handle(mirror(rig)) as h:
    x0 = g["x0"]
    J, f, d, damp = _first_iterate(h, x0)
    for k in (1, 3, 5) + ((10,) if h.n_params >= 100 else ()):
      ref = lsmr(scaled_operator(J, d), f, damp=damp, maxiter=k)
      for form in LSMR_FORMS:
        h.set_lsmr_fused(form)
        _, scale, _ = h.lsmr_solve(x0, damp, maxiter=1)
        assert np.abs(scale / d - 1).max() <= 1e-11           # (the device's own first-iterate scaling: sqrt of diag(J^T J) from the block records)
        gn, _, info = h.lsmr_solve(x0, damp, scale=d, maxiter=k)
        assert (info["istop"], info["itn"]) == (int(ref[1]), int(ref[2])), (name, k, form, info, ref[1:3])
        for key, r in zip(("normr", "normar", "normA", "condA", "normx"), ref[3:]):
          assert abs(info[key] - r) <= 1e-10 * abs(r), (name, k, form, key, info[key], r)
        assert np.linalg.norm(gn - ref[0]) <= 1e-10 * np.linalg.norm(ref[0]), (name, k, form)


@pytest.mark.parametrize("name", CALL_CASES)
def test_device_lsmr_call_matches_scipy(name, record_property):
  """ONE complete lsmr(J_h, f, damp, atol = btol = 1e-6) call on the first linearisation: the device stops for scipy's reason within a
  few iterations of scipy's count, and its solution solves the damped problem to the SAME level -- measured with the matrix itself
  (host CSR arithmetic), not with either side's recurrence estimates: the true test2 = |A^T r - damp^2 x| / (|A|_F |r|) of the device's
  solution is within a factor 2 of that of scipy's, the damped objectives agree to what the stopping rule leaves open.  The recurrence scalars themselves are
  compared where that is meaningful (test_device_lsmr_first_steps_equal_scipys).  Every iteration form of the call is held to this."""
  from scipy.sparse.linalg import lsmr
  from lsmr_emulation import scaled_operator
  g, rig = _load_any(name)
  calls = {}
  with Handle(mirror(rig)) as h:
    x0 = g["x0"]
    J, f, d, damp = _first_iterate(h, x0)
    for form in LSMR_FORMS:
      h.set_lsmr_fused(form)
      calls[form] = h.lsmr_solve(x0, damp, scale=d)
  ref = lsmr(scaled_operator(J, d), f, damp=damp)
  Jh = J @ __import__("scipy.sparse", fromlist=["diags"]).diags(d)
  normA_F = np.sqrt(Jh.power(2).sum() + damp ** 2 * J.shape[1])

  def true_tests(p):
    r = f - Jh @ p
    rbar = np.sqrt(r @ r + damp ** 2 * (p @ p))
    return np.linalg.norm(Jh.T @ r - damp ** 2 * p) / (normA_F * rbar), 0.5 * rbar ** 2
  t2_ref, obj_ref = true_tests(ref[0])
  for form, (gn, scale, info) in calls.items():
    t2_dev, obj_dev = true_tests(gn)
    record_property(f"form{form}_itn_device_scipy", (info["itn"], int(ref[2])))
    record_property(f"form{form}_true_test2_device_scipy", (float(t2_dev), float(t2_ref)))
    print(f"{name} form {form}: istop {info['istop']} / {ref[1]}, itn {info['itn']} / {ref[2]}, true test2 {t2_dev:.2e} / {t2_ref:.2e}, "
          f"objective rel diff {abs(obj_dev - obj_ref) / obj_ref:.1e}, |x_dev - x_scipy| / |x| {np.linalg.norm(gn - ref[0]) / np.linalg.norm(ref[0]):.1e}")
    assert info["istop"] == int(ref[1]), (form, info, ref[1:3])
    assert abs(info["itn"] - int(ref[2])) <= max(3, 0.02 * int(ref[2])), (form, info["itn"], int(ref[2]))
    # (atol = 1e-6: below a tenth of it both solutions are converged to rounding and the ratio means nothing -- tiny_handeye: 4e-9 / 8e-9)
    assert t2_dev <= 2.0 * t2_ref + 1e-7 and t2_ref <= 2.0 * t2_dev + 1e-7, (form, t2_dev, t2_ref)
    # (two approximate minimisers stopped by the same rule: their objectives differ by what atol = 1e-6 leaves open -- 1e-8 ... 1e-6
    #  relative on these fixtures, more where the call runs into maxiter, istop 7)
    assert abs(obj_dev - obj_ref) <= (1e-5 if info["istop"] in (1, 2) else 1e-3) * obj_ref, form


@pytest.mark.parametrize("name", ["cfg1", "tiny_handeye", "tiny_fixintr", "cfg2", "cfg3_40", "cfg4_40", "cfg5_40", "manypairs", "cfg5_handeye"])
def test_lsmr_call_sequence_of_a_solve(name):
  """the per-trust-region-iteration (istop, itn) sequence of the default solver (mcba_debug_lsmr_trace) against scipy's own TRF + LSMR on
  the device's residuals / Jacobian (tests/lsmr_emulation.trf_lsmr): the same stopping reasons in the same order -- including the
  istop = 7 calls that run into maxiter = n -- and iteration counts within 5 %."""
  from lsmr_emulation import trf_lsmr
  g, rig = _load_any(name)
  with Handle(mirror(rig)) as h:
    calls = []
    trf_lsmr(h.residuals, h.jacobian, g["x0"], solver="scipy", calls=calls)
    h.set_lsmr_trace(True)
    res = h.solve(g["x0"], tr_solver="lsmr")
    trace = h.lsmr_trace()
    total = h.lsmr_iterations()
  assert [c["istop"] for c in trace] == [c["istop"] for c in calls], (trace, [(c["istop"], c["itn"]) for c in calls])
  for a, b in zip(trace, calls):
    # (measured worst case over the eight rigs and the builds of this round: 4 of 133 at cfg5_40 -- a last-bit change of the gradient,
    #  e.g. another summation order in k_shared_final, moves the crossing of a stopping test by a few iterations)
    assert abs(a["itn"] - b["itn"]) <= max(4, 0.05 * b["itn"]), (a["itn"], b["itn"])
    assert np.isfinite([a["normr"], a["normar"], a["normA"], a["condA"], a["normx"]]).all()
  assert sum(c["itn"] for c in trace) == total and res.nfev == int(g["ba_nfev"])


@pytest.mark.parametrize("cfg", ["cfg5", "cfg3", "cfg4", "cfg5_handeye"])
def test_converged_optimum_at_full_size(cfg, record_property):
  """SURVEY 7, protocol C at the STATED sizes of BASELINE configs[2] / [3] / [4]: the converged optimum of the REFERENCE's own residual
  function (tests/golden/cfg*_endpoint.npz: ba_tight_*, oracle/make_endpoint.py tight -- Levenberg-Marquardt on the reference's
  `evaluate`, verified stationary with the reference's own 3-point differences) is reached by the exact-step solver run to tight
  tolerance within 1e-6 px -- the one sense in which "the" end point of these problems is defined beyond the reference's own
  run-to-run spread -- from the reference's end point AND from the initial guess."""
  g, rig = load_endpoint(cfg)
  if "ba_tight_rms" not in g:
    pytest.skip("tight optimum of the reference not generated (oracle/make_endpoint.py tight)")
  tight = float(g["ba_tight_rms"])
  with Handle(mirror(rig)) as h:
    for start in ("x0", "ba_x_raw"):
      res = h.solve(g[start], tolerance=1e-14, xtol=1e-14, gtol=1e-14, max_iterations=400)
      e, v = h.reprojection_error(res.x)
      rms = float(np.sqrt(np.mean(e[v.astype(bool)] ** 2)))
      record_property(f"native_from_{start}_minus_tight_px", rms - tight)
      print(f"{cfg}: tight optimum of the reference {tight:.12f} px; native solver from {start}: {rms - tight:+.2e} px, nfev {res.nfev}, "
            f"cost rel {res.cost / float(g['ba_tight_cost']) - 1:+.1e}")
      assert abs(rms - tight) <= 1e-6, (cfg, start, rms - tight)
      assert res.cost == pytest.approx(float(g["ba_tight_cost"]), rel=1e-9)
    e, v = h.reprojection_error(g["ba_tight_x"])
    assert abs(float(np.sqrt(np.mean(e[v.astype(bool)] ** 2))) - tight) <= 1e-9       # (the device's residuals at the reference's optimum)


def _exact_products():
  import json
  path = os.path.join(GOLDEN, "exact_products.json")
  return json.load(open(path)) if os.path.exists(path) else {}


@pytest.mark.parametrize("name", ["cfg2", "cfg3_40", "cfg4_40", "cfg5_40", "manypairs", "cfg5", "cfg3", "cfg4"])
def test_default_solver_lands_on_scipys_exact_product_end_point(name, record_property):
  """WHY the default solver ends a few 1e-6 px BELOW the reference's single run on every BASELINE-size rig (round-5 review): scipy's own
  algorithm on the reference's residual function (tests/golden/exact_products.json, oracle/make_exact_products.py) ends in two
  clusters -- with scipy.sparse's double products anywhere within ~1e-6 px of the reference's run (that IS the reference's
  arithmetic; its run-to-run spread), and with the same products accumulated in 80-bit precision 1e-7 ... 2.5e-6 px lower, tightly.
  The device's products (per-lane partial sums + tree reductions: a few ulp) are of the second kind: the default solver lands on the
  exact-product end point of scipy's algorithm within 1e-6 px on the 40-frame rigs and 6 x 400 x 5, in every iteration form (at
  8 x 500 x 2 and 16 x 1000 x 5 scipy's own variants spread over 1e-6 px among themselves: the reference's measured spread is the tolerance)."""
  xp = _exact_products().get(name)
  if xp is None or "longdouble_mean_rms" not in xp:
    pytest.skip("exact-product end point not generated (oracle/make_exact_products.py)")
  full = name in ("cfg3", "cfg4", "cfg5")
  g, rig = load_endpoint(name) if full else _load_any(name)
  target = float(xp["longdouble_mean_rms"])
  # 8 x 500 x 2 / 16 x 1000 x 5 at full size: scipy's own variants (double / 80-bit products, row orders) spread over 1e-6 px among
  # themselves there, like the reference's perturbed re-runs (3.4e-6 / 5.7e-6): the resolution is that spread, as for the end point itself
  runs = [r["rms"] for r in xp["runs"]]
  tol = 1e-6 if (max(runs) - min(runs) <= 3e-6 and name not in ("cfg3", "cfg4")) else max(1e-6, endpoint_spread(g))
  with Handle(mirror(rig)) as h:
    for form in LSMR_FORMS:
      h.set_lsmr_fused(form)
      res = h.solve(g["x0"], tr_solver="lsmr")
      e, v = h.reprojection_error(res.x)
      rms = float(np.sqrt(np.mean(e[v.astype(bool)] ** 2)))
      record_property(f"form{form}_minus_exact_product_px", rms - target)
      print(f"{name} form {form}: device - scipy(exact products) {rms - target:+.2e} px; scipy(exact products) - reference "
            f"{xp['longdouble_mean_minus_reference']:+.2e}; scipy(double products, reordered) - reference {xp.get('double_mean_minus_reference', float('nan')):+.2e}")
      assert abs(rms - target) <= tol, (name, form, rms - target, tol)
      assert res.nfev == int(xp["reference_nfev"])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 1023, 1024, 1025, 8 * 1024 + 17, 100_000, 1_527_914])
def test_wide_dot_keeps_the_order_of_additions(n):
  """The three sums of the 2-D subspace step over the m residual rows ([Jg.Jgn | Jg.Jg | Jgn.Jgn], once per trust-region iteration) were ONE
  workgroup walking the vectors (k_dot, 0.49 ms at m = 1.5 M); k_dot3_part / k_dot3_fin put each of its 16 wavefronts on a CU of its own and
  keep every lane's order of additions and the order of the wavefront totals: the same bits for every length, ragged tails included --
  otherwise the trajectories of the chaotic fixtures move (a plain two-stage reduction took tiny_rolling from 22 to 17 evaluations)."""
  import ctypes as C
  from multical_amd import _lib
  lib = _lib.load()
  rng = np.random.default_rng(n)
  a = np.ascontiguousarray(rng.normal(size=max(n, 1)) * np.exp(rng.normal(size=max(n, 1)) * 3))
  b = np.ascontiguousarray(rng.normal(size=max(n, 1)) * np.exp(rng.normal(size=max(n, 1)) * 3))
  single, wide = np.zeros(3), np.zeros(3)
  P = C.POINTER(C.c_double)
  rc = lib.mcba_debug_dot3(a.ctypes.data_as(P), b.ctypes.data_as(P), n, single.ctypes.data_as(P), wide.ctypes.data_as(P))
  assert rc == 0
  assert np.array_equal(single, wide), (single, wide)
  if n > 0:
    want = np.array([np.dot(a[:n], b[:n]), np.dot(a[:n], a[:n]), np.dot(b[:n], b[:n])])
    assert np.allclose(wide, want, rtol=1e-9, atol=1e-9 * np.sqrt(want[1] * want[2]))

