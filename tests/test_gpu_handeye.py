"""GPU (MI355X): the hand-eye motion model (HandEye, motion/hand_eye.py) at full size.

cfg5_handeye is BASELINE configs[4]'s 6 x 400 x 5 fisheye rig driven by `HandEyeCalibration.bundle_adjust`: 12 hand-eye columns
(world_wrt_base, gripper_wrt_camera) plus 30 board-pose columns, no per-frame block (DF = 0), cameras and camera poses held.  No other
full-size rig reaches that regime: the assembly sums chunk partials only, k_shared_final takes its DF == 0 branches, the exact-step
solver eliminates no frames, the covariance has no frame blocks, and the default solver resolves to the cached LSMR form (form 3) with
the static cache layout.  Every comparison here is against an independent reference: the unmodified reference's fixtures
(tests/golden/cfg5_handeye_*.npz), the oracle (oracle/restate.py, pinned to the reference at this size by
tests/test_oracle.py::test_oracle_matches_reference_at_full_size), or sums accumulated in extended precision on the host.
(The residual checksums, end point, outlier loop, tight optimum and single-LSMR-call tests of this rig sit beside those of the other
full-size rigs in tests/test_gpu_parity.py and tests/test_gpu_lsmr.py.)
"""
import math
import os
import socket
import sys

import numpy as np
import pytest

from multical_amd import synthetic, gauge
from multical_amd.backend import Handle
from oracle import restate
from util import mirror, sub_rig, rel_col_error

pytestmark = pytest.mark.gpu

NAME = "cfg5_handeye"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rig():
  r = synthetic.make_rig(NAME)
  assert r.cfg["motion"] == "hand_eye" and r.optimize["camera_poses"] is False and r.optimize["cameras"] is False
  return r


@pytest.fixture(scope="module")
def endpoint():
  from test_gpu_lsmr import load_endpoint
  return load_endpoint(NAME)


def _x1(c):
  """a point away from the initial guess (the normal equations at x0 alone would not see errors that vanish there)"""
  rng = np.random.default_rng(41)
  return c.param_vec + 1e-3 * rng.normal(size=c.param_vec.size)


def _extended(J, r):
  """J^T J, J^T r, J^T |r|, |J|^T |J| and 1/2 r.r with every sum accumulated in long double (42 columns: a dense copy is cheap)"""
  Jd = J.toarray()
  Jl, rl = Jd.astype(np.longdouble), r.astype(np.longdouble)
  A = np.abs(Jd)
  return dict(H=Jl.T @ Jl, g=Jl.T @ rl, Jd=Jd, Jl=Jl, A=A, AA=A.T @ A, Ar=A.T @ np.abs(r),
              cost=0.5 * math.fsum((r * r).tolist()))


def _rel(dev, ref, bound):
  """largest |dev - ref| / bound; entries with bound 0 must be exactly 0 on the device"""
  d = np.abs(dev.astype(np.longdouble) - ref).astype(np.float64)
  assert np.all(d[bound == 0] == 0), "structurally zero entries are not zero"
  live = bound > 0
  return float((d[live] / bound[live]).max()) if live.any() else 0.0


def test_handeye_rig_has_no_frame_block(rig):
  c = mirror(rig)
  assert c.param_vec.size == 12 + 6 * rig.valid.shape[2]                     # 12 hand-eye + 30 board-pose parameters
  with Handle(c) as h:
    assert h.n_params == 42 and h.n_residuals == 2 * int(rig.valid.sum())
    cov = h.covariance(_x1(c), hold=gauge.default_hold(c), frames=True)
  assert cov.shared_index.size == 42 and cov.frame_index.shape == (rig.valid.shape[1], 0)


def test_jacobian_on_a_slice_against_central_differences_of_the_oracle(rig):
  """mcba_jacobian on the first 24 frames (util.sub_rig slices he_base_wrt_gripper) against dense 3-point differences of the oracle:
  per column, at x0 and away from it."""
  from scipy.optimize._numdiff import approx_derivative
  from scipy.sparse import csr_matrix
  sub = sub_rig(rig, 24)
  c = mirror(sub)
  oc = restate.from_rig(sub)
  for x in (c.param_vec, _x1(c)):
    J3 = csr_matrix(approx_derivative(oc.evaluate, x, method='3-point'))
    with Handle(c) as h:
      J = h.jacobian(x)
    assert J.shape == J3.shape == (oc.evaluate(x).size, 42)
    assert rel_col_error(J, J3) < 2e-7
    S = oc.sparsity_matrix.tocsr()
    assert (abs(J) > 0).multiply(S == 0).nnz == 0                             # inside the reference's sparsity pattern


def test_jacobian_directional_derivatives_at_full_size(rig, record_property):
  """J v of mcba_jacobian against (r(x + h v) - r(x - h v)) / 2h of the oracle at the full 345 756 rows, for random directions."""
  c = mirror(rig)
  oc = restate.from_rig(rig)
  rng = np.random.default_rng(43)
  x = _x1(c)
  with Handle(c) as h:
    J = h.jacobian(x)
  worst = 0.0
  for _ in range(3):
    v = rng.normal(size=x.size)
    step = 1e-6
    fd = (oc.evaluate(x + step * v) - oc.evaluate(x - step * v)) / (2 * step)
    jv = J @ v
    worst = max(worst, float(np.abs(jv - fd).max() / np.abs(jv).max()))
  record_property("jv_vs_central_difference_rel", worst)
  assert worst < 2e-7, worst


@pytest.mark.parametrize("mfma", [1, 0])
def test_normal_equations_against_extended_precision_sums(rig, mfma, record_property):
  """H = dense_hessian(), (cost, g, diag) of mcba_normal_equations and of mcba_normal_equations_device against J^T J, J^T r and
  1/2 r.r of mcba_jacobian / mcba_residuals summed in long double: |dH_ij| <= 1e-12 (|J|^T |J|)_ij, |dg_i| <= 1e-12 (|J|^T |r|)_i --
  every entry, structurally zero ones exactly zero (no frame block: all 345 756 rows land in the dense 42 x 42 part)."""
  c = mirror(rig)
  worst = {}
  with Handle(c) as h:
    h.set_mfma(mfma)
    for tag, x in (("x0", c.param_vec), ("x1", _x1(c))):
      J, r = h.jacobian(x), h.residuals(x)
      ref = _extended(J, r)
      cost, g, diag = h.normal_equations(x)
      H = h.dense_hessian()
      assert np.array_equal(H, H.T)
      eH = _rel(H, ref["H"], ref["AA"])
      eg = _rel(g, ref["g"], ref["Ar"])
      ed = _rel(diag, np.diagonal(ref["H"]), np.diagonal(ref["AA"]))
      ec = abs(cost - ref["cost"]) / ref["cost"]
      worst[tag] = (eH, eg, ed, ec)
      assert eH <= 1e-12 and ed <= 1e-12, (tag, eH, ed)
      assert eg <= 1e-12, (tag, eg)
      assert ec <= 1e-12, (tag, ec)
      # the enqueued form at the x already on the device: the same numbers
      h.normal_equations_device()
      h.synchronize()
      assert np.array_equal(h.dense_hessian(), H)
  record_property("max_rel_H_g_diag_cost", worst)
  print(f"{NAME} mfma={mfma}: " + ", ".join(f"{k}: H {v[0]:.1e} g {v[1]:.1e} diag {v[2]:.1e} cost {v[3]:.1e}" for k, v in worst.items()))


@pytest.mark.parametrize("form", [2, 3])
def test_lsmr_products_against_extended_precision_sums(rig, form, record_property):
  """the matrix-free products of the LSMR iteration -- mcba_debug_lsmr_products (J v, J^T u) and mcba_debug_lsmr_fused_products
  (J v, J^T J v) in form 2 and in the cached form 3 (one pass fills the per-observation cache in the static layout, the pass under test
  streams it back) -- against the same products of mcba_jacobian in long double: |d(Jv)_i| <= 1e-12 (|J| |v|)_i,
  |d(J^T u)_j| <= 1e-12 (|J|^T |u|)_j, |d(J^T J v)_j| <= 1e-11 (|J|^T |J| |v|)_j."""
  c = mirror(rig)
  rng = np.random.default_rng(47 + form)
  worst = [0.0, 0.0, 0.0]
  for x in (c.param_vec, _x1(c)):
    with Handle(c) as h:
      J = h.jacobian(x)
      v = rng.normal(size=h.n_params)
      u = rng.normal(size=h.n_residuals)
      jv, jtu = h.lsmr_products(x, v, u)
      h.set_lsmr_fused(form)
      fjv, w = h.lsmr_fused_products(x, v)
      fjv2, w2 = h.lsmr_fused_products(x, v)
      h.set_lsmr_fused(2)
      bjv, bw = h.lsmr_fused_products(x, v)
    Jd = J.toarray()
    Jl = Jd.astype(np.longdouble)
    A = np.abs(Jd)
    ref_jv = Jl @ v.astype(np.longdouble)
    bound_jv = A @ np.abs(v)
    worst[0] = max(worst[0], _rel(jv, ref_jv, bound_jv), _rel(fjv, ref_jv, bound_jv))
    worst[1] = max(worst[1], _rel(jtu, Jl.T @ u.astype(np.longdouble), A.T @ np.abs(u)))
    worst[2] = max(worst[2], _rel(w, Jl.T @ ref_jv, A.T @ bound_jv))
    assert np.array_equal(fjv, fjv2) and np.array_equal(w, w2)               # deterministic
    assert np.array_equal(fjv, bjv) and np.array_equal(w, bw)                # the cached form is the same arithmetic: same bits
  record_property("max_rel_jv_jtu_jtjv", worst)
  print(f"{NAME} form {form}: J v {worst[0]:.1e}, J^T u {worst[1]:.1e}, J^T J v {worst[2]:.1e}")
  assert worst[0] <= 1e-12 and worst[1] <= 1e-12 and worst[2] <= 1e-11, worst


def test_default_solver_end_point_in_every_lsmr_form(rig, endpoint, record_property):
  """Calibration.bundle_adjust's default solver against the unmodified reference's HandEyeCalibration.bundle_adjust end point: the
  automatic form (-1, which resolves to the cached form 3 on this rig), 3, 2, 1 and 0 take the reference's nfev / status and land within
  max(1e-6 px, the reference's own spread under 1e-12 px perturbations) of its RMS; -1, 3 and 2 return the same bits."""
  from test_gpu_lsmr import endpoint_spread
  g, _ = endpoint
  c = mirror(rig)
  assert np.array_equal(c.param_vec, g["x0"])
  ref, spread = float(g["ba_rms"]), endpoint_spread(g)
  xs, out = {}, {}
  with Handle(c) as h:
    for form in (-1, 3, 2, 1, 0):
      h.set_lsmr_fused(form)
      res = h.solve(g["x0"], tr_solver="lsmr")
      e, v = h.reprojection_error(res.x)
      rms = float(np.sqrt(np.mean(e[v.astype(bool)] ** 2)))
      xs[form], out[form] = res.x, (res.nfev, res.status, rms - ref)
      record_property(f"form{form}_minus_reference_px", rms - ref)
  record_property("reference_spread_px", spread)
  print(f"{NAME}: reference {ref:.9f} px (nfev {int(g['ba_nfev'])}, {float(g['ba_seconds']):.0f} s on the host), spread {spread:.1e}; "
        + ", ".join(f"form {f}: {o[2]:+.2e} px nfev {o[0]}" for f, o in out.items()))
  for form, (nfev, status, d) in out.items():
    assert (nfev, status) == (int(g["ba_nfev"]), int(g["ba_status"])), (form, out[form])
    assert abs(d) <= max(1e-6, spread), (form, d, spread)
  assert np.array_equal(xs[-1], xs[3]) and np.array_equal(xs[3], xs[2]), (np.abs(xs[-1] - xs[3]).max(), np.abs(xs[3] - xs[2]).max())


def test_covariance_without_frame_blocks_matches_scipy(rig):
  """mcba_covariance with K = 0 eliminated frame blocks (no k_schur_frame, no SYRK): the whole 42 x 42 covariance against scipy's
  Cholesky of the dense H at the solution, gauge.default_hold (the first board's pose)."""
  from test_gpu_covariance import _compare, _solve
  c = mirror(rig)
  hold = gauge.default_hold(c)
  assert hold.sum() == 6
  with Handle(c) as h:
    x = _solve(h, c.param_vec)
    cost, _, _ = h.normal_equations(x)
    H = h.dense_hessian()
    cov = _compare(h, x, hold, H, h.n_residuals, 2.0 * cost, 1e-7, cross=True)
  assert cov.frames.shape == (rig.valid.shape[1], 0, 0) and np.all(np.isfinite(cov.std))


# ---- two ranks on one GPU (frame shards; DF = 0: every message is made of shared entries only) ------------------------------------
def _free_port():
  s = socket.socket()
  s.bind(("127.0.0.1", 0))
  p = s.getsockname()[1]
  s.close()
  return p


def _sharded_worker(rank, world, port, out):
  sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
  import faulthandler
  faulthandler.dump_traceback_later(240, exit=True)      # a deadlocked collective must end the test with a traceback, not stall it
  import torch
  import torch.distributed as dist
  from multical_amd import distributed as mdist, synthetic as syn
  from util import mirror as mir
  os.environ["MASTER_ADDR"] = "127.0.0.1"
  os.environ["MASTER_PORT"] = str(port)
  torch.cuda.set_device(0)
  dist.init_process_group("gloo", rank=rank, world_size=world, timeout=__import__("datetime").timedelta(seconds=60))
  c = mir(syn.make_rig(NAME))
  x0 = c.param_vec
  h = mdist.sharded_handle(c)
  h.set_allreduce_trace(1 << 20)
  rec = {}
  for solver in ("lsmr", "exact"):
    h.allreduce_stats(reset=True)
    res = h.solve(x0, tr_solver=solver)
    sizes = h.allreduce_stats(reset=True, cap=1 << 20)[2]
    e, v = h.reprojection_error(res.x)
    sq = torch.tensor([float((e[v] ** 2).sum()), float(v.sum())], dtype=torch.float64)
    dist.all_reduce(sq)
    rec[solver] = dict(x=res.x, nfev=res.nfev, status=res.status, rms=float(np.sqrt(sq[0] / sq[1])), sizes=np.array(sizes))
  if rank == 0:
    np.savez(out, **{f"{s}_{k}": v for s, d in rec.items() for k, v in d.items()})
  h.close()
  dist.destroy_process_group()


def test_frame_sharded_solves_on_two_ranks(rig, tmp_path):
  import torch.multiprocessing as mp
  out = str(tmp_path / "sharded_handeye.npz")
  mp.spawn(_sharded_worker, args=(2, _free_port(), out), nprocs=2, join=True)
  sh = np.load(out)
  c = mirror(rig)
  ns = c.param_vec.size
  with Handle(c) as h:
    single = {}
    for solver in ("lsmr", "exact"):
      res = h.solve(c.param_vec, tr_solver=solver)
      e, v = h.reprojection_error(res.x)
      single[solver] = (res, float(np.sqrt(np.mean(e[v] ** 2))))
  res, rms = single["lsmr"]
  assert (int(sh["lsmr_nfev"]), int(sh["lsmr_status"])) == (res.nfev, res.status)
  assert abs(float(sh["lsmr_rms"]) - rms) <= 1e-6
  res, rms = single["exact"]
  assert (int(sh["exact_nfev"]), int(sh["exact_status"])) == (res.nfev, res.status)
  assert np.abs(sh["exact_x"] - res.x).max() <= 1e-7
  assert abs(float(sh["exact_rms"]) - rms) < 1e-9
  # no message carries a frame entry: with DF = 0 every parameter is shared (the sizes of the sharded tests of tests/test_distributed.py
  # with n_motion = 0)
  G, S = 2 * ns + 6, ns * ns + ns
  assert set(int(v) for v in sh["exact_sizes"]) <= {G, S, 4 * 2, 3 * 2 + 1, 4}, sorted(set(int(v) for v in sh["exact_sizes"]))
  assert set(int(v) for v in sh["lsmr_sizes"]) <= {G, 4 * 2, 1, ns, 6, 4, ns + 5}, sorted(set(int(v) for v in sh["lsmr_sizes"]))
