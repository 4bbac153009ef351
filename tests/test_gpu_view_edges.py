"""GPU (MI355X): the per-view kernels -- k_linearize, k_residual, k_cost, k_lsmr_jv / jtu / fused / fused2 -- at every edge of their
64-observation chunks, on all 42 view shapes they are instantiated for (7 camera units x 3 motion models x {intrinsics optimised,
fixed}) and on three rigs whose 816-point board is walked in two segments.  The rigs come from tests/planted_rigs.py: views of
1, 2, 4, 5, 8, 9, 60, 61, 63, 64, 65, 68, 127, 128, 129, 192, 256 and 257 inliers on both cameras next to empty ones.

Which kernel a test reaches: k_residual and k_jacobian in test_forward_pass; k_linearize in test_normal_equations, test_each_count_isolated,
test_several_views_per_workgroup, test_robust_instantiation and test_switch_forced_forms; k_lsmr_jv / k_lsmr_jtu (+ k_lsmr_gather) and
k_lsmr_fused2 (+ k_lsmr_gather3) in test_lsmr_products; k_lsmr_fused (+ k_lsmr_gather2), which only an LSMR solve launches, in
test_lsmr_first_steps; k_cost in test_trial_step_cost (plain-FMA handle: every trial step) and in the solves of
test_switch_forced_forms (MCBA_FUSED=0: main stream, MCBA_SPEC_ACCEPT=0: side stream).  The per-view kernels iterate the list of
ACTIVE views: the empty views of these rigs are met by the slot-parallel kernels (k_residual's table form, k_jacobian), by the view
tables and by the compaction only.

References: the oracle (oracle/restate.py, pinned bit for bit to the reference on these rigs by tests/test_oracle_vs_reference.py), its
3-point differences, and the host build of the product's device functions (tests/hostmath, pinned to the oracle on these rigs by
tests/test_planted_rigs_host.py).  Tolerances are the project's own: 1e-9 px residuals, 1e-12 relative cost, 1e-12 max for H /
gradient / diagonal against the host build, 1e-11 max against J^T J of the device Jacobian, 1e-12 sum |J||v| for J v and 1e-11 for
J^T J v, 1e-10 for the first LSMR steps against scipy's.  No convergence claim is made anywhere: frames with fewer residuals than
parameters are in these rigs on purpose.  Every test records the largest observed error / tolerance ratio (`max_ratio`)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import planted_rigs as pr
from hostmath_lib import HostMath
from multical_amd.backend import Handle
from oracle import restate
from util import mirror, rel_col_error

pytestmark = pytest.mark.gpu

EDGES = [("edges",) + s for s in pr.SHAPES]
BIG = [("bigboard",) + s for s in pr.BIG_SHAPES]
ids = lambda rigs: [r[0] + "-" + pr.shape_id(r[1:]) for r in rigs]
all_rigs = pytest.mark.parametrize("key", EDGES + BIG, ids=ids(EDGES + BIG))
edge_rigs = pytest.mark.parametrize("key", EDGES, ids=ids(EDGES))


class Case(object):
  """One planted rig with its references; everything is computed once, shared by the tests and left unchanged."""

  def __init__(self, key):
    kind, unit, motion, optk = key
    self.kind = kind
    self.rig, self.planted = (pr.planted_rig if kind == "edges" else pr.planted_bigboard)(unit, motion, optk)
    self.c = mirror(self.rig)
    self.oc = restate.from_rig(self.rig)
    x0 = self.c.param_vec
    assert np.array_equal(x0, self.oc.param_vec)
    self.xs = [x0, x0 + 1e-3 * np.random.default_rng(5).normal(size=x0.size)]
    self.hm = HostMath(self.c)

  @functools.lru_cache(maxsize=None)
  def r(self, i):
    return self.oc.evaluate(self.xs[i])

  @functools.lru_cache(maxsize=None)
  def host(self, i):
    """(H, g, cost) of the host build"""
    return self.hm.normal_equations(self.xs[i])

  @functools.lru_cache(maxsize=None)
  def sparsity(self):
    from scipy.sparse import csr_matrix
    return csr_matrix(self.oc.sparsity_matrix)

  @functools.lru_cache(maxsize=None)
  def differences(self, i):
    from scipy.optimize._numdiff import approx_derivative, group_columns
    from scipy.sparse import csr_matrix
    S = self.sparsity()
    return csr_matrix(approx_derivative(self.oc.evaluate, self.xs[i], method='3-point', sparsity=(S, group_columns(S))))


@functools.lru_cache(maxsize=None)
def case(key):
  return Case(key)


class Worst(object):
  """largest error / tolerance ratio of a test"""

  def __init__(self):
    self.ratio = 0.0

  def check(self, err, tol, what):
    err, tol = float(err), float(tol)
    ratio = err / tol if tol > 0 else (0.0 if err == 0 else np.inf)
    self.ratio = max(self.ratio, ratio)
    assert err <= tol, (what, err, tol)

  def close(self, got, want, rel, what, scale=None):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    s = float(np.abs(want).max(initial=0.0)) if scale is None else float(scale)
    self.check(np.abs(got - want).max(initial=0.0), rel * s, what)


@pytest.fixture
def worst(record_property):
  w = Worst()
  yield w
  record_property("max_ratio", w.ratio)


def check_normal_equations(w, cs, h, i, tag):
  """cost / gradient / diagonal / H of the handle's current configuration at point i against the host build and the oracle"""
  Hh, gh, _ = cs.host(i)
  r = cs.r(i)
  cost, grad, diag = h.normal_equations(cs.xs[i])
  H = h.dense_hessian()
  w.check(abs(cost - 0.5 * r @ r), 1e-12 * 0.5 * r @ r, (tag, "cost"))
  w.close(grad, gh, 1e-12, (tag, "gradient"))
  w.close(H, Hh, 1e-12, (tag, "H"))
  w.close(diag, np.diag(Hh), 1e-12, (tag, "diagonal"), scale=np.abs(Hh).max())
  assert np.array_equal(H, H.T), tag
  return cost, grad, diag, H


@all_rigs
def test_forward_pass(key, worst):
  """k_residual, the error table and k_jacobian: residuals and errors against the oracle, the Jacobian against the oracle's 3-point
  differences (2e-7 per column), against the host build (1e-11 max) and inside the oracle's sparsity pattern."""
  cs, w = case(key), worst
  with Handle(cs.c) as h:
    assert h.n_params == cs.xs[0].size
    assert h.n_residuals == 2 * int(cs.rig.valid.sum())
    for i, x in enumerate(cs.xs):
      r = h.residuals(x)
      assert r.shape == cs.r(i).shape
      w.check(np.abs(r - cs.r(i)).max(), 1e-9, ("residuals", i))
      err, valid = h.reprojection_error(x)
      eo, vo = cs.oc.with_param_vec(x).reprojection_error_table()
      assert np.array_equal(valid, vo)
      w.check(np.abs(err[vo] - eo[vo]).max(), 1e-9, ("error table", i))
      J = h.jacobian(x)
      J3 = cs.differences(i)
      assert J.shape == J3.shape
      w.check(rel_col_error(J, J3), 2e-7, ("J against 3-point differences", i))
      Jh = cs.hm.jacobian(x)
      w.check(np.abs((J - Jh)).max(), 1e-11 * np.abs(Jh).max(), ("J against the host build", i))
      nz = abs(J) > 0
      assert nz.multiply(cs.sparsity() != 0).nnz == nz.nnz                   # inside the oracle's sparsity pattern


@pytest.mark.parametrize("mfma", [1, 0])
@all_rigs
def test_normal_equations(key, mfma, worst):
  """k_linearize + assembly against the host build: the MFMA kernel (table-fed fused form over the compacted tables) and the plain-FMA
  one (table form with k_tmat, generic-loss instantiation)."""
  cs, w = case(key), worst
  with Handle(cs.c) as h:
    h.set_mfma(mfma)
    for i, x in enumerate(cs.xs):
      cost, grad, diag, H = check_normal_equations(w, cs, h, i, i)
      J = h.jacobian(x)
      JtJ = (J.T @ J).toarray()
      w.close(H, JtJ, 1e-11, ("H against J^T J", i))
      w.close(grad, J.T @ cs.r(i), 1e-11, ("gradient against J^T r", i))


@edge_rigs
def test_each_count_isolated(key, worst):
  """One wrong observation in a 1-observation view must not hide under the norm of a 257-observation view: for every planted count
  the inlier set is cut to the views of that count alone; cost against the oracle under the same mask, gradient and H against
  J_k^T r_k and J_k^T J_k of the device Jacobian under that mask (slot-parallel, independent of the chunking), scaled by the subset's
  own maxima; columns no remaining view touches exactly zero.  Then the empty set, and the full set again: bit for bit what the
  handle returned before the masks."""
  cs, w = case(key), worst
  with Handle(cs.c) as h:
    before = [(h.normal_equations(x), h.dense_hessian()) for x in cs.xs]
    for k, views in cs.planted.items():
      mask = pr.view_mask(cs.rig, views)
      assert int(mask.sum()) == k * len(views)
      h.set_inliers(mask)
      assert h.n_residuals == 2 * k * len(views)
      ock = cs.oc.copy(inlier_mask=mask)
      for i, x in enumerate(cs.xs):
        rk = ock.evaluate(x)
        w.check(np.abs(h.residuals(x) - rk).max(), 1e-9, ("residuals", k, i))
        Jk = h.jacobian(x)
        cost, grad, diag = h.normal_equations(x)
        H = h.dense_hessian()
        w.check(abs(cost - 0.5 * rk @ rk), 1e-12 * 0.5 * rk @ rk, ("cost", k, i))
        JtJ = (Jk.T @ Jk).toarray()
        w.close(H, JtJ, 1e-11, ("H", k, i))
        w.close(diag, np.diag(JtJ), 1e-11, ("diagonal", k, i), scale=np.abs(JtJ).max())
        w.close(grad, Jk.T @ rk, 1e-11, ("gradient", k, i))
        assert np.array_equal(H, H.T)
        untouched = np.asarray(abs(Jk).sum(axis=0)).ravel() == 0        # (none under hand-eye with everything else fixed)
        assert not grad[untouched].any() and not diag[untouched].any(), (k, i)
        assert not H[untouched].any() and not H[:, untouched].any(), (k, i)
    h.set_inliers(np.zeros(cs.rig.valid.shape, dtype=bool))
    assert h.n_residuals == 0 and h.residuals(cs.xs[0]).size == 0
    cost, grad, diag = h.normal_equations(cs.xs[0])
    assert cost == 0.0 and not grad.any() and not diag.any() and not h.dense_hessian().any()
    h.set_inliers(cs.rig.valid)
    for x, ((cost0, grad0, diag0), H0) in zip(cs.xs, before):
      cost, grad, diag = h.normal_equations(x)
      assert cost == cost0 and np.array_equal(grad, grad0) and np.array_equal(diag, diag0)
      assert np.array_equal(h.dense_hessian(), H0)


@pytest.mark.parametrize("grid", [1, 2, 3])
@all_rigs
def test_several_views_per_workgroup(key, grid, worst):
  """A persistent workgroup carries staging rows, accumulators, the VALU head and tail, the prefetched observation and the time-shared
  buffer from one view into the next.  With one workgroup a single wavefront walks the whole list of active views in its order:
  classes of ceil(count / 64) chunks, largest class first, view-index order inside a class (k_active_count / k_active_scatter) --
  here 257, 257, 256, 256, then 192 and 129 mixed, then 65 .. 128 mixed, then 1 .. 64 mixed, so a view of one chunk follows a view of
  two, a tail of 1 follows a full chunk of 64, and so on; views without inliers are not in the list.  With two and three workgroups
  the neighbours change.  Same references and tolerances as with one view per workgroup, and cost and H within 1e-12 of the default
  grid."""
  cs, w = case(key), worst
  with Handle(cs.c) as h:
    for mfma in (1, 0):
      h.set_mfma(mfma)
      h.set_lin_grid(0)
      default = [(h.normal_equations(x)[0], h.dense_hessian()) for x in cs.xs]
      h.set_lin_grid(grid)
      for i in range(len(cs.xs)):
        cost, grad, diag, H = check_normal_equations(w, cs, h, i, (mfma, i))
        w.check(abs(cost - default[i][0]), 1e-12 * default[i][0], ("cost against the default grid", mfma, i))
        w.close(H, default[i][1], 1e-12, ("H against the default grid", mfma, i))


@all_rigs
def test_lsmr_products(key, worst):
  """k_lsmr_jv / k_lsmr_jtu / k_lsmr_gather and the kernels of the default iteration, k_lsmr_fused2 / k_lsmr_gather3, in their three
  forms (cached state, evaluating, masks form) and with one and two persistent workgroups, against the device Jacobian.  (Settings 1
  and 0 of set_lsmr_fused are issued as the issue lists them; in this hook they launch the evaluating kernel of setting 2 again --
  k_lsmr_fused itself is reached by test_lsmr_first_steps.)"""
  cs, w = case(key), worst
  rng = np.random.default_rng(8)
  with Handle(cs.c) as h:
    for i, x in enumerate(cs.xs):
      J = h.jacobian(x)
      A = abs(J)
      v, u = rng.normal(size=h.n_params), rng.normal(size=h.n_residuals)
      sv, su = (A @ np.abs(v)).max(), A.T @ np.abs(u)
      jv, jtu = h.lsmr_products(x, v, u)
      jv_only, _ = h.lsmr_products(x, v, None)
      _, jtu_only = h.lsmr_products(x, None, u)
      w.check(np.abs(jv - J @ v).max(), 1e-12 * sv, ("J v", i))
      w.check(np.abs(jtu - J.T @ u).max(), 1e-12 * su.max(), ("J^T u", i))
      assert not jtu[su == 0].any()
      assert np.array_equal(jv, jv_only) and np.array_equal(jtu, jtu_only)
      ref = J @ v
      sw = A.T @ np.abs(ref)

      def fused(tag):
        jv, wv = h.lsmr_fused_products(x, v)
        w.check(np.abs(jv - ref).max(), 1e-12 * sv, ("fused J v", tag, i))
        w.check(np.abs(wv - J.T @ ref).max(), 1e-11 * sw.max(), ("fused J^T J v", tag, i))
        assert not wv[sw == 0].any(), (tag, i)
        return jv, wv

      out = {}
      for mode in (3, 2, 1, 0):
        h.set_lsmr_fused(mode)
        out[mode] = fused(mode)
      h.set_lsmr_fused(2)
      h.set_lsmr_masks_form(True)
      out["masks"] = fused("masks")
      h.set_lsmr_masks_form(False)
      assert np.array_equal(out[2][0], out[3][0]) and np.array_equal(out[2][1], out[3][1])     # the cached state: same arithmetic
      if cs.kind == "edges":
        assert np.array_equal(out[2][0], out["masks"][0]) and np.array_equal(out[2][1], out["masks"][1])
      else:   # (the masks form walks the big board in segments and deals its observations to other lanes)
        w.check(np.abs(out[2][0] - out["masks"][0]).max(), 1e-12 * sv, ("masks form J v", i))
        w.check(np.abs(out[2][1] - out["masks"][1]).max(), 1e-11 * sw.max(), ("masks form J^T J v", i))
      for grid in (1, 2):
        h.set_lsmr_grid(grid)
        fused(("grid", grid))
        jv_g, jtu_g = h.lsmr_products(x, v, u)
        w.check(np.abs(jv_g - J @ v).max(), 1e-12 * sv, ("J v", "grid", grid, i))
        w.check(np.abs(jtu_g - J.T @ u).max(), 1e-12 * su.max(), ("J^T u", "grid", grid, i))
        assert not jtu_g[su == 0].any()
      h.set_lsmr_grid(2048)
      h.set_lsmr_fused(-1)


@all_rigs
def test_robust_instantiation(key, worst):
  """The Huber instantiation of k_linearize with the scale at the median |r|, so that both branches of the loss are taken within the
  views of every count; against scipy's own scaling of the device Jacobian and the oracle's residuals."""
  from scipy.optimize._lsq.least_squares import construct_loss_function
  from scipy.optimize._lsq.common import scale_for_robust_loss_function
  cs, w = case(key), worst
  with Handle(cs.c) as h:
    for i, x in enumerate(cs.xs):
      f = cs.r(i)
      s = float(np.median(np.abs(f)))
      linear = np.mean((f / s) ** 2 <= 1.0)
      assert 0.2 <= linear <= 0.8, linear
      J = h.jacobian(x).toarray()
      cost, grad, diag = h.normal_equations(x, loss="huber", f_scale=s)
      H = h.dense_hessian()
      rho = construct_loss_function(f.size, "huber", s)(f)
      Js, fs = scale_for_robust_loss_function(J.copy(), f.copy(), rho)
      w.check(abs(cost - 0.5 * np.sum(rho[0])), 1e-12 * 0.5 * np.sum(rho[0]), ("cost", i))
      w.check(np.abs(H - Js.T @ Js).max(), 1e-11 * np.abs(H).max(), ("H", i))
      w.check(np.abs(grad - Js.T @ fs).max(), 1e-11 * np.abs(grad).max(), ("gradient", i))
      assert np.array_equal(H, H.T)


@all_rigs
def test_lsmr_first_steps(key, worst):
  """k_lsmr_fused (three-launch iteration) and the six-launch iteration are only launched by an LSMR solve: lsmr(J_h, f, damp,
  maxiter = k) for k = 1 and 3 Golub-Kahan steps on the first linearisation, every iteration form, against scipy on the device
  Jacobian -- stopping reason, iteration count, the five norms and the solution to 1e-10, the bound
  test_gpu_lsmr.py::test_device_lsmr_first_steps_equal_scipys holds the same call to on the fixtures (a bound on the first steps of
  the bidiagonalisation, no convergence claim) -- and once more with ONE persistent workgroup walking all views."""
  from scipy.sparse.linalg import lsmr
  from lsmr_emulation import scaled_operator
  from test_gpu_lsmr import _first_iterate
  cs, w = case(key), worst
  x0 = cs.xs[0]
  with Handle(cs.c) as h:
    J, f, d, damp = _first_iterate(h, x0)
    for k in (1, 3):
      ref = lsmr(scaled_operator(J, d), f, damp=damp, maxiter=k)
      for form, grid in [(3, 2048), (2, 2048), (1, 2048), (0, 2048), (2, 1), (1, 1), (0, 1)]:
        h.set_lsmr_fused(form)
        h.set_lsmr_grid(grid)
        gn, _, info = h.lsmr_solve(x0, damp, scale=d, maxiter=k)
        assert (info["istop"], info["itn"]) == (int(ref[1]), int(ref[2])), (k, form, grid, info, ref[1:3])
        for name, r in zip(("normr", "normar", "normA", "condA", "normx"), ref[3:]):
          w.check(abs(info[name] - r), 1e-10 * abs(r), (k, form, grid, name))
        w.check(np.linalg.norm(gn - ref[0]), 1e-10 * np.linalg.norm(ref[0]), (k, form, grid, "solution"))


@all_rigs
def test_trial_step_cost(key, worst):
  """k_cost evaluates trial steps of the exact-step solver: the cost the solve reports is the oracle's at the point it returns.
  On a default handle an accepted step takes its cost from the speculative k_linearize at the new point and k_cost only runs on a
  retry; on a plain-FMA handle (set_mfma(0): no speculation) EVERY trial step is evaluated by k_cost on the main stream.  Both are
  run with max_iterations = 2 (one trial step) and 5 (up to four, retries included).  The plain-FMA solve of 5 evaluations must have
  moved: then the cost it reports is one k_cost formed -- a statement about which kernel the test reaches (one of four trial steps
  from the perturbed truth reduces the cost), not about where the solve ends."""
  cs, w = case(key), worst
  x0 = cs.xs[0]
  with Handle(cs.c) as h:
    for mfma in (1, 0):
      h.set_mfma(mfma)
      for iterations in (2, 5):
        res = h.solve(x0, max_iterations=iterations)
        ro = cs.oc.evaluate(res.x)
        assert np.isfinite(res.cost) and 1 <= res.nfev <= iterations
        w.check(abs(res.cost - 0.5 * ro @ ro), 1e-10 * 0.5 * ro @ ro, ("cost of the returned point", mfma, iterations))
        if mfma == 0 and iterations == 5:
          assert not np.array_equal(res.x, x0) and res.cost < res.initial_cost, (iterations, res.nfev, res.cost, res.initial_cost)


SWITCH_CODE = r"""
import sys, os, numpy as np
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import planted_rigs as pr
from util import mirror
from multical_amd.backend import Handle
from multical_amd import _lib
out_path, switch, kind, unit = sys.argv[1:5]
if switch != "default":
  _lib.set_switch(*switch.split("="))
shapes = pr.BIG_SHAPES if kind == "bigboard" else [s for s in pr.SHAPES if s[0] == unit]
out = {}
for s in shapes:
  rig, _ = (pr.planted_bigboard if kind == "bigboard" else pr.planted_rig)(*s)
  c = mirror(rig)
  x0 = c.param_vec
  xs = [x0, x0 + 1e-3 * np.random.default_rng(5).normal(size=x0.size)]
  with Handle(c) as h:
    for grid in (0, 1):          # one view per workgroup, and ONE workgroup that walks them all
      h.set_lin_grid(grid)
      for i, x in enumerate(xs):
        cost, grad, diag = h.normal_equations(x)
        key = pr.shape_id(s) + "/" + str(i) + "/" + str(grid)
        out[key + "/cost"], out[key + "/grad"], out[key + "/diag"], out[key + "/H"] = cost, grad, diag, h.dense_hessian()
    h.set_lin_grid(0)
    for iterations in (2, 5):    # trial steps of the exact-step solver (k_cost under MCBA_FUSED=0 and MCBA_SPEC_ACCEPT=0)
      res = h.solve(x0, max_iterations=iterations)
      key = pr.shape_id(s) + "/solve" + str(iterations)
      out[key + "/x"], out[key + "/cost"], out[key + "/initial_cost"] = res.x, res.cost, res.initial_cost
np.savez(out_path, **out)
"""
SWITCHES = ["default", "MCBA_LIN_COMPACT=0", "MCBA_FUSED=0", "MCBA_SPEC_ACCEPT=0"]
K_COST_SWITCHES = ["MCBA_FUSED=0", "MCBA_SPEC_ACCEPT=0"]     # every trial step evaluated by k_cost: main stream / side stream


def run_switches(tmp_path, kind, unit):
  """cost / gradient / diagonal / H of the rigs under the default linearisation and under each forcing switch, one process each (a switch
  is read once per process); a process that fails ends the test before the next one starts"""
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  env = {k: v for k, v in os.environ.items() if not k.startswith("MCBA_")}
  res = {}
  for sw in SWITCHES:
    path = str(tmp_path / (sw.replace("=", "_") + ".npz"))
    p = subprocess.run([sys.executable, "-c", SWITCH_CODE, path, sw, kind, unit], cwd=root, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (sw, p.returncode, p.stderr[-2000:])
    res[sw] = dict(np.load(path))
  return res


def check_switch_forced(w, res, shapes, kind):
  default, masks, table, side = (res[sw] for sw in SWITCHES)
  assert set(default) == set(masks) == set(table) == set(side) and len(default) == (16 + 6) * len(shapes)
  for s in shapes:
    cs = case((kind,) + s)
    for sw in SWITCHES:
      for iterations in (2, 5):
        key = pr.shape_id(s) + "/solve" + str(iterations)
        x, cost = res[sw][key + "/x"], float(res[sw][key + "/cost"])
        ro = cs.oc.evaluate(x)
        w.check(abs(cost - 0.5 * ro @ ro), 1e-10 * 0.5 * ro @ ro, (sw, key, "cost of the returned point"))
        if sw in K_COST_SWITCHES and iterations == 5:     # the solve moved: the reported cost is one k_cost formed (see test_trial_step_cost)
          assert not np.array_equal(x, cs.xs[0]) and cost < float(res[sw][key + "/initial_cost"]), (sw, key)
    for i, grid in [(0, 0), (1, 0), (0, 1), (1, 1)]:
      key = pr.shape_id(s) + "/" + str(i) + "/" + str(grid)
      Hh, gh, _ = cs.host(i)
      r = cs.r(i)
      for sw in SWITCHES:
        a = res[sw]
        w.check(abs(float(a[key + "/cost"]) - 0.5 * r @ r), 1e-12 * 0.5 * r @ r, (sw, key, "cost"))
        w.close(a[key + "/grad"], gh, 1e-12, (sw, key, "gradient"))
        w.close(a[key + "/H"], Hh, 1e-12, (sw, key, "H"))
        w.close(a[key + "/diag"], np.diag(Hh), 1e-12, (sw, key, "diagonal"), scale=np.abs(Hh).max())
      for q in ("cost", "grad", "diag", "H"):
        a, m, t = default[key + "/" + q], masks[key + "/" + q], table[key + "/" + q]
        if kind == "edges":     # same lane of the same chunk for every observation in forms 2 and 3: the same bits
          assert np.array_equal(a, m), (key, q)
        else:                   # (form 2 walks the big board in segments: other chunk boundaries)
          w.close(m, a, 1e-12, ("masks form against the default", key, q), scale=np.abs(default[key + "/" + ("H" if q == "diag" else q)]).max())
        w.close(t, a, 1e-11, ("table form against the default", key, q), scale=np.abs(default[key + "/" + ("H" if q == "diag" else q)]).max())


@pytest.mark.parametrize("unit", list(pr.UNITS))
def test_switch_forced_forms(unit, tmp_path, worst):
  """The forms of k_linearize the default never takes on these rigs, each forced with its switch in a process of its own, on the six
  rigs of a camera unit: the masks + slot tables instead of the compacted observation tables (MCBA_LIN_COMPACT=0, form 2:
  bit-identical to form 3) and the table form behind k_tmat (MCBA_FUSED=0: 1e-11 of the default); all against the host build, with
  one view per workgroup and with one workgroup for all views.  Each process also solves with 2 and 5 evaluations: under
  MCBA_FUSED=0 k_cost evaluates every trial step on the main stream, under MCBA_SPEC_ACCEPT=0 on the side stream beside
  k_linearize; the reported cost against the oracle at the returned point."""
  w = worst
  shapes = [s for s in pr.SHAPES if s[0] == unit]
  assert len(shapes) == 6
  check_switch_forced(w, run_switches(tmp_path, "edges", unit), shapes, "edges")


def test_switch_forced_forms_on_the_big_board(tmp_path, worst):
  """... and on the three rigs with the 816-point board, where form 2 walks two segments (an empty first or second one among them) and
  agrees with form 3 to round-off."""
  w = worst
  check_switch_forced(w, run_switches(tmp_path, "bigboard", "-"), pr.BIG_SHAPES, "bigboard")
