"""GPU (MI355X): the kernels between the per-view kernels and the Cholesky factorisation -- the Schur step k_schur_frame,
k_schur_syrk<true|false>, k_schur_syrk3, k_schur_reduce, k_schur_backsub and the covariance route k_cov_trinv, k_schur_syrk on L^-1,
k_cov_fold, k_cov_frame<DF> -- at every tile and split edge, through the production entry points, on the rigs of
tests/reduced_rigs.py: rigs chosen by the width ns of the reduced system, the size DF of a frame block and the number of frames.

  test_step          ncol = ns + 1 one below, on and one above a multiple of 16; ntile = 8 | 9 (k_schur_syrk | k_schur_syrk3), 9, 10, 11
                     and 12 (ntile % 3 = 0, 1, 2); ncol = 160 | 161 (LDS | panel Cholesky); K = DF F from 6 to 132 rows: below one
                     32-row batch, either side of the ksplit doublings, wavefronts of k_schur_syrk3 without rows; hand-eye (K = 0)
  test_forced_forms  the SYRK form the handle does not choose and splits it never chooses (without rows, an odd count, the unrolled
                     loop of k_schur_reduce), each forced with its switch in a process of its own
  test_covariance    ns = 12, one below / on / one above 32, 48, 64 and 80, ns = 1005 next to the documented limit and the
                     refusal beyond it; DF = 6, 12, 0; one frame and several; with and without the cross blocks

References: the host build of the product's device functions (tests/hostmath, pinned to the oracle on these rigs by
tests/test_reduced_rigs_host.py) and numpy / scipy on its H.  Tolerances are the project's own: 1e-12 of the maximum for H, gradient and
diagonal, 1e-12 for the scaling, 1e-8 of max |ref| for the step, 1e-9 for the two quadratic-form identities of the trust-region
driver, 1e-8 on |dSigma_ij| / sqrt(Sigma_ii Sigma_jj).  The dampings of a rig are the two smallest of reduced_rigs.REG_LADDER at
which cond(D H D + reg I) 2^-52 n <= 1e-10, so that the dense solve stays a hundred times inside the step's tolerance on its own.
Every test records the largest observed error / tolerance ratio (`max_ratio`)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import reduced_rigs as rr
from hostmath_lib import HostMath
from multical_amd.backend import Handle
from multical_amd._lib import McbaError
from multical_amd import gauge
from test_gpu_covariance import _compare
from test_gpu_view_edges import Worst, worst      # noqa: F401  (worst: the fixture that records max_ratio)
from util import mirror

pytestmark = pytest.mark.gpu


class Case(object):
  """One rig with its references; everything is computed once, shared by the tests and left unchanged."""

  def __init__(self, name):
    self.rig = rr.reduced_rig(name)
    self.c = mirror(self.rig)
    x0 = self.c.param_vec
    self.xs = [x0, x0 + 1e-3 * np.random.default_rng(5).normal(size=x0.size)]
    self.hm = HostMath(self.c)

  @functools.lru_cache(maxsize=None)
  def host(self, i):
    """(H, g, cost) of the host build"""
    return self.hm.normal_equations(self.xs[i])

  @functools.lru_cache(maxsize=None)
  def regs(self, i):
    return tuple(reg for reg, _ in rr.step_regs(self.host(i)[0]))


@functools.lru_cache(maxsize=None)
def case(name):
  return Case(name)


def check_linearisation(w, cs, i, grad, diag, H, tag):
  Hh, gh, _ = cs.host(i)
  w.close(H, Hh, 1e-12, (tag, "H"))
  w.close(grad, gh, 1e-12, (tag, "gradient"))
  w.close(diag, np.diag(Hh), 1e-12, (tag, "diagonal"), scale=np.abs(Hh).max())
  assert np.array_equal(H, H.T), tag


def check_step(w, cs, i, reg, gn, ghs, si, tag):
  """(D H D + reg I)^-1 D g from the Schur / Cholesky kernels against the dense solve on the host build's H"""
  Hh, gh, _ = cs.host(i)
  n = gh.size
  Hs, d = rr.jacobi(Hh)
  w.close(si, 1 / d, 1e-12, (tag, "scale_inv"))
  ref = np.linalg.solve(Hs + reg * np.eye(n), d * gh)
  w.close(gn, ref, 1e-8, (tag, "gn"))
  # the two identities the trust-region driver takes its quadratic forms from (see test_schur_cholesky_step)
  q01, q11 = ghs @ Hs @ gn, gn @ Hs @ gn
  w.check(abs((ghs @ ghs - reg * (ghs @ gn)) - q01), 1e-9 * abs(q01), (tag, "q01"))
  w.check(abs((ghs @ gn - reg * (gn @ gn)) - q11), 1e-9 * abs(q11), (tag, "q11"))


@pytest.mark.parametrize("mfma", [1, 0])
@pytest.mark.parametrize("name", rr.STEP)
def test_step(name, mfma, worst):
  """The default form of the handle (matrix pipe: k_schur_syrk<true> below nine tile columns, k_schur_syrk3 from nine) and the
  plain-FMA one (set_mfma(0): k_schur_syrk<false> for every size)."""
  cs, w = case(name), worst
  with Handle(cs.c) as h:
    h.set_mfma(mfma)
    for i, x in enumerate(cs.xs):
      cost, grad, diag = h.normal_equations(x)
      H = h.dense_hessian()
      check_linearisation(w, cs, i, grad, diag, H, (i,))
      for reg in cs.regs(i):
        gn, ghs, si = h.debug_gn_step(reg)
        check_step(w, cs, i, reg, gn, ghs, si, (i, reg))
        again = h.debug_gn_step(reg)
        assert all(np.array_equal(a, b) for a, b in zip((gn, ghs, si), again)), (i, reg)
      cost2, grad2, diag2 = h.normal_equations(x)
      assert cost2 == cost and np.array_equal(grad2, grad) and np.array_equal(diag2, diag) and np.array_equal(h.dense_hessian(), H)
      gn2 = h.debug_gn_step(cs.regs(i)[-1])[0]
      assert np.array_equal(gn2, gn), i


FORCED_CODE = r"""
import sys, json, numpy as np
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import reduced_rigs as rr
from util import mirror
from multical_amd.backend import Handle
from multical_amd import _lib
out_path, switch, regs = sys.argv[1], sys.argv[2], json.loads(sys.argv[3])
if switch != "default":
  _lib.set_switch(*switch.split("="))
out = {}
for name, by_point in regs.items():
  c = mirror(rr.reduced_rig(name))
  x0 = c.param_vec
  xs = [x0, x0 + 1e-3 * np.random.default_rng(5).normal(size=x0.size)]
  with Handle(c) as h:
    for i, x in enumerate(xs):
      cost, grad, diag = h.normal_equations(x)
      key = name + "/" + str(i)
      out[key + "/grad"], out[key + "/diag"], out[key + "/H"] = grad, diag, h.dense_hessian()
      for reg in by_point[i]:
        gn, ghs, si = h.debug_gn_step(reg)
        again = h.debug_gn_step(reg)
        assert all(np.array_equal(a, b) for a, b in zip((gn, ghs, si), again)), (key, reg)
        out[key + "/" + repr(reg) + "/gn"], out[key + "/" + repr(reg) + "/ghs"], out[key + "/" + repr(reg) + "/si"] = gn, ghs, si
np.savez(out_path, **out)
"""
BELOW_NINE = ["ns62-static-F10", "ns64-rolling-F5", "ns127-static-F22"]            # ntile 4, 5 and 8
FROM_NINE = [n for n in rr.STEP if rr.ntile(rr.BY_NAME[n].ns) >= 9]
SPLIT_RIGS = ["ns126-static-F21", "ns64-rolling-F5", "ns160-rolling-F11"]          # static, rolling, under k_schur_syrk3
FORCED = [("MCBA_SYRK3=1", BELOW_NINE), ("MCBA_SYRK3=0", FROM_NINE)] + [(f"MCBA_KSPLIT={k}", SPLIT_RIGS) for k in (1, 5, 16, 64)]


def run_forced(tmp_path, switch, names):
  """gradient / diagonal / H and the steps of the rigs under the handle's own choice and under the switch, one process each (a switch
  is read once per process); a process that fails ends the test before the next one starts"""
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  env = {k: v for k, v in os.environ.items() if not k.startswith("MCBA_")}
  regs = json.dumps({name: [list(case(name).regs(i)) for i in (0, 1)] for name in names})
  res = {}
  for sw in ("default", switch):
    path = str(tmp_path / (sw.replace("=", "_") + ".npz"))
    p = subprocess.run([sys.executable, "-c", FORCED_CODE, path, sw, regs], cwd=root, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (sw, p.returncode, p.stderr[-2000:])
    res[sw] = dict(np.load(path))
  return res["default"], res[switch]


def test_the_forced_rigs_are_what_they_are_meant_to_be():
  assert all(rr.ntile(rr.BY_NAME[n].ns) < 9 for n in BELOW_NINE) and len(FROM_NINE) == 7
  assert {rr.ntile(rr.BY_NAME[n].ns) % 3 for n in FROM_NINE} == {0, 1, 2}
  assert [rr.BY_NAME[n].motion for n in SPLIT_RIGS] == ["static", "rolling", "rolling"]
  assert [rr.ntile(rr.BY_NAME[n].ns) >= 9 for n in SPLIT_RIGS] == [False, False, True]
  assert all(n in rr.STEP for n in BELOW_NINE + SPLIT_RIGS)


@pytest.mark.parametrize("switch,names", FORCED, ids=[f[0] for f in FORCED])
def test_forced_forms(switch, names, tmp_path, worst):
  """MCBA_SYRK3=1: k_schur_syrk3 where most of its 48-column blocks are padding; MCBA_SYRK3=0: k_schur_syrk<true> at nine tile
  columns and more; MCBA_KSPLIT = 1, 5, 16, 64: one split for all rows, an odd number of splits, the four-way unrolled loop of
  k_schur_reduce, splits without rows (K = 60 .. 132 rows).  The same checks as test_step, and every forced form within 1e-12 of
  max |gn| of the form the handle chooses."""
  w = worst
  default, forced = run_forced(tmp_path, switch, names)
  assert set(default) == set(forced) and len(default) == (2 * 3 + 2 * 2 * 3) * len(names)
  for name in names:
    cs = case(name)
    for i in (0, 1):
      key = name + "/" + str(i)
      for tag, res in (("default", default), (switch, forced)):
        check_linearisation(w, cs, i, res[key + "/grad"], res[key + "/diag"], res[key + "/H"], (tag, key))
        for reg in cs.regs(i):
          k = key + "/" + repr(reg)
          check_step(w, cs, i, reg, res[k + "/gn"], res[k + "/ghs"], res[k + "/si"], (tag, k))
      for reg in cs.regs(i):
        k = key + "/" + repr(reg) + "/gn"
        w.close(forced[k], default[k], 1e-12, (switch, k, "against the default form"))


def covariance_hold(cs):
  return rr.covariance_hold(cs.rig, cs.c, cs.host(0)[0])


@pytest.mark.parametrize("name", rr.COVARIANCE)
def test_covariance(name, worst):
  """sigma2 (J^T J)^-1 of the free parameters at the perturbed point with sigma2 = 1 given (no solve: the covariance is defined at
  any x, and a given sigma2 keeps the cost out of the comparison) against scipy's dense Cholesky on the host build's H: shared,
  frame and cross blocks and std to 1e-8, rows and columns of held parameters exactly zero, std of unobserved parameters NaN.  The
  large rig: all of `shared` and 8 frames (all it has)."""
  cs, w = case(name), worst
  t = cs.rig.target
  x = cs.xs[1]
  Hh, _, cost = cs.host(1)
  hold = covariance_hold(cs)
  F = cs.rig.shape[2]
  frames = None if F <= 8 else np.unique(np.linspace(0, F - 1, 8).astype(int))
  ratios = []
  with Handle(cs.c) as h:
    cov = _compare(h, x, hold, Hh, cs.hm.m, 2.0 * cost, 1e-8, frames=frames, cross=t.cross, sigma2=1.0, ratios=ratios)
  for r in ratios:
    w.check(r, 1.0, "covariance")
  assert cov.sigma2 == 1.0 and cov.shared.shape == (t.ns, t.ns) and cov.frames.shape == (F,) + (rr.DF[t.motion],) * 2
  assert ("frame_shared" in cov) == t.cross
  if rr.DF[t.motion] > 0:
    assert ratios and np.isfinite(cov.frames).all()
  held_shared = hold[cov.shared_index]
  assert not cov.shared[held_shared].any() and not cov.shared[:, held_shared].any()


def test_covariance_refuses_the_rig_beyond_its_limit():
  cs = case(rr.REFUSED)
  assert cs.rig.shape[0] >= 1024
  with Handle(cs.c) as h:
    with pytest.raises(McbaError, match="at most 1023"):
      h.covariance(cs.xs[1], hold=gauge.default_hold(cs.c), sigma2=1.0)
    cost, grad, diag = h.normal_equations(cs.xs[1])      # the handle is still usable after the refusal
    assert np.isfinite(cost) and np.isfinite(grad).all()
