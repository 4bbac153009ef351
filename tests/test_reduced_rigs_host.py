"""CPU: the rigs of tests/reduced_rigs.py before any GPU is involved -- every rig meets its size target (ns, DF, K from the lowered
problem) and the conditions under which the references of tests/test_gpu_reduced_system.py stay inside their tolerances on their
own, and the host build of the product's device functions (tests/hostmath) is pinned to the oracle on them exactly as
tests/test_planted_rigs_host.py pins it on the planted rigs."""
import functools

import numpy as np
import pytest

import reduced_rigs as rr
from hostmath_lib import HostMath
from oracle import restate
from test_planted_rigs_host import oracle_differences
from util import mirror, rel_col_error


@functools.lru_cache(maxsize=None)
def host(name):
  """(rig, mirror Calibration, HostMath, (H, g, cost) at x0)"""
  rig = rr.reduced_rig(name)
  c = mirror(rig)
  hm = HostMath(c)
  return rig, c, hm, hm.normal_equations(c.param_vec)


def test_the_targets_cover_every_edge():
  """the sets the rigs were chosen for, from the targets alone"""
  step = [rr.BY_NAME[n] for n in rr.STEP]
  ncols = {t.ns + 1 for t in step}
  assert min(ncols) == 13
  assert {16 * m + e for m in (2, 4, 8, 10, 11) for e in (-1, 0, 1)} | {129} <= ncols
  assert {8, 9, 10, 11} <= {rr.ntile(t.ns) for t in step} and {160, 161} <= ncols
  shapes = {(t.motion, t.frames[0]) for t in step}
  assert {("static", f) for f in (1, 2, 5, 6, 10, 11, 21, 22)} | {("rolling", f) for f in (1, 3, 5, 6, 11)} <= shapes
  assert any(t.motion == "hand_eye" and (t.ns + 1) % 16 == 0 for t in step)
  K3 = {rr.DF[t.motion] * t.frames[0] for t in step if t.ns >= 128}
  assert {6, 12, 18, 36} <= K3 and max(K3) >= 128
  chosen = {rr.ksplit(t.ns, rr.DF[t.motion] * t.frames[0]) for t in step}
  assert {1, 2, 4} <= chosen
  forms = {rr.syrk_form(t.ns, rr.DF[t.motion] * t.frames[0]) for t in step}
  assert forms == {"none", "k_schur_syrk<true>", "k_schur_syrk3"}
  cov = [rr.BY_NAME[n] for n in rr.COVARIANCE]
  widths = {t.ns for t in cov}
  assert {12} | {16 * m + e for m in (2, 3, 4, 5) for e in (-1, 0, 1)} <= widths
  assert {1, 2, 3, 4, 5} <= {(t.ns + 15) // 16 for t in cov}
  assert sum(1000 <= ns <= 1023 for ns in widths) == 1 and rr.BY_NAME[rr.REFUSED].ns >= 1024
  assert {rr.DF[t.motion] for t in cov} == {0, 6, 12} and {t.cross for t in cov} == {True, False}
  assert any(t.frames[0] == 1 for t in cov) and any(t.frames[0] > 1 for t in cov)
  assert 25 <= len(rr.NAMES) <= 30


@pytest.mark.parametrize("name", rr.NAMES)
def test_size_and_conditions(name):
  rig, c, hm, (H, g, cost) = host(name)
  t = rig.target
  ns, DF, F, K = rig.shape
  # the lowered problem: ns = n_params - n_motion, n_motion = DF F (hand-eye: no eliminated block, ns = n)
  assert hm.n == c.param_vec.size == ns + K and (ns, DF, K) == (t.ns, rr.DF[t.motion], rr.DF[t.motion] * F)
  assert rig.valid.any(axis=(0, 2, 3)).all()                                  # every frame has a view
  assert all(p.shape[0] == 81 for p in rig.board_points)
  diag = np.diag(H)
  if t.step:
    for reg, bound in rr.step_regs(H):
      Hs = rr.jacobi(H)[0] + reg * np.eye(hm.n)
      assert np.linalg.cond(Hs) * 2.0 ** -52 * hm.n <= rr.STEP_CONDITION, (reg, bound)
  if t.cov:
    hold = rr.covariance_hold(rig, c, H)
    cond, pivot2, free = rr.covariance_conditions(H, hold)
    assert cond <= rr.COV_CONDITION and pivot2 >= rr.COV_PIVOT2, (cond, pivot2)
    assert hm.m > free
    unobserved = np.flatnonzero(diag == 0)
    if t.ns == 32:
      # two cameras at the least (module docstring of reduced_rigs) and one entry each that no observation moves -- the skew, held at
      # zero by every camera model: 2 of 32.  Nothing else is unobserved.
      assert unobserved.size == 2
    else:
      assert unobserved.size <= rr.UNOBSERVED_SHARE * ns, (unobserved.size, ns)


@pytest.mark.parametrize("name", rr.NAMES)
def test_host_build_against_the_oracle(name):
  rig, c, hm, (H, g, cost) = host(name)
  oc = restate.from_rig(rig)
  x0 = c.param_vec
  assert np.array_equal(x0, oc.param_vec)                                     # parameter packing, bitwise
  assert hm.n == x0.size and hm.m == 2 * int(rig.valid.sum())
  J = hm.jacobian(x0)
  J3, S = oracle_differences(oc, x0)
  assert J.shape == J3.shape and rel_col_error(J, J3) < 2e-7
  nz = abs(J) > 0
  assert nz.multiply(S != 0).nnz == nz.nnz                                    # inside the oracle's sparsity pattern
  r = hm.residuals(x0)
  assert np.abs(r - oc.evaluate(x0)).max() < 1e-9
  Jd = J.toarray()
  JtJ, Jtr = Jd.T @ Jd, Jd.T @ r
  assert np.abs(H - JtJ).max() <= 1e-12 * np.abs(JtJ).max()
  assert np.abs(g - Jtr).max() <= 1e-12 * np.abs(Jtr).max()
  assert cost == pytest.approx(0.5 * r @ r, rel=1e-12)
