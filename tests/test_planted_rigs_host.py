"""CPU: the reference chain of tests/test_gpu_view_edges.py on the planted rigs (tests/planted_rigs.py), before any GPU is involved:
the host build of the product's device functions (tests/hostmath) against the oracle on all 42 view shapes plus the three rigs
with an 816-point board -- shapes neither had seen (rolling shutter with every distortion model, hand-eye with free intrinsics,
pinhole + fisheye under rolling shutter and hand-eye)."""
import numpy as np
import pytest

import planted_rigs as pr
from hostmath_lib import HostMath
from oracle import restate
from util import mirror, rel_col_error

RIGS = [("edges",) + s for s in pr.SHAPES] + [("bigboard",) + s for s in pr.BIG_SHAPES]


def make(kind, unit, motion, optk):
  return (pr.planted_rig if kind == "edges" else pr.planted_bigboard)(unit, motion, optk)


def oracle_differences(oc, x):
  """3-point differences of the oracle's residuals, columns grouped by the oracle's sparsity pattern."""
  from scipy.optimize._numdiff import approx_derivative, group_columns
  from scipy.sparse import csr_matrix
  S = csr_matrix(oc.sparsity_matrix)
  return csr_matrix(approx_derivative(oc.evaluate, x, method='3-point', sparsity=(S, group_columns(S)))), S


def test_placement_holds_on_every_shape():
  """every count on both cameras, at least two empty views, every segment pair of the big board on a view (asserted in the
  helper), and the rigs stay small"""
  for kind, unit, motion, optk in RIGS:
    rig, planted = make(kind, unit, motion, optk)
    assert all(len(v) > 0 for v in planted.values())
    assert 5000 < 2 * int(rig.valid.sum()) < 7000, (kind, unit, motion, optk)
    assert rig.optimize["cameras"] is optk and rig.cfg["motion"] == motion
  rig, planted = pr.planted_rig("mix14", "rolling", True)
  assert [c.model for c in rig.init.cameras] == ["standard", "fisheye"]


@pytest.mark.parametrize("kind,unit,motion,optk", RIGS, ids=[r[0] + "-" + pr.shape_id(r[1:]) for r in RIGS])
def test_host_build_against_the_oracle(kind, unit, motion, optk):
  rig, _ = make(kind, unit, motion, optk)
  c = mirror(rig)
  oc = restate.from_rig(rig)
  x0 = c.param_vec
  assert np.array_equal(x0, oc.param_vec)                                     # parameter packing, bitwise
  hm = HostMath(c)
  assert hm.n == x0.size and hm.m == 2 * int(rig.valid.sum())
  J = hm.jacobian(x0)
  J3, S = oracle_differences(oc, x0)
  assert J.shape == J3.shape and rel_col_error(J, J3) < 2e-7
  nz = abs(J) > 0
  assert nz.multiply(S != 0).nnz == nz.nnz                                    # inside the oracle's sparsity pattern
  r = hm.residuals(x0)
  assert np.abs(r - oc.evaluate(x0)).max() < 1e-9
  H, g, cost = hm.normal_equations(x0)
  Jd = J.toarray()
  JtJ, Jtr = Jd.T @ Jd, Jd.T @ r
  assert np.abs(H - JtJ).max() <= 1e-12 * np.abs(JtJ).max()
  assert np.abs(g - Jtr).max() <= 1e-12 * np.abs(Jtr).max()
  assert cost == pytest.approx(0.5 * r @ r, rel=1e-12)
