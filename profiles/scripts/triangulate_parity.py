"""The figures behind tests/test_triangulate_host.py on the five fixture shapes, seeds 1 .. 5: the g++ build of
csrc/mcba_triangulate.h against the numpy restatement with a central-difference Jacobian (tests/triangulate_reference.py).  No GPU.

    python profiles/scripts/triangulate_parity.py > profiles/triangulate_parity.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import triangulate_host_lib as th    # noqa: E402
import triangulate_reference as tr   # noqa: E402
from multical_amd import triangulate   # noqa: E402


def main():
  print("host build of csrc/mcba_triangulate.h against tests/triangulate_reference.py (central differences, step %g m)" % tr.FD_STEP)
  print("whitened = in pixels through H = L L^T of the restatement; spread = distance between the restatement's optima from two starts")
  print(f"{'shape':18s} seed  points  OK  max lin.  |L^-1 g| returned   restatement's own   spread two starts   distance to its optimum   cond(H)")
  for (C, F, M, rolling), label in zip(th.SHAPES, th.SHAPE_IDS):
    for seed in range(1, 6):
      rig = th.make_rig(C, F, M, rolling, seed=seed)
      got = th.run(rig)
      ok = (got.status == triangulate.OK).ravel()
      n = rig.valid.sum(axis=0).ravel()
      caps = [k for k in range(1, 21) if (th.run(rig, max_iterations=k).status.ravel()[n >= 2] == triangulate.OK).all()]
      prob = th.reference_problem(rig)
      X = got.points.reshape(-1, 3)
      H, g, _, _ = prob.normal_equations(np.where(ok[:, None], X, 0.0))
      start, _ = prob.linear_start()
      a = prob.refine(start)
      b = prob.refine(start + np.random.default_rng(5).normal(0.0, 1e-3, start.shape))
      Ha, ga, _, _ = prob.normal_equations(np.where(ok[:, None], a, 0.0))
      print(f"{label:18s} {seed:4d} {int((n >= 2).sum()):7d} {int(ok.sum()):4d} {caps[0] if caps else -1:8d} "
            f"{tr.whitened_gradient(H[ok], g[ok]).max():18.2e} {tr.whitened_gradient(Ha[ok], ga[ok]).max():20.2e} "
            f"{tr.whitened_norm(H[ok], (a - b)[ok]).max():19.2e} {tr.whitened_norm(H[ok], (X - a)[ok]).max():25.2e} "
            f"{np.linalg.cond(H[ok]).max():9.1e}")


if __name__ == "__main__":
  main()
