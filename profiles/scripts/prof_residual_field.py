"""mcba_residual_gram at a full-size BASELINE configuration (default grid 5 x 4, 5 folds, inliers only, 16 x 12 coverage maps): the
four timing slots of the call (mcba_debug_residual_gram_ms: projection pass, k_residual_gram and k_residual_gram_fold by HIP events,
the whole call by host clock) and the wall time from Python with the numpy algebra of Calibration.residual_field on top.  Medians of
10 calls after 2 warm-up calls.  The CPU side of profiles/residual_field_timing.txt (a scipy.sparse B^T B of the same table) comes
from `--cpu`, which needs no GPU.

    python profiles/scripts/prof_residual_field.py cfg3 | cfg4 [--cpu]
"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from multical_amd import synthetic, calibration, residual_field   # noqa: E402


def med(f, n=10, warm=2):
  for _ in range(warm):
    f()
  out = []
  for _ in range(n):
    t0 = time.perf_counter()
    r = f()
    out.append([(time.perf_counter() - t0) * 1e3] + list(r or []))
  return np.median(np.array(out), axis=0)


def sparse_gram(points, valid, sizes, nx, ny):
  """the host alternative: a scipy.sparse design matrix [rows, K + 2] per camera from the downloaded table, then B^T B"""
  from scipy.sparse import csr_matrix
  K = residual_field.n_control(nx, ny)
  out = []
  for c, (W, H) in enumerate(sizes):
    px = points[c][valid[c]]
    (ix, tx), (iy, ty) = residual_field.cell(px[:, 0], W, nx), residual_field.cell(px[:, 1], H, ny)
    wx, wy = residual_field.cubic_weights(tx), residual_field.cubic_weights(ty)
    n = px.shape[0]
    cols = ((iy[:, None, None] + np.arange(4)[None, :, None]) * (nx + 3) + ix[:, None, None] + np.arange(4)[None, None, :]).reshape(n, 16)
    vals = (wy[:, :, None] * wx[:, None, :]).reshape(n, 16)
    r = np.zeros((n, 2))                                     # (the residual columns: their values do not change the cost)
    data = np.hstack([vals, r + 1.0])
    cols = np.hstack([cols, np.full((n, 1), K), np.full((n, 1), K + 1)])
    A = csr_matrix((data.ravel(), cols.ravel(), np.arange(0, 18 * n + 1, 18)), shape=(n, K + 2))
    out.append((A.T @ A).toarray())
  return out


def main(cfg, cpu):
  rig = synthetic.make_rig(cfg)
  sizes = [tuple(int(v) for v in cam.image_size) for cam in rig.init.cameras]
  C, F, B, P = rig.valid.shape
  if cpu:
    w = med(lambda: sparse_gram(rig.points, rig.valid, sizes, 5, 4) and None, n=5, warm=1)[0]
    print(f"{cfg}: {C} x {F} x {B} x {P} slots {C * F * B * P}, valid {int(rig.valid.sum())}")
    print(f"  scipy.sparse design matrices + B^T B on the host (one fold, table already in memory)   wall {w:9.3f} ms")
    return
  from multical_amd.backend import Handle
  c = calibration.from_rig(rig)
  with Handle(c) as h:
    x = h.solve(c.param_vec, tolerance=1e-10, max_iterations=100, tr_solver="exact").x
    print(f"{cfg}: {C} x {F} x {B} x {P} slots {C * F * B * P}, residuals {h.n_residuals}, {h.device_info()}")

    def call():
      h.residual_gram(x, sizes)
      ms, _ = residual_field.last_call_ms()
      return [ms["project"], ms["gram"], ms["fold"], ms["call"]]
    w, project, gram, fold, whole = med(call)
    _, rows = residual_field.last_call_ms()
    print(f"  mcba_residual_gram 5 x 4, 5 folds: rows {rows}   projection pass {project * 1e3:8.1f} us   k_residual_gram {gram * 1e3:8.1f} us   "
          f"k_residual_gram_fold {fold * 1e3:8.1f} us   call {whole:8.3f} ms   wall from Python {w:8.3f} ms")
    g = h.residual_gram(x, sizes)
    t0 = time.perf_counter()
    sigma2 = float(g.gram[..., -2, -2].sum() + g.gram[..., -1, -1].sum()) / (2.0 * g.count.sum())   # (the raw residual variance)
    out = residual_field.analyse(g.gram, g.count, g.outside, g.coverage, sizes, 5, 4, sigma2)
    print(f"  numpy algebra on the blocks {(time.perf_counter() - t0) * 1e3:8.3f} ms; cv_gain {np.array2string(out.cv_gain, precision=3)} "
          f"z {np.array2string(out.z, precision=1)}")


if __name__ == "__main__":
  main(sys.argv[1], "--cpu" in sys.argv[2:])
