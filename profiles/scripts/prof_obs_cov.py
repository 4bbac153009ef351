"""mcba_observation_covariance at a full-size BASELINE configuration: HIP-event time of the per-observation pass alone (k_obscov +
k_obscov_fold) and wall time of the whole call, with both per-slot outputs, with the studentised errors only and with none
(pred_cov = NULL, student = NULL), beside mcba_covariance on the same run.  Medians of 10 calls after 2 warm-up calls.

    python profiles/scripts/prof_obs_cov.py cfg3 | cfg4
"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from multical_amd import synthetic, gauge, calibration   # noqa: E402
from multical_amd.backend import Handle                  # noqa: E402


def med(f, n=10, warm=2):
  for _ in range(warm):
    f()
  wall, ev = [], []
  for _ in range(n):
    t0 = time.perf_counter()
    e = f()
    wall.append((time.perf_counter() - t0) * 1e3)
    ev.append(e)
  return float(np.median(wall)), (float(np.median(ev)) if ev[0] is not None else None)


def main(cfg):
  rig = synthetic.make_rig(cfg)
  c = calibration.from_rig(rig)
  hold = gauge.default_hold(c)
  with Handle(c) as h:
    x = h.solve(c.param_vec, tolerance=1e-12, max_iterations=200, tr_solver="exact").x
    C, F, B, P = h.shape
    print(f"{cfg}: {C} x {F} x {B} x {P} slots {C * F * B * P}, residuals {h.n_residuals}, {h.device_info()}")
    w, _ = med(lambda: h.covariance(x, hold=hold, frames=True, cross=False) and None)
    print(f"  mcba_covariance (no cross blocks)                wall {w:8.3f} ms")
    for label, kw in (("pred_cov + student", dict(cov=True, student=True)), ("student only (pred_cov = NULL)", dict(cov=False, student=True)),
                      ("no per-slot output", dict(cov=False, student=False))):
      def call():
        h.observation_covariance(x, hold=hold, **kw)
        return h.observation_covariance_ms()
      w, e = med(call)
      print(f"  mcba_observation_covariance, {label:32s} wall {w:8.3f} ms   per-observation pass (HIP events) {e * 1e3:8.1f} us")
    out = h.observation_covariance(x, hold=hold, cov=False, student=False)
    print(f"  trace {out.trace!r} (p_free = {h.n_residuals - out.dof}), max predicted std per camera {np.array2string(out.cam_max_std, precision=3)}")


if __name__ == "__main__":
  main(sys.argv[1])
