"""profiles/reduced_system_parity.txt: the rigs of tests/reduced_rigs.py -- shape of the reduced system, the forms the handle takes for it,
the CPU-side condition numbers of the references and the largest error / tolerance ratios tests/test_gpu_reduced_system.py observed.

  pytest -m gpu tests/test_gpu_reduced_system.py -o junit_family=xunit1 --junitxml=reduced_system.xml      (on the MI355X)
  python profiles/scripts/reduced_system_parity.py reduced_system.xml > profiles/reduced_system_parity.txt  (CPU)
"""
import os
import sys
import xml.etree.ElementTree as ET

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np                      # noqa: E402

import reduced_rigs as rr               # noqa: E402
from hostmath_lib import HostMath       # noqa: E402
from util import mirror                 # noqa: E402


def ratios(path):
  out = {}
  for tc in ET.parse(path).getroot().iter("testcase"):
    for p in tc.iter("property"):
      if p.get("name") == "max_ratio":
        out[tc.get("name")] = float(p.get("value"))
  return out


def main(path):
  got = ratios(path)
  print("Reduced-system parity: tests/test_gpu_reduced_system.py on an MI355X (gfx950), rigs of tests/reduced_rigs.py.")
  print("ratio = largest observed error / tolerance of a test case (tolerances: H, gradient, diagonal, scale 1e-12; step 1e-8 of max |ref|;")
  print("quadratic-form identities 1e-9; covariance 1e-8 on |dSigma_ij| / sqrt(Sigma_ii Sigma_jj)); all references from the host build's H.")
  print()
  print("STEP ROUTE (test_step): ncol = ns + 1, ntile = ceil(ncol / 16), K = DF F; `bound` = cond(D H D + reg I) 2^-52 n at x0 (limit 1e-10)")
  print(f"{'rig':<20}{'C x B model':<30}{'ns':>5}{'DF':>4}{'F':>4}{'K':>5}{'ncol':>6}{'ntile':>6}{'ksplit':>7}  {'SYRK form':<20}{'Cholesky':<9}"
        f"{'reg (bound)':<34}{'ratio mfma':>11}{'ratio fma':>11}")
  cov_rows = []
  for name in rr.NAMES:
    rig = rr.reduced_rig(name)
    t = rig.target
    ns, DF, F, K = rig.shape
    C, B, models, camera_poses = rig.composition
    comp = f"{C} x {B} {'fixed' if models is None else models[0]}{'' if camera_poses or t.motion == 'hand_eye' else ' (poses held)'}"
    c = mirror(rig)
    H = HostMath(c).normal_equations(c.param_vec)[0]
    if t.step:
      regs = "  ".join(f"{reg:g} ({bound:.1e})" for reg, bound in rr.step_regs(H))
      print(f"{name:<20}{comp:<30}{ns:>5}{DF:>4}{F:>4}{K:>5}{ns + 1:>6}{rr.ntile(ns):>6}{rr.ksplit(ns, K):>7}  {rr.syrk_form(ns, K):<20}"
            f"{rr.cholesky_form(ns):<9}{regs:<34}{got[f'test_step[{name}-1]']:>11.2e}{got[f'test_step[{name}-0]']:>11.2e}")
    if t.cov:
      diag = np.diag(H)
      hold = rr.covariance_hold(rig, c, H)
      cond, pivot2, free = rr.covariance_conditions(H, hold)
      e = diag.size - 1 if rig.optimize["cameras"] else ns - 1       # the last shared parameter: x = [camera poses | board poses | motion | cameras]
      last = "held" if hold[e] else ("unobs" if diag[e] == 0 else "free")
      cov_rows.append(f"{name:<20}{comp:<30}{ns:>5}{DF:>4}{F:>4}{(ns + 15) // 16:>7}{str(t.cross):>7}{free:>6}{int(hold.sum()):>6}"
                      f"{int((diag == 0).sum()):>7}{last:>6}{cond:>10.1e}{pivot2:>10.1e}{got[f'test_covariance[{name}]']:>10.2e}")
  print()
  print("FORCED FORMS (test_forced_forms): every forced form against the host build and within 1e-12 of max |gn| of the handle's own choice")
  print(f"{'switch':<18}{'ratio':>10}  rigs")
  import test_gpu_reduced_system as tg
  for switch, names in tg.FORCED:
    if switch.startswith("MCBA_KSPLIT"):
      what = ", ".join(f"{n} (chosen {rr.ksplit(*rr.reduced_rig(n).shape[::3])})" for n in names)
    else:
      what = ", ".join(f"{n} (ntile {rr.ntile(rr.BY_NAME[n].ns)})" for n in names)
    print(f"{switch:<18}{got[f'test_forced_forms[{switch}]']:>10.2e}  {what}")
  print()
  print("COVARIANCE ROUTE (test_covariance): tiles of ns, nsp = 16 ceil(ns / 16); cond and the smallest squared Cholesky pivot of the scaled")
  print("free Hessian at x0 (limits 1e6 and 1e-8); `unobs` = parameters with diag(H) = 0 (std NaN), `held` = gauge + distortion coefficients,")
  print("`last` = the last shared parameter, the last column of the last tile (free where the last coefficient of every camera can stay free)")
  print(f"{'rig':<20}{'C x B model':<30}{'ns':>5}{'DF':>4}{'F':>4}{'nsp/16':>7}{'cross':>7}{'free':>6}{'held':>6}{'unobs':>7}{'last':>6}{'cond':>10}{'pivot^2':>10}{'ratio':>10}")
  print("\n".join(cov_rows))
  t = rr.BY_NAME[rr.REFUSED]
  print(f"{rr.REFUSED:<20}{'':<30}{t.ns:>5}   refused: \"at most 1023\" (test_covariance_refuses_the_rig_beyond_its_limit)")


if __name__ == "__main__":
  main(sys.argv[1])
