"""mcba_hand_eye (tables.hand_eye_batch's device call) at the camera-pair problem lists of cfg5 (6 x 400 x 5) and cfg5_40
(6 x 40 x 5): every (master camera, slave camera, master board, slave board) combination with 3 common frames over the rig's truth
chain perturbed by its pose noise.  Prints the device call's four phase times (preparation | uploads | kernel | downloads; medians
of 5 calls after 2 warm-up calls) and the problem count; the time of the g++ build of the same header on one core (tests/handeye_host) and of the numpy restatement (tests/handeye_reference.py).

    python profiles/scripts/prof_hand_eye.py --device      # needs the GPU
    python profiles/scripts/prof_hand_eye.py --host        # host build + restatement, no GPU
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from multical_amd import synthetic, tables, _lib   # noqa: E402


def breakdown():
  ms, n = _lib.call_ms("hand_eye", range(4))
  return np.array(list(ms.values())), n


def main(device, host):
  import handeye_host_lib as hh
  import handeye_reference as R
  for name in ("cfg5", "cfg5_40"):
    poses, valid, _, (C_, F, B) = hh.camera_board_chain(synthetic.make_rig(name), noise_seed=7)
    ia, ib, _ = hh.camera_pair_problems(valid, C_, B)
    args = (poses, valid, poses, valid, ia, ib)
    host_out = hh.hand_eye_batch(*args, invert=True)
    n = host_out[2]
    print(f"{name}: table {C_ * B} rows x {F} frames ({int(valid.sum())} poses), {len(ia)} problems of {n.min()} .. {n.max()} pairs "
          f"(median {int(np.median(n))}), status {np.bincount(host_out[3], minlength=3).tolist()} (ok, too few, degenerate)")
    if device:
      call = lambda: tables.hand_eye_batch(*args, invert=True)
      for _ in range(2):
        out = call()
      wall, parts = [], []
      for _ in range(5):
        t0 = time.perf_counter()
        out = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        parts.append(breakdown())
      count = parts[-1][1]
      parts = np.median(np.array([p[0] for p in parts]), axis=0)
      print(f"  device call from Python            wall {np.median(wall):9.3f} ms; {count} problems launched; |X - X_host| "
            f"{np.abs(out[0] - host_out[0]).max():.1e}")
      print(f"    inside the library: preparation {parts[0]:9.3f} ms | uploads {parts[1]:9.3f} ms | kernel {parts[2]:9.3f} ms | "
            f"downloads {parts[3]:9.3f} ms")
    if host:
      times = []
      for _ in range(5):
        t0 = time.perf_counter()
        hh.hand_eye_batch(*args, invert=True)
        times.append(time.perf_counter() - t0)
      print(f"  host build of csrc/mcba_handeye.h (g++ -O2, one core) {np.median(times) * 1e3:9.3f} ms for the list")
      t0 = time.perf_counter()
      ref = R.batch(*args, invert=True)
      t_ref = time.perf_counter() - t0
      print(f"  numpy restatement (np.linalg.svd of K, lstsq) {t_ref * 1e3:9.1f} ms for the list; |X - X_host| "
            f"{np.abs(ref[0] - host_out[0]).max():.1e}")


if __name__ == "__main__":
  main("--device" in sys.argv, "--host" in sys.argv)
