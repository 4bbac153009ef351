"""mcba_view_poses (tables.make_pose_table's device call) at a full-size BASELINE configuration: wall time of the call from
Python with the library's own breakdown (plan + gather of the active views | uploads | kernel | downloads + scatter), the views
that converged, the mean Levenberg-Marquardt linearisations per view, and the host restatement (tests/pnp_reference.py: numpy
Newton undistortion + scipy least_squares) per view on one core beside it.  Medians of 5 calls after 2 warm-up calls.

    python profiles/scripts/prof_pose_table.py cfg3 | cfg4            # 8 x 500 x 2 (<= 324 corners), 16 x 1000 x 5 (<= 81)
    python profiles/scripts/prof_pose_table.py cfg3 --kernel          # + k_view_pose under rocprofv3 --kernel-trace --stats
    python profiles/scripts/prof_pose_table.py cfg3 --calls-only      # (what the --kernel child runs)
"""
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from multical_amd import synthetic, tables, _lib   # noqa: E402


def breakdown():
  ms, n = _lib.call_ms("view_poses", range(4))
  return np.array(list(ms.values())), n


def main(cfg, calls_only=False, kernel=False):
  rig = synthetic.make_rig(cfg)
  cams, boards = rig.truth.cameras, rig.board_points
  call = lambda: tables.view_poses(rig.points, rig.valid, boards, cams)
  for _ in range(2):
    out = call()
  wall, parts = [], []
  for _ in range(5):
    t0 = time.perf_counter()
    out = call()
    wall.append((time.perf_counter() - t0) * 1e3)
    parts.append(breakdown()[0])
  if calls_only:
    return
  poses, sse, n_used, status, iters = out
  parts, n_active = np.median(np.array(parts), axis=0), breakdown()[1]
  C_, F, B, P = rig.valid.shape
  ok = status == tables.VIEW_OK
  err = np.sqrt(sse[ok] / n_used[ok])
  print(f"{cfg}: {C_} x {F} x {B} views {C_ * F * B}, <= {P} corners, {n_active} views launched ({n_active / (C_ * F * B):.2f} of the table), "
        f"{int(rig.valid.sum())} corners")
  print(f"  status: ok {int(ok.sum())}, too few {int((status == 1).sum())}, degenerate {int((status == 3).sum())}, "
        f"not converged in 50 {int((status == 4).sum())}; LM linearisations mean {iters[ok].mean():.2f} max {iters.max()}; "
        f"views above 1 px (point norm) {float((err > 1).mean()):.3f}")
  print(f"  call from Python                  wall {np.median(wall):8.3f} ms")
  print(f"  inside the library: plan + gather {parts[0]:8.3f} ms | uploads {parts[1]:8.3f} ms | kernel {parts[2]:8.3f} ms | "
        f"downloads + scatter {parts[3]:8.3f} ms   (upload of the gathered observation rows: "
        f"{n_active * P * 17 / 1e6:.1f} MB, {parts[1] / np.median(wall):.2f} of the call)")
  # the host restatement on one core: a sample of the launched views
  import pnp_reference as ref
  from pnp_host_lib import truth_chain
  chain = truth_chain(rig)
  views = np.argwhere(ok)[:: max(1, int(ok.sum()) // 24)][:24]
  t0 = time.perf_counter()
  for c, f, b in views:
    m = np.flatnonzero(rig.valid[c, f, b])
    ref.solve(cams[c], np.asarray(boards[b], dtype=np.float64)[m], rig.points[c, f, b][m], chain[c, f, b])
  per = (time.perf_counter() - t0) / len(views) * 1e3
  print(f"  host restatement (numpy Newton + scipy least_squares, started at the truth), one core: {per:.2f} ms a view over "
        f"{len(views)} views -> {per * n_active / 1e3:.1f} s for the table")
  if kernel:
    d = tempfile.mkdtemp(prefix="pose_table_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "pose", "--", sys.executable,
           os.path.abspath(__file__), cfg, "--calls-only"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    files = glob.glob(os.path.join(d, "**", "pose_kernel_stats.csv"), recursive=True)
    if r.returncode != 0 or not files:
      print(f"  rocprofv3 run failed (exit {r.returncode}): {r.stderr[-400:]}")
      return
    for row in csv.DictReader(open(files[0])):
      if "k_view_pose" in row["Name"]:
        print(f"  rocprofv3 --kernel-trace --stats: {row['Name'].split('(')[0][-40:]} calls {row['Calls']} avg "
              f"{float(row['AverageNs']) / 1e3:.1f} us min {float(row['MinNs']) / 1e3:.1f} max {float(row['MaxNs']) / 1e3:.1f}")


if __name__ == "__main__":
  main(sys.argv[1], calls_only="--calls-only" in sys.argv, kernel="--kernel" in sys.argv)
