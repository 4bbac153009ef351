"""mcba_triangulate (multical_amd/triangulate.py) at the board corners of the two largest configurations: every (frame, board, corner)
of the rig's own point table through Calibration.triangulate at the truth parameters,

    cfg3    8 cameras x  500 frames x 2 boards, rolling shutter   (M = 2 x 324 slots a frame)
    cfg4   16 cameras x 1000 frames x 5 boards, static            (M = 5 x  81 slots a frame)

Prints the four timing slots of the call (mcba_debug_triangulate_ms: uploads, HIP-event kernel time, downloads, whole call; medians
of 5 calls after 2 warm-up calls), the points that came back and their reconstruction error; with --host the g++ build of the same
header on one core and the numpy restatement of the tests, each on the first frames of the same table and per point.

    python profiles/scripts/prof_triangulate.py --device                 # needs the GPU
    python profiles/scripts/prof_triangulate.py --host                   # host build + restatement, no GPU
    python profiles/scripts/prof_triangulate.py --host --frames 20       # rehearsal: the first 20 frames of each rig
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from multical_amd import calibration, synthetic, triangulate   # noqa: E402

HOST_FRAMES, RESTATEMENT_FRAMES = 20, 2


def option(name, default):
  return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def table_of(calib, frames=None):
  """(cameras, views, views_end, points [C,F,M,2], mask [C,F,M]) of the calibration's own table, the first `frames` frames"""
  C, F, B, P = calib.point_table.valid.shape
  F = F if frames is None else min(F, frames)
  start, end = calib._rig_poses()
  views = triangulate.rig_views(calib.camera_poses.poses, start[:F])
  views_end = None if end is None else triangulate.rig_views(calib.camera_poses.poses, end[:F])
  points = np.ascontiguousarray(np.asarray(calib.point_table.points)[:, :F].reshape(C, F, B * P, 2))
  mask = np.ascontiguousarray(np.asarray(calib.inliers)[:, :F].reshape(C, F, B * P))
  return list(calib.cameras), views, views_end, points, mask


def main():
  frames = option("--frames", None)
  frames = None if frames is None else int(frames)
  for name in ("cfg3", "cfg4"):
    t0 = time.perf_counter()
    rig = synthetic.make_rig(name, frames=frames)
    calib = calibration.from_rig(rig, "truth")
    C, F, B, P = calib.point_table.valid.shape
    seen = calib.inliers.sum(axis=0)
    print(f"{name}: {C} cameras x {F} frames x {B} boards x {P} slots = {F * B * P} points a call, {int((seen >= 2).sum())} seen by >= 2 cameras, "
          f"{int(calib.inliers.sum())} observations ({rig.cfg['motion']}; rig synthesised in {time.perf_counter() - t0:.1f} s)")
    if "--device" in sys.argv:
      rows = []
      for i in range(7):
        t = calib.triangulate()
        ms, count = triangulate.last_call_ms()
        if i >= 2:
          rows.append([ms["upload"], ms["kernel"], ms["download"], ms["call"]])
      up, kernel, down, call = np.median(np.array(rows), axis=0)
      print(f"  device   uploads {up:8.3f} ms | kernel {kernel:8.3f} ms | downloads {down:8.3f} ms | whole call {call:8.3f} ms   "
            f"({count} points launched, {1e6 * kernel / max(int((seen >= 2).sum()), 1):.3f} ns of kernel per triangulated point)")
      r = calib.reconstruction_error()
      q = r.overall.quantiles
      print(f"           statuses {np.bincount(t.status.ravel(), minlength=5).tolist()} (OK, TOO_FEW, DEGENERATE, NOT_CONVERGED, BEHIND); reconstruction "
            f"RMS {1e3 * r.overall.rms:.3f} mm, median {1e3 * q[2]:.3f} mm, max {1e3 * q[4]:.3f} mm over {r.overall.n} corners")
    if "--host" in sys.argv:
      import triangulate_host_lib as th
      import triangulate_reference as tr
      cams, views, views_end, points, mask = table_of(calib, HOST_FRAMES)
      th.lib()
      t0 = time.perf_counter()
      got = th.on_host(triangulate.triangulate, cams, views, points, mask, views_end=views_end)
      dt = time.perf_counter() - t0
      n = int((got.status == triangulate.OK).sum())
      print(f"  host build of csrc/mcba_triangulate.h (g++ -O2, one core), first {views.shape[1]} frames: {dt * 1e3:9.1f} ms, {n} points "
            f"triangulated = {1e6 * dt / max(n, 1):8.2f} us a point; x {F / views.shape[1]:.0f} = {dt * F / views.shape[1]:7.2f} s a call")
      cams, views, views_end, points, mask = table_of(calib, RESTATEMENT_FRAMES)
      t0 = time.perf_counter()
      prob = tr.Problem(cams, views, points, mask, views_end=views_end)
      start, solvable = prob.linear_start()
      prob.refine(start)
      dt = time.perf_counter() - t0
      print(f"  numpy restatement (tests/triangulate_reference.py, all points of a call at once), first {views.shape[1]} frames: {dt * 1e3:9.1f} ms, "
            f"{int(solvable.sum())} points = {1e6 * dt / max(int(solvable.sum()), 1):8.2f} us a point")
    if "--device" not in sys.argv:
      print("  device: **unmeasured** in this run")


if __name__ == "__main__":
  main()
