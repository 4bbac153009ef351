"""mcba_rig_poses (multical_amd/localize.py) on the tables of the two largest configurations, every frame of the rig's own point table
localised with cameras, camera poses, boards and board poses at the truth,

    cfg3    8 cameras x  500 frames x 2 boards, rolling shutter   (12 unknowns a frame)
    cfg4   16 cameras x 1000 frames x 5 boards, static            ( 6 unknowns a frame)

each without `init` (start from the frame's own views: k_view_pose + candidate scoring) and with it (the perturbed poses the
synthetic rig hands the bundle adjustment).  Prints the five timing slots of the call (mcba_debug_rig_poses_ms: uploads, start kernel
and refinement kernel by HIP events, downloads, whole call; medians of 5 calls after 2 warm-up calls); beside them bundle_adjust(
solver="native") with only `motion` enabled on the same table from the same start (wall time of the call on a cached handle), and with
--host the g++ build of the same header on one core over the same table (every frame: measured, not extrapolated).  Everything printed also goes to
profiles/rig_pose_timing.txt.

    python profiles/scripts/prof_rig_pose.py --device                 # needs the GPU
    python profiles/scripts/prof_rig_pose.py --host                   # host build, no GPU
    python profiles/scripts/prof_rig_pose.py --host --frames 20       # rehearsal: the first 20 frames of each rig
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from multical_amd import calibration, localize, synthetic   # noqa: E402

_lines = []


def say(line):
  print(line, flush=True)
  _lines.append(line)


def option(name, default):
  return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def timed(fn):
  rows = []
  for i in range(7):
    r = fn()
    ms, count = localize.last_call_ms()
    if i >= 2:
      rows.append([ms["upload"], ms["start_kernel"], ms["kernel"], ms["download"], ms["call"]])
  return r, np.median(np.array(rows), axis=0), count


def first_frames(calib, F):
  from multical_amd.structs import Table
  table = Table.create(points=np.ascontiguousarray(np.asarray(calib.point_table.points)[:, :F]),
                       valid=np.ascontiguousarray(np.asarray(calib.point_table.valid)[:, :F]))
  start, end = calib._rig_poses()
  return table, (start[:F], None if end is None else end[:F])


def main():
  frames = option("--frames", None)
  frames = None if frames is None else int(frames)
  for name in ("cfg3", "cfg4"):
    t0 = time.perf_counter()
    rig = synthetic.make_rig(name, frames=frames)
    truth = calibration.from_rig(rig, "truth")
    calib = truth.copy(motion=calibration.from_rig(rig, "init").motion)      # shared blocks at the truth, frames at the perturbed start
    C, F, B, P = calib.point_table.valid.shape
    per_frame = np.moveaxis(np.asarray(calib.valid), 1, 0).reshape(F, -1).sum(axis=1)
    say(f"{name}: {C} cameras x {F} frames x {B} boards, {int(per_frame.sum())} observations, {int(np.median(per_frame))} a frame in the median, "
        f"{int(per_frame.max())} at most ({rig.cfg['motion']}; rig synthesised in {time.perf_counter() - t0:.1f} s)")
    if "--device" in sys.argv:
      for label, fn in (("no init", lambda: calib.localize(calib.point_table)), ("init   ", lambda: calib.localize(inliers_only=False))):
        r, (up, start, kernel, down, call), count = timed(fn)
        ok = r.status == localize.OK
        rms = np.sqrt(r.sse[ok].sum() / max(r.n_obs[ok].sum(), 1))
        say(f"  device, {label}: uploads {up:8.3f} ms | start kernel {start:8.3f} ms | refinement kernel {kernel:8.3f} ms | downloads {down:8.3f} ms | "
            f"whole call {call:8.3f} ms   ({count} frames launched, {1e3 * kernel / max(count, 1):.2f} us of refinement a frame)")
        say(f"           statuses {np.bincount(r.status, minlength=5).tolist()} (OK, TOO_FEW, DEGENERATE, NOT_CONVERGED, BEHIND); RMS {rms:.4f} px over the "
            f"OK frames, linearisations median {int(np.median(r.iters[ok]))} max {int(r.iters.max())}")
      try:
        only = calib.enable(cameras=False, boards=False, camera_poses=False, board_poses=False, motion=True)
        only.bundle_adjust(solver="native", max_iterations=1)              # (creates and caches the handle)
        t0 = time.perf_counter()
        out, res = only.bundle_adjust(solver="native", tolerance=1e-12, return_result=True)
        dt = time.perf_counter() - t0
        say(f"  bundle_adjust(solver='native'), only motion enabled, same table and start: {dt * 1e3:9.1f} ms wall, nfev {res.nfev}, RMS "
            f"{np.sqrt(2.0 * res.cost / max(int(per_frame.sum()), 1)):.4f} px (one trust region and one stopping rule for all frames)")
      except Exception as e:   # noqa: BLE001  (the comparison is optional: say so, go on)
        say(f"  bundle_adjust(solver='native') with only motion enabled did not run: {type(e).__name__}: {e}: **unmeasured**")
    else:
      say("  device: **unmeasured** in this run")
    if "--host" in sys.argv:
      import localize_host_lib as lh
      lh.lib()
      n = F
      table, (start, end) = first_frames(calib, n)
      for label, init in (("no init", None), ("init   ", (start, end) if end is not None else start)):
        t0 = time.perf_counter()
        with lh.host_backend():
          r = calib.localize(table, init=init)
        dt = time.perf_counter() - t0
        say(f"  host build of csrc/mcba_localize.h (g++ -O2, one core), {label}, all {n} frames: {dt * 1e3:9.1f} ms a call = {1e3 * dt / n:8.3f} ms a frame; "
            f"statuses {np.bincount(r.status, minlength=5).tolist()}")
  with open(os.path.join(ROOT, "profiles", "rig_pose_timing.txt"), "w") as fh:
    fh.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
  main()
