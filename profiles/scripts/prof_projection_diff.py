"""mcba_projection_diff (multical_amd/compare.py) at the 8 cameras of cfg3 and the 16 of cfg4 (2000 x 1500): calibration 0 is the truth,
calibration 1 the rig's initial guess.

    default call    16 x 12 map and 60 x 40 fit a camera, one call for all cameras: rotation at infinity, rigid at 2 m, transfer
    full map        2000 x 1500 pixels of camera 0 with the default fit; the same as a transfer from the next camera

Prints the five timing slots of the call (mcba_debug_projection_diff_ms: uploads, fit kernel and map kernel by HIP events, downloads,
whole call; medians of 5 calls after 2 warm-up calls), the linearisations of the fits (the fit kernel is a latency chain on as many
CUs as jobs fit) and the transfer share; with --host the g++ build of the same header on one core over the default call and over a
200 x 150 map of one camera (a full map on one core is not run: its time is the per-query time of that map times the pixels, marked
extrapolated).

    python profiles/scripts/prof_projection_diff.py --device [--out FILE]    # needs the GPU
    python profiles/scripts/prof_projection_diff.py --host                   # host build, no GPU
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from multical_amd import compare, synthetic, uncertainty   # noqa: E402

SLOTS = ("upload", "fit", "map", "download", "call")
lines = []


def say(text):
  print(text, flush=True)
  lines.append(text)


def rig_models(name):
  rig = synthetic.make_rig(name)
  return (uncertainty.RigModel(rig.truth.cameras, rig.truth.camera_poses), uncertainty.RigModel(rig.init.cameras, rig.init.camera_poses),
          rig.truth.cameras)


def jobs_of(cams, cameras, kind, grid):
  jobs = []
  for b in cameras:
    size = cams[b].image_size
    where = dict(grid=uncertainty.grid_of(size, grid))
    if kind == "transfer":
      jobs.append(compare.Job(b, (b + 1) % len(cams), 2.0, **where))
    else:
      distance, mode = (np.inf, compare.ROTATION) if kind == "rotation" else (2.0, compare.RIGID)
      jobs.append(compare.Job(b, None, distance, mode, fit_grid=uncertainty.grid_of(size, (60, 40)), **where))
  return jobs


def timed(rig0, rig1, jobs, repeats=5, warm=2):
  rows = []
  for i in range(warm + repeats):
    r = compare.run_jobs(rig0, rig1, jobs)
    ms, n = compare.last_call_ms()
    if i >= warm:
      rows.append([ms[k] for k in SLOTS])
  return np.median(np.array(rows), axis=0), n, r


def describe(ms):
  return ", ".join(f"{k} {v:.3f} ms" for k, v in zip(SLOTS, ms))


def device():
  for name in ("cfg3", "cfg4"):
    rig0, rig1, cams = rig_models(name)
    C = len(cams)
    for kind in ("rotation", "rigid", "transfer"):
      ms, n, r = timed(rig0, rig1, jobs_of(cams, range(C), kind, (16, 12)))
      its = r.fit_info[:, 1].astype(int)
      say(f"{name}, {C} cameras, default call ({kind}): {n} queries, {describe(ms)}; linearisations {its.min()} .. {its.max()}, "
          f"{int((r.status == compare.OK).sum())} OK, fit statuses {sorted(set(r.fit_info[:, 4].astype(int).tolist()))}")
    size = cams[0].image_size
    for kind in ("rotation", "rigid", "transfer"):
      ms, n, r = timed(rig0, rig1, jobs_of(cams, [0], kind, size), repeats=3, warm=1)
      say(f"{name}, camera 0 full map {size[0]} x {size[1]} ({kind}): {describe(ms)}; map {1e6 * ms[2] / n:.2f} ns a pixel, "
          f"{int((r.status == compare.OK).sum())} of {n} OK")


def host():
  import projdiff_host_lib as pl
  rig0, rig1, cams = rig_models("cfg3")
  cases = [(f"{len(cams)} cameras, default call", range(len(cams)), (16, 12)), ("camera 0, 200 x 150 map", [0], (200, 150))]
  for kind in ("rotation", "rigid", "transfer"):
    for label, cameras, grid in cases:
      jobs = jobs_of(cams, cameras, kind, grid)
      pl.on_host(compare.run_jobs, rig0, rig1, jobs)
      t = time.perf_counter()
      r = pl.on_host(compare.run_jobs, rig0, rig1, jobs)
      dt = time.perf_counter() - t
      say(f"host build, one core, cfg3 ({kind}): {label}: {1e3 * dt:.1f} ms for {len(r.status)} queries and {len(jobs)} jobs"
          + (f"; a 2000 x 1500 map at that rate {3e6 * dt / len(r.status):.1f} s (extrapolated, not run)" if len(jobs) == 1 else ""))


if __name__ == "__main__":
  if "--device" in sys.argv:
    device()
  if "--host" in sys.argv:
    host()
  if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "a") as f:
      f.write("\n".join(lines) + "\n")
