"""mcba_stereo_calibrate (multical_amd/stereo.py) on the tables of the two largest configurations: every camera pair of the rig from
its own common views, cameras at the truth, views started from the truth chain (Calibration.pairwise_extrinsics),

    cfg3    8 cameras x  500 frames x 2 boards, rolling shutter: 28 pairs (the pair model is static: it ignores the readout)
    cfg4   16 cameras x 1000 frames x 5 boards, static: 120 pairs, 97 of them with a common view

Prints the four timing slots of the call (mcba_debug_stereo_calibrate_ms: host preparation, uploads, kernel by HIP events, downloads;
medians of 5 calls after 2 warm-up calls), the wall time of the wrapper, the passes a pair and the share of the call that is upload;
beside them, with --host, the g++ build of the same header on one core over the same table, and, with --bundle N, a Python loop of
two-camera bundle_adjust(solver="native") calls over N pairs spread over the list (cameras and board poses held, camera poses and frames
free, the pair's common corners).  Everything printed also goes to --out (default profiles/stereo_timing.txt).

    python profiles/scripts/prof_stereo.py --device --bundle 6       # needs the GPU
    python profiles/scripts/prof_stereo.py --host                    # host build, no GPU
    python profiles/scripts/prof_stereo.py --host --frames 20        # rehearsal: 20 frames of each rig
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from multical_amd import calibration, stereo, synthetic   # noqa: E402

_lines = []


def say(line):
  print(line, flush=True)
  _lines.append(line)


def option(name, default):
  return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def pair_calibration(calib, i, j, min_common=4):
  """the two-camera calibration over the common corners of pair (i, j): cameras, boards and board poses held"""
  from multical_amd.parameters import ParamList
  from multical_amd.structs import Table
  valid = np.asarray(calib.valid)
  common = valid[i] & valid[j]
  common &= (common.sum(axis=-1) >= min_common)[..., None]
  points = np.asarray(calib.point_table.points)[[i, j]]
  names = [calib.cameras.names[i], calib.cameras.names[j]]
  poses = calib.camera_poses.copy(pose_table=Table.create(poses=np.asarray(calib.camera_poses.poses)[[i, j]], valid=np.ones(2, dtype=bool)),
                                  names=names)
  sub = calib.copy(cameras=ParamList([calib.cameras[i], calib.cameras[j]], names), camera_poses=poses,
                   point_table=Table.create(points=points, valid=np.stack([common, common])), inlier_mask=None)
  return sub.enable(cameras=False, boards=False, board_poses=False, camera_poses=True, motion=True)


def main():
  frames = option("--frames", None)
  frames = None if frames is None else int(frames)
  n_bundle = int(option("--bundle", 0))
  out_path = option("--out", os.path.join(ROOT, "profiles", "stereo_timing.txt"))
  for name in ("cfg3", "cfg4"):
    t0 = time.perf_counter()
    rig = synthetic.make_rig(name, frames=frames)
    calib = calibration.from_rig(rig, "truth")
    C, F, B, P = calib.point_table.valid.shape
    say(f"{name}: {C} cameras x {F} frames x {B} boards x {P} slots ({rig.cfg['motion']}; rig synthesised in {time.perf_counter() - t0:.1f} s)")
    if "--device" in sys.argv:
      rows, walls = [], []
      for k in range(7):
        t0 = time.perf_counter()
        r = calib.pairwise_extrinsics()
        wall = (time.perf_counter() - t0) * 1e3
        ms, launched = stereo.last_call_ms()
        if k >= 2:
          rows.append([ms["prepare"], ms["upload"], ms["kernel"], ms["download"]])
          walls.append(wall)
      prep, up, kernel, down = np.median(np.array(rows), axis=0)
      call = prep + up + kernel + down
      have = (r.status == stereo.OK) | (r.status == stereo.NOT_CONVERGED)
      say(f"  device: {len(r.pairs)} pairs, {launched} launched, views a pair {int(r.n_views.min())} .. {int(r.n_views.max())} (median "
          f"{int(np.median(r.n_views))}), points a pair median {int(np.median(r.n_points))}, {int(r.n_points.sum())} in all")
      say(f"  device: host preparation {prep:8.3f} ms | uploads {up:8.3f} ms | kernel (HIP events) {kernel:8.3f} ms | downloads {down:8.3f} ms | "
          f"call {call:8.3f} ms, upload share {100.0 * up / call:.0f} %; Calibration.pairwise_extrinsics wall {np.median(walls):8.3f} ms")
      say(f"  device: statuses {np.bincount(r.status, minlength=4).tolist()} (OK, TOO_FEW, DEGENERATE, NOT_CONVERGED); passes a pair median "
          f"{int(np.median(r.iterations[have]))} max {int(r.iterations.max())}; {1e3 * kernel / max(launched, 1):.1f} us of kernel a pair "
          f"(the pairs run side by side: the kernel ends with its slowest pair); rms median {np.nanmedian(r.rms):.4f} px")
      if n_bundle > 0:
        try:
          cold, warm, views = [], [], []
          picks = np.unique(np.linspace(0, len(r.pairs) - 1, n_bundle).astype(int))      # spread over the list of pairs
          for k in picks:
            sub = pair_calibration(calib, int(r.pairs[k, 0]), int(r.pairs[k, 1]))
            t0 = time.perf_counter()
            sub.bundle_adjust(solver="native", tolerance=1e-12)                # (creates its handle: what a loop over pairs pays)
            cold.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            sub.bundle_adjust(solver="native", tolerance=1e-12)                # (the same call again on the cached handle)
            warm.append(time.perf_counter() - t0)
            views.append(int(r.n_views[k]))
          say(f"  Python loop of two-camera bundle_adjust(solver='native') calls over {len(picks)} pairs spread over the list (views "
              f"{views}): {1e3 * np.mean(cold):9.1f} ms a pair with its handle, {1e3 * np.mean(warm):9.1f} ms on a cached handle "
              f"(x {len(r.pairs)} pairs = {1e3 * np.mean(cold) * len(r.pairs):9.1f} / {1e3 * np.mean(warm) * len(r.pairs):9.1f} ms, extrapolated)")
        except Exception as e:   # noqa: BLE001  (the comparison is optional: say so, go on)
          say(f"  Python loop of two-camera bundle_adjust calls did not run: {type(e).__name__}: {e}: **unmeasured**")
      else:
        say("  Python loop of two-camera bundle_adjust calls: **unmeasured** in this run")
    else:
      say("  device: **unmeasured** in this run")
    if "--host" in sys.argv:
      import stereo_host_lib as sh
      sh.lib()
      t0 = time.perf_counter()
      with sh.host_backend():
        r = calib.pairwise_extrinsics()
      dt = time.perf_counter() - t0
      say(f"  host build of csrc/mcba_stereo.h (g++ -O2, one core), all {len(r.pairs)} pairs of {F} frames: {dt * 1e3:9.1f} ms a call = "
          f"{1e3 * dt / max(len(r.pairs), 1):8.3f} ms a pair; statuses {np.bincount(r.status, minlength=4).tolist()}")
  with open(out_path, "w") as fh:
    fh.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
  main()
