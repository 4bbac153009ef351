"""mcba_calibrate_intrinsics (tables.calibrate_intrinsics' device call) at two sizes: 8 cameras x ~50 views x 324 corners and
16 cameras x ~50 views x 81 corners (72 frames of one board, seen in 0.7 of them).  Prints the device call's four phase times
(plan + gather | uploads | kernels | downloads + scatter; medians of 5 calls after 2 warm-up calls), the time of the g++ build of
the same header on one core (tests/intrinsic_host) and of the numpy / scipy restatement (tests/intrinsic_reference.py, one camera,
scaled to the rig).

    python profiles/scripts/prof_intrinsics.py --device      # needs the GPU
    python profiles/scripts/prof_intrinsics.py --host        # host build + restatement, no GPU
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from multical_amd import synthetic, tables, _lib   # noqa: E402
from multical_amd.structs import struct   # noqa: E402

SIZES = [("8 x 50 x 324", dict(cameras=8, frames=72, boards=["aprilgrid_9x9"], motion="static", model="standard",
                               optimize_cameras=True, layout="stereo", seed=41)),
         ("16 x 50 x 81", dict(cameras=8, frames=72, boards=["charuco_10x10"], motion="static", model="standard",
                               optimize_cameras=True, layout="stereo", seed=42))]


def make(label, cfg):
  """The rig of a size; the 16-camera one is two 8-camera rigs side by side (a wider stereo bar would lose sight of the board)."""
  rig = synthetic.make_rig(cfg)
  if label.startswith("16"):
    other = synthetic.make_rig(dict(cfg, seed=cfg["seed"] + 1))
    rig.points, rig.valid = np.concatenate([rig.points, other.points]), np.concatenate([rig.valid, other.valid])
    rig.truth.cameras = rig.truth.cameras + other.truth.cameras
  return rig


def breakdown():
  ms, n = _lib.call_ms("calibrate_intrinsics", range(4))
  return np.array(list(ms.values())), n


def main(device, host):
  for label, cfg in SIZES:
    rig = make(label, cfg)
    table = struct(points=rig.points, valid=rig.valid)
    sizes = [c.image_size for c in rig.truth.cameras]
    views = (rig.valid.sum(axis=3) >= 4).sum(axis=(1, 2))
    print(f"{label}: {len(sizes)} cameras, views per camera {views.min()} .. {views.max()} (mean {views.mean():.1f}), "
          f"{rig.valid.shape[3]} corners a board, {int(rig.valid.sum())} corners, model standard (5 coefficients)")
    if device:
      call = lambda: tables.calibrate_intrinsics(table, rig.board_points, sizes)
      for _ in range(2):
        out = call()
      wall, parts = [], []
      for _ in range(5):
        t0 = time.perf_counter()
        out = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        parts.append(breakdown()[0])
      parts = np.median(np.array(parts), axis=0)
      print(f"  device call from Python           wall {np.median(wall):9.3f} ms; status {np.bincount(out.camera_status, minlength=5).tolist()} "
            f"(ok, too few views, degenerate, not converged, masked); LM passes {out.lm_iterations.min()} .. {out.lm_iterations.max()}; "
            f"error {out.error.min():.4f} .. {out.error.max():.4f} px")
      print(f"  inside the library: plan + gather {parts[0]:9.3f} ms | uploads {parts[1]:9.3f} ms | kernels {parts[2]:9.3f} ms | "
            f"downloads + scatter {parts[3]:9.3f} ms")
    if host:
      import intrinsic_host_lib as L
      import intrinsic_reference as R
      L.build()
      t0 = time.perf_counter()
      ref = L.calibrate_intrinsics(table, rig.board_points, sizes)
      t_host = time.perf_counter() - t0
      print(f"  host build of csrc/mcba_intrinsic.h (g++ -O2, one core) {t_host * 1e3:9.1f} ms for the rig; LM passes "
            f"{ref.lm_iterations.min()} .. {ref.lm_iterations.max()}; error {ref.error.min():.4f} .. {ref.error.max():.4f} px")
      rig.models = ["standard"] * len(sizes)
      slots, v = L.camera_views(rig, 0)
      prob = R.Problem(v, "standard")
      blk, poses = L.perturbed(L.truth_block(rig.truth.cameras[0]), L.truth_poses(rig, 0, slots))
      t0 = time.perf_counter()
      res = prob.solve(blk, poses)
      t_ref = time.perf_counter() - t0
      print(f"  numpy / scipy restatement, camera 0 ({len(slots)} views, {res.nfev} evaluations + polish) {t_ref:7.2f} s, "
            f"x {len(sizes)} cameras = {t_ref * len(sizes):7.1f} s; |K - K_host| {np.abs(res.block[:4] - ref.cameras[0, :4]).max():.2e} px")


if __name__ == "__main__":
  main("--device" in sys.argv, "--host" in sys.argv)
