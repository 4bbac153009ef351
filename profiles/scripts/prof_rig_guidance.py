"""mcba_rig_view_information (multical_amd/guidance.py) at the 8 cameras of cfg3 (2000 x 1500) and at its first two, their
first board, a random joint factor of all stored camera and pose blocks but the first pose (in the units of the parameters: the cost
does not depend on its values): r = 8 x 15 - 6 = 114 and 2 x 15 - 6 = 24.

    candidates      guidance.rig_candidate_poses: 350 a camera (7 x 5 centres x 2 distances x 5 tilts), every one a (view, camera)
                    slot for every camera of the group; focus: 16 x 12 pixels of camera 0 at the candidates' median distance

Prints the four timing slots of the call (mcba_debug_rig_view_information_ms: uploads | the kernels and the scoring rounds with
their transfers, by HIP events | downloads | whole call; medians of 5 calls after 2 warm-up calls) with n = 0 picks (one scoring round)
and n = 3; with --host the g++ build of the same header on one core over the same call; with --trace one warm call and one traced call
of the 8-camera set for a kernel trace (rocprofv3 --kernel-trace --stats -- python profiles/scripts/prof_rig_guidance.py --trace).

    python profiles/scripts/prof_rig_guidance.py --device [--out FILE]    # needs the GPU
    python profiles/scripts/prof_rig_guidance.py --host [--out FILE]      # host build, no GPU
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from multical_amd import guidance, synthetic, uncertainty   # noqa: E402

SLOTS = ("upload", "kernel", "download", "call")
lines = []


def say(text):
  print(text, flush=True)
  lines.append(text)


def problem(n_cameras):
  rig = synthetic.make_rig("cfg3")
  model = uncertainty.RigModel(rig.truth.cameras[:n_cameras], np.asarray(rig.truth.camera_poses)[:n_cameras])
  pts = np.asarray(rig.board_points[0], dtype=np.float64)
  rng = np.random.default_rng(0)
  sizes = [5 + model.n_dist[c] + 6 for c in range(n_cameras)]
  p = sum(sizes)
  F = rng.normal(size=(p, p - n_cameras - 6)) * 3e-4
  factors, at = [], 0
  for c in range(n_cameras):
    Fc = F[at:at + sizes[c]].copy()
    Fc[:4] *= 1e3
    Fc[4] = 0.0
    if c == 0:
      Fc[-6:] = 0.0
    factors.append(guidance.rig_device_factor(model, c, Fc))
    at += sizes[c]
  Z, _ = guidance.rig_candidate_poses(model.cameras, model.poses, pts)
  views = [guidance.RigView(0, z) for z in Z]
  centre = 0.5 * (pts.min(axis=0) + pts.max(axis=0))
  at0 = (model.poses[0][None] @ Z)[:, :3, :3] @ centre + (model.poses[0][None] @ Z)[:, :3, 3]
  focus = guidance.RigFocus(0, list(range(n_cameras)), uncertainty.grid_of(model.cameras[0].image_size, (16, 12)),
                            float(np.median(np.linalg.norm(at0, axis=1))))
  return model, factors, pts, views, focus


def call(model, factors, pts, views, focus, n):
  return guidance.rig_view_information(model.cameras, model.poses, factors, [pts], views, focus, n=n, with_A=False)


def device():
  for n_cameras in (8, 2):
    model, factors, pts, views, focus = problem(n_cameras)
    for n in (0, 3):
      rows = []
      for i in range(7):
        r = call(model, factors, pts, views, focus, n)
        ms, slots = guidance.last_rig_call_ms()
        if i >= 2:
          rows.append([ms[k] for k in SLOTS])
      ms = np.median(np.array(rows), axis=0)
      say(f"cfg3, {n_cameras} cameras: {len(views)} candidates of {len(pts)} corners, {slots} slots, r = {r.r}, n = {n}: "
          + ", ".join(f"{k} {v:.3f} ms" for k, v in zip(SLOTS, ms))
          + f"; {int((r.status == guidance.OK).sum())} OK, {int(r.n_visible.sum())} visible corners, mean cameras per OK view "
          f"{float(r.n_cameras[r.status == guidance.OK].mean()):.2f}, focus RMS {r.focus_before:.4f}"
          + (f" -> {r.pick_focus_rms[-1]:.4f} px" if n else " px"))


def trace():
  model, factors, pts, views, focus = problem(8)
  call(model, factors, pts, views, focus, 3)
  call(model, factors, pts, views, focus, 3)


def host():
  import rigview_host_lib as rl
  for n_cameras in (8, 2):
    model, factors, pts, views, focus = problem(n_cameras)
    rl.lib()
    t = time.perf_counter()
    r = rl.on_host(call, model, factors, pts, views, focus, 3)
    dt = time.perf_counter() - t
    say(f"host build, one core, cfg3, {n_cameras} cameras: {1e3 * dt:.0f} ms for {len(views)} candidates of {len(pts)} corners, r = {r.r}, "
        f"n = 3 (marshalling included)")


if __name__ == "__main__":
  if "--device" in sys.argv:
    device()
  if "--trace" in sys.argv:
    trace()
  if "--host" in sys.argv:
    host()
  if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "a") as f:
      f.write("\n".join(lines) + "\n")
