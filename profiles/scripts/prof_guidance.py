"""mcba_view_information (multical_amd/guidance.py) at the 8 cameras of cfg3 and the 16 of cfg4 (2000 x 1500), their first board, a
full-rank factor of every camera's intrinsics (random, in the units of the parameters: the cost does not depend on its values).

    default set     guidance.candidate_poses: 7 x 5 centres x 2 distances x 5 tilts = 350 candidates a camera, 16 x 12 focus grid
    large set       40 x 25 centres x 2 distances x 5 tilts = 10 000 candidates a camera

Prints the four timing slots of the call (mcba_debug_view_information_ms: uploads | k_view_schur and the scoring rounds with their
transfers, by HIP events | downloads | whole call; medians of 5 calls after 2 warm-up calls) with n = 0 picks (one scoring round: the
difference to n = 3 is three more rounds) and n = 3, the counted flops of k_view_schur -- 4 KI r for the two rows Kc W of a point
(KI = 18 padded) and 2 (r + 6)(r + 7) for their share of the upper Gram triangle -- and their share of the 78.6 TFLOP/s FP64 peak
taking the whole device slot of the n = 0 call as the kernel's time (an upper bound of its time, so a lower bound of its share);
with --host the g++ build of the same header on one core over the default set.

    python profiles/scripts/prof_guidance.py --device [--out FILE]    # needs the GPU
    python profiles/scripts/prof_guidance.py --host                   # host build, no GPU
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
PEAK = 78.6e12
lines = []


def say(text):
  print(text, flush=True)
  lines.append(text)


def problem(name, centres):
  rig = synthetic.make_rig(name)
  model = uncertainty.RigModel(rig.truth.cameras, rig.truth.camera_poses)
  pts = np.asarray(rig.board_points[0], dtype=np.float64)
  rng = np.random.default_rng(0)
  factors, views = [], []
  for c, cam in enumerate(model.cameras):
    p = 5 + model.n_dist[c]
    F = rng.normal(size=(p, p - 1)) * 3e-4
    F[:4] *= 1e3
    F[4] = 0.0
    factors.append((uncertainty.camera_map(model.n_dist[c], model.fix_aspect[c]) @ F, False))
    views += [guidance.View(c, 0, T) for T in guidance.candidate_poses(cam, pts, centres=centres)]
  foci = [guidance.Focus(c, np.inf, grid=uncertainty.grid_of(cam.image_size, (16, 12))) for c, cam in enumerate(model.cameras)]
  return model, factors, pts, views, foci


def timed(run, repeats=5, warm=2):
  rows = []
  for i in range(warm + repeats):
    r = run()
    ms, n = guidance.last_call_ms()
    if i >= warm:
      rows.append([ms[k] for k in SLOTS])
  return np.median(np.array(rows), axis=0), n, r


def describe(ms):
  return ", ".join(f"{k} {v:.3f} ms" for k, v in zip(SLOTS, ms))


def device():
  for name in ("cfg3", "cfg4"):
    for label, centres in (("default set", (7, 5)), ("large set", (40, 25))):
      model, factors, pts, views, foci = problem(name, centres)
      r_max = max(W.shape[1] for W, _ in factors)
      for n in (0, 3):
        ms, launched, r = timed(lambda: guidance.view_information(model.cameras, factors, [pts], views, foci, n=n, with_S=False))
        text = (f"{name}, {len(model.cameras)} cameras, {label}: {len(views)} candidates of {len(pts)} corners, r = {r_max}, n = {n}: "
                f"{describe(ms)}; {int((r.status == guidance.OK).sum())} OK, {int(r.n_visible.sum())} visible corners")
        if n == 0:
          flops = len(views) * len(pts) * (4.0 * 18 * r_max + 2.0 * (r_max + 6) * (r_max + 7))
          text += (f"; k_view_schur {flops / 1e9:.2f} GFLOP counted = {flops / (ms[1] * 1e-3) / 1e12:.2f} TFLOP/s = "
                   f"{flops / (ms[1] * 1e-3) / PEAK:.3f} of the FP64 peak (whole device slot)")
        say(text)


def host():
  import guidance_host_lib as gl
  for name in ("cfg3", "cfg4"):
    model, factors, pts, views, foci = problem(name, (7, 5))
    run = lambda: gl.on_host(guidance.view_information, model.cameras, factors, [pts], views, foci, n=3, with_S=False)   # noqa: E731
    run()
    t = time.perf_counter()
    run()
    dt = time.perf_counter() - t
    say(f"host build, one core, {name}, default set: {1e3 * dt:.1f} ms for {len(views)} candidates of {len(pts)} corners, n = 3 "
        f"(marshalling included); 10 000 candidates a camera at that rate {dt * 1e4 * len(model.cameras) / len(views):.1f} s "
        f"(extrapolated, not run)")


if __name__ == "__main__":
  if "--device" in sys.argv:
    device()
  if "--host" in sys.argv:
    host()
  if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "a") as f:
      f.write("\n".join(lines) + "\n")
