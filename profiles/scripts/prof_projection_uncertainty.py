"""mcba_projection_uncertainty (multical_amd/uncertainty.py) at the 8 cameras of cfg3 (2000 x 1500, truth parameters):

    default grid    16 x 12 cells a camera, one call for the 8 cameras
    full map        2000 x 1500 pixels, one call per camera

each against the rig frame and as a transfer from the neighbouring camera at 2 m.  The covariance is a synthetic full-rank one
over the stored parameters of every job (the time depends on its rank only: r = 19 for the rig frame, 38 for a transfer with these
5-coefficient cameras).  Prints the four timing slots of the call (mcba_debug_projection_uncertainty_ms: uploads, HIP-event kernel
time, downloads, whole call; medians of 5 calls after 2 warm-up calls) and the achieved FP64 rate from the counted flops of the
column loop (103 r per query against the rig frame, 217 r for a transfer; the Newton inverse and the projections are
not counted); with --host the g++ build of the same header on one core over the default grids and over a 200 x 150 grid of one
camera (a full map on one core is not run: its time is the per-query time of that grid times the pixels, marked extrapolated).

    python profiles/scripts/prof_projection_uncertainty.py --device [--out FILE]    # needs the GPU
    python profiles/scripts/prof_projection_uncertainty.py --host                   # host build, no GPU
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from multical_amd import synthetic, uncertainty   # noqa: E402

FLOPS = {None: 103, "transfer": 217}
lines = []


def say(text):
  print(text, flush=True)
  lines.append(text)


def rig_model():
  rig = synthetic.make_rig("cfg3")
  cams = rig.truth.cameras
  return uncertainty.RigModel(cams, rig.truth.camera_poses), cams


def spd(p, seed):
  A = np.random.default_rng(seed).normal(size=(p, p))
  S = 1e-6 * (A @ A.T + 0.1 * np.eye(p))
  S[4, :] = 0.0
  S[:, 4] = 0.0
  return S


def jobs_of(model, cams, cameras, transfer, grid):
  jobs = []
  for b in cameras:
    a = (b + 1) % len(cams) if transfer else None
    S = spd(model.stored_count(b, a), b)
    if a is not None:
      k = model.stored_count(b, a) - (model.n_dist[a] + 1)
      S[k, :] = 0.0
      S[:, k] = 0.0
    jobs.append(uncertainty.Job(b, a, 2.0, S, grid=uncertainty.grid_of(cams[b].image_size, grid)))
  return jobs


def timed(model, jobs, repeats=5, warm=2):
  rows = []
  for i in range(warm + repeats):
    cov, std, status = uncertainty.run_jobs(model, jobs)
    ms, n = uncertainty.last_call_ms()
    if i >= warm:
      rows.append([ms[k] for k in ("upload", "kernel", "download", "call")])
  return np.median(np.array(rows), axis=0), n, status


def rank_of(model, job):
  sigma = np.where(job.loose[:, None] | job.loose[None, :], 0.0, job.sigma)
  return uncertainty.factor(sigma).shape[1]


def device():
  model, cams = rig_model()
  for transfer in (False, True):
    mode = "transfer from the next camera" if transfer else "rig frame"
    jobs = jobs_of(model, cams, range(len(cams)), transfer, (16, 12))
    r = rank_of(model, jobs[0])
    ms, n, status = timed(model, jobs)
    say(f"{mode}: 8 cameras x 16 x 12 grid, r = {r}: {n} queries, upload {ms[0]:.3f} ms, kernel {ms[1]:.3f} ms, download {ms[2]:.3f} ms, "
        f"call {ms[3]:.3f} ms; {int((status == uncertainty.OK).sum())} OK")
    per_camera = []
    for b in range(len(cams)):
      ms, n, status = timed(model, jobs_of(model, cams, [b], transfer, cams[b].image_size), repeats=3, warm=1)
      per_camera.append(ms)
      flops = FLOPS["transfer" if transfer else None] * r * n
      say(f"{mode}: camera {b} full map {cams[b].image_size[0]} x {cams[b].image_size[1]}: kernel {ms[1]:.2f} ms ({1e6 * ms[1] / n:.2f} ns a "
          f"pixel, {flops / ms[1] / 1e9:.2f} TFLOP/s FP64 counted), download {ms[2]:.1f} ms, call {ms[3]:.1f} ms; "
          f"{int((status == uncertainty.OK).sum())} of {n} OK")
    tot = np.sum(per_camera, axis=0)
    say(f"{mode}: 8 full maps (24 M pixels): kernels {tot[1]:.1f} ms, calls {tot[3]:.1f} ms")


def host():
  import uncertainty_host_lib as ul
  model, cams = rig_model()
  for transfer in (False, True):
    mode = "transfer from the next camera" if transfer else "rig frame"
    for label, cameras, grid in (("8 cameras x 16 x 12 grid", range(len(cams)), (16, 12)), ("camera 0, 200 x 150 grid", [0], (200, 150))):
      jobs = jobs_of(model, cams, cameras, transfer, grid)
      ul.on_host(uncertainty.run_jobs, model, jobs)
      t = time.perf_counter()
      cov, std, status = ul.on_host(uncertainty.run_jobs, model, jobs)
      dt = time.perf_counter() - t
      n = len(status)
      say(f"host build, one core, {mode}: {label}: {1e3 * dt:.1f} ms, {1e9 * dt / n:.0f} ns a query; a 2000 x 1500 map at that rate "
          f"{3e6 * dt / n:.1f} s (extrapolated, not run)")


if __name__ == "__main__":
  if "--device" in sys.argv:
    device()
  if "--host" in sys.argv:
    host()
  if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "a") as f:
      f.write("\n".join(lines) + "\n")
