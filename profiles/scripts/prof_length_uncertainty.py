"""mcba_reconstruction_pairs (multical_amd/reconstruction.py: run_pair_jobs) at cfg3 (8 cameras, 5 Brown-Conrady coefficients, 2000 x 1500):

    boards          Calibration.length_errors() with its default pairs (every corner with the corner farthest from it on its board):
                    the 8 cameras as one group, the calibration's own covariance, the views the triangulation offered each corner
    map             cameras 0 and 1 as a pair, the 1000 x 750 grid of camera 0 at 2 m, every point with its right-hand neighbour,
                    reference camera 0, a synthetic full-rank covariance (prof_reconstruction_uncertainty.factors_of)

Prints the four timing slots of the call (mcba_debug_reconstruction_pairs_ms: uploads, HIP-event kernel time, downloads, whole call;
medians of 5 calls after 2 warm-up calls) and the share of the FP64 peak (78.6 TFLOP/s) the MFMA loop reaches by counted flops,
2 ends x 2 x 3 x 24 G x ldw a pair (front and tail are not counted).  The yardstick is k_reconstruction_uncertainty over the same ends as
2 x pairs points (points[pairs], masks[pairs]) re-measured in the same run: the pair kernel does the same front and product per end and a
longer tail.  The ratio is reported, not asserted.  With --host the g++ build of the same header on one core over the same jobs (the
map on a 200 x 150 grid).

    python profiles/scripts/prof_length_uncertainty.py --device [--host] [--out FILE]    # needs the GPU
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from multical_amd import calibration, reconstruction, synthetic, uncertainty   # noqa: E402
import prof_reconstruction_uncertainty as point_prof                          # noqa: E402

PEAK = 78.6e12
lines = []
SLOTS = ("upload", "kernel", "download", "call")


def say(text):
  print(text, flush=True)
  lines.append(text)


def timed(call, getter, repeats=5, warm=2):
  rows = []
  for i in range(warm + repeats):
    res = call()
    ms, n = getter()
    if i >= warm:
      rows.append([ms[k] for k in SLOTS])
  return np.median(np.array(rows), axis=0), n, res


def measure(label, cameras, poses, job, pairs, sigma2=0.25, margin=0.0):
  """the pair call over (job, pairs) and the point call over the same ends, 2 x pairs points"""
  pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
  G, r = len(job.group), job.factors[0][0].shape[1]
  ldw = (r + 15) // 16 * 16
  ms, n, res = timed(lambda: reconstruction.run_pair_jobs(cameras, poses, [job], [pairs], sigma2, margin), reconstruction.last_pair_call_ms)
  flops = 2.0 * 2.0 * 3 * 24 * G * ldw * n
  ok = int((res.status == reconstruction.OK).sum())
  say(f"{label}: G = {G}, r = {r}, {n} pairs over {len(job.points)} points: upload {ms[0]:.3f} ms, kernel {ms[1]:.3f} ms ({1e6 * ms[1] / n:.2f} ns a "
      f"pair), download {ms[2]:.3f} ms, call {ms[3]:.3f} ms; MFMA loop {flops / 1e9:.3f} GFLOP counted = {flops / (1e-3 * ms[1]) / 1e12:.2f} TFLOP/s "
      f"= {flops / (1e-3 * ms[1]) / PEAK:.3f} of the FP64 peak; {ok} OK")
  ends = reconstruction.Job(job.group, job.reference, job.factors, job.points[pairs.ravel()],
                            None if job.masks is None else job.masks[pairs.ravel()])
  pm, pn, _ = timed(lambda: reconstruction.run_jobs(cameras, poses, [ends], sigma2, margin), reconstruction.last_call_ms)
  say(f"    yardstick, k_reconstruction_uncertainty over the same ends: {pn} points, kernel {pm[1]:.3f} ms ({1e6 * pm[1] / pn:.2f} ns a point), "
      f"call {pm[3]:.3f} ms; pair kernel / point kernel = {ms[1] / pm[1]:.3f}, pair call / point call = {ms[3] / pm[3]:.3f}")
  return res


def on_host(label, cameras, poses, job, pairs):
  import length_uncertainty_host_lib as ll
  t = time.perf_counter()
  res = ll.on_host(reconstruction.run_pair_jobs, cameras, poses, [job], [pairs], 0.25, 0.0)
  dt = time.perf_counter() - t
  say(f"host build, one core, {label}: {len(res.status)} pairs, {1e3 * dt:.1f} ms, {1e6 * dt / max(len(res.status), 1):.2f} us a pair")


def boards_job():
  """what Calibration.length_errors() of cfg3 sends to run_pair_jobs, captured from one call"""
  c = calibration.from_rig(synthetic.make_rig("cfg3")).enable(cameras=True)
  seen, real = [], reconstruction.run_pair_jobs

  def capture(cameras, poses, jobs, pairs, sigma2=1.0, margin=0.0):
    seen.append((cameras, poses, jobs[0], np.asarray(pairs[0], dtype=np.int64), sigma2, margin))
    return real(cameras, poses, jobs, pairs, sigma2, margin)
  reconstruction.run_pair_jobs = capture
  try:
    t = time.perf_counter()
    e = c.length_errors()
    dt = time.perf_counter() - t
  finally:
    reconstruction.run_pair_jobs = real
  s = e.studentized[e.valid]
  say(f"boards: cfg3 length_errors(): {1e3 * dt:.1f} ms in all (triangulate, covariance and its factor included); {int(e.valid.sum())} valid pairs; "
      f"length error RMS {1e3 * e.overall.rms:.4f} mm, median std calibration {1e3 * float(np.median(e.std_cal[e.valid])):.4f} mm, noise "
      f"{1e3 * float(np.median(e.std_noise[e.valid])):.4f} mm; studentised RMS {float(np.sqrt(np.mean(s ** 2))):.3f}, median |.| "
      f"{float(np.median(np.abs(s))):.3f} (in-sample)")
  return seen[0]


def map_job(grid, on_host_build=False):
  pair, cams = point_prof.group_model((0, 1))
  factors, _ = point_prof.factors_of(pair)
  px = uncertainty.Job(0, None, 1.0, np.zeros((0, 0)), grid=uncertainty.grid_of(cams[0].image_size, grid)).pixel_array()
  pts = point_prof.grid_points(pair, px, [2.0], on_host_build)
  pairs = np.stack([np.arange(len(pts) - 1), np.arange(1, len(pts))], axis=1)
  return pair, reconstruction.Job(range(2), 0, factors, pts), pairs


if __name__ == "__main__":
  host = "--host" in sys.argv
  if "--device" in sys.argv:
    cameras, poses, job, pairs, sigma2, margin = boards_job()
    measure("boards: cfg3 length_errors() default pairs", cameras, poses, job, pairs, sigma2, margin)
    if host:
      on_host("boards: cfg3 length_errors() default pairs", cameras, poses, job, pairs)
    pair, mjob, mpairs = map_job((1000, 750))
    measure("map: cameras 0 and 1, 1000 x 750 at 2 m, neighbours, reference camera 0", pair.cameras, pair.poses, mjob, mpairs)
  if host:
    pair, mjob, mpairs = map_job((200, 150), True)
    on_host("map: cameras 0 and 1 on a 200 x 150 grid, neighbours", pair.cameras, pair.poses, mjob, mpairs)
  if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "a") as f:
      f.write("\n".join(lines) + "\n")
