"""mcba_reconstruction_uncertainty (multical_amd/reconstruction.py) at cfg3 (8 cameras, 5 Brown-Conrady coefficients, 2000 x 1500):

    volume          the 8 cameras as one group, the 16 x 12 grid of camera 0 at 5 distances (960 points), both references
    map             cameras 0 and 1 as a pair, every pixel of camera 0 at 2 m (3 M points), reference camera 0
    corners         the corners of cfg3 that two or more cameras saw, through Calibration.triangulate(calibration_cov=True)

volume and map run on the truth parameters with a synthetic full-rank covariance over the stored parameters of the group (skews and
the pose of camera 0 held; the time depends on its rank only), corners on the calibration's own covariance.  Prints the four timing
slots of the call (mcba_debug_reconstruction_uncertainty_ms: uploads, HIP-event kernel time, downloads, whole call; medians of 5 calls
after 2 warm-up calls) and the share of the FP64 peak (78.6 TFLOP/s) that the kernel's MFMA loop reaches by counted flops, 2 x 3 x 24 G x
ldw a point (the front -- projections, B = J^T P, the 3 x 3 factorisation -- and the tail are not counted); with --host the g++ build
of the same header on one core (the map on a 200 x 150 grid: its 3 M points are extrapolated, not run).

    python profiles/scripts/prof_reconstruction_uncertainty.py --device [--out FILE]    # needs the GPU
    python profiles/scripts/prof_reconstruction_uncertainty.py --host                   # host build, no GPU
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from multical_amd import guidance, reconstruction, synthetic, uncertainty   # noqa: E402

PEAK = 78.6e12
lines = []


def say(text):
  print(text, flush=True)
  lines.append(text)


def group_model(members):
  rig = synthetic.make_rig("cfg3")
  cams = [rig.truth.cameras[c] for c in members]
  return uncertainty.RigModel(cams, rig.truth.camera_poses[list(members)]), cams


def factors_of(model, seed=1):
  """(factors, r): a synthetic covariance over the stored blocks of the group, skews and the pose of slot 0 held"""
  sizes = [5 + n + 6 for n in model.n_dist]
  p = sum(sizes)
  A = np.random.default_rng(seed).normal(size=(p, p))
  S = 1e-8 * (A @ A.T + 0.1 * np.eye(p))
  dead, at = [], 0
  for c, n in enumerate(sizes):
    dead.append(at + 4)
    if c == 0:
      dead += list(range(at + n - 6, at + n))
    at += n
  S[dead, :] = 0.0
  S[:, dead] = 0.0
  F = guidance.scaled_factor(S)
  out, at = [], 0
  for c, n in enumerate(sizes):
    out.append(guidance.rig_device_factor(model, c, F[at:at + n]))
    at += n
  return out, F.shape[1]


def grid_points(model, px, distances, on_host):
  """reconstruction.grid_points through the library, or through the g++ build of the undistortion"""
  if not on_host:
    return reconstruction.grid_points(model.cameras, model.poses, 0, px, distances).reshape(-1, 3)
  import undistort_host_lib as uh
  with uh.host_backend():
    return reconstruction.grid_points(model.cameras, model.poses, 0, px, distances).reshape(-1, 3)


def workloads(on_host=False):
  """[(label, model, job, r)] of the volume, and what the map is made from"""
  out = []
  big, cams = group_model(range(8))
  factors, r = factors_of(big)
  px = uncertainty.Job(0, None, 1.0, np.zeros((0, 0)), grid=uncertainty.grid_of(cams[0].image_size, (16, 12))).pixel_array()
  pts = grid_points(big, px, [1.0, 1.5, 2.0, 3.0, 4.0], on_host)
  for ref in (None, 0):
    out.append((f"volume: 8 cameras, 16 x 12 x 5, r = {r}, reference {'rig' if ref is None else 'camera 0'}", big,
                reconstruction.Job(range(8), ref, factors, pts), r))
  pair, cams = group_model((0, 1))
  factors, r = factors_of(pair)
  return out, (pair, cams, factors, r)


def timed(model, job, repeats=5, warm=2):
  rows = []
  for i in range(warm + repeats):
    res = reconstruction.run_jobs(model.cameras, model.poses, [job], 0.25, 0.0)
    ms, n = reconstruction.last_call_ms()
    if i >= warm:
      rows.append([ms[k] for k in ("upload", "kernel", "download", "call")])
  return np.median(np.array(rows), axis=0), n, res


def report(label, ms, n, res, G, r):
  ldw = (r + 15) // 16 * 16
  flops = 2.0 * 3 * 24 * G * ldw * n
  say(f"{label}: {n} points, upload {ms[0]:.3f} ms, kernel {ms[1]:.3f} ms ({1e6 * ms[1] / n:.2f} ns a point), download {ms[2]:.3f} ms, call "
      f"{ms[3]:.3f} ms; MFMA loop {flops / 1e9:.3f} GFLOP counted = {flops / (1e-3 * ms[1]) / 1e12:.2f} TFLOP/s = "
      f"{flops / (1e-3 * ms[1]) / PEAK:.3f} of the FP64 peak; {int((res.status == reconstruction.OK).sum())} OK")


def map_points(pair, cams, grid):
  px = uncertainty.Job(0, None, 1.0, np.zeros((0, 0)), grid=uncertainty.grid_of(cams[0].image_size, grid)).pixel_array()
  return px


def device():
  vol, (pair, cams, factors, r) = workloads()
  for label, model, job, rr in vol:
    ms, n, res = timed(model, job)
    report(label, ms, n, res, 8, rr)
  px = map_points(pair, cams, cams[0].image_size)
  pts = grid_points(pair, px, [2.0], False)
  ms, n, res = timed(pair, reconstruction.Job(range(2), 0, factors, pts), repeats=3, warm=1)
  report(f"map: cameras 0 and 1, 2000 x 1500 x 1 at 2 m, r = {r}, reference camera 0", ms, n, res, 2, r)
  from multical_amd import calibration
  c = calibration.from_rig(synthetic.make_rig("cfg3")).enable(cameras=True)
  c.triangulate(calibration_cov=True)
  t = time.perf_counter()
  plain = c.triangulate()
  t_plain = time.perf_counter() - t
  rows = []
  for _ in range(3):
    t = time.perf_counter()
    tab = c.triangulate(calibration_cov=True)
    rows.append(time.perf_counter() - t)
    ms, n = reconstruction.last_call_ms()
  r = c.reconstruction_uncertainty(points=[[0.0, 0.0, 2.0]]).r
  G = c.size.cameras
  flops = 2.0 * 3 * 24 * G * ((r + 15) // 16 * 16) * n
  ok = np.isfinite(tab.cov_cal).all(axis=(-1, -2))
  cal = np.sqrt(np.trace(tab.cov_cal[ok], axis1=-2, axis2=-1))
  noise = np.sqrt(np.trace(tab.cov[ok], axis1=-2, axis2=-1))
  say(f"corners: cfg3, triangulate(calibration_cov=True): {n} corners seen twice or more, the reconstruction call: upload {ms['upload']:.3f} ms, "
      f"kernel {ms['kernel']:.3f} ms ({1e6 * ms['kernel'] / max(n, 1):.2f} ns a corner; G = {G}, r = {r}: MFMA loop {flops / 1e9:.3f} GFLOP counted = "
      f"{flops / (1e-3 * ms['kernel']) / 1e12:.2f} TFLOP/s = {flops / (1e-3 * ms['kernel']) / PEAK:.3f} of the FP64 peak), download {ms['download']:.3f} ms, call {ms['call']:.3f} ms; "
      f"triangulate() {1e3 * t_plain:.1f} ms without, {1e3 * float(np.median(rows)):.1f} ms with the flag (the covariance of the calibration "
      f"included); {int(ok.sum())} OK; median sqrt(trace) calibration {1e3 * float(np.median(cal)):.4f} mm, noise {1e3 * float(np.median(noise)):.4f} mm")


def host():
  import reconstruction_uncertainty_host_lib as rl
  vol, (pair, cams, factors, r) = workloads(on_host=True)
  for label, model, job, rr in vol:
    rl.on_host(reconstruction.run_jobs, model.cameras, model.poses, [job], 0.25, 0.0)
    t = time.perf_counter()
    res = rl.on_host(reconstruction.run_jobs, model.cameras, model.poses, [job], 0.25, 0.0)
    dt = time.perf_counter() - t
    say(f"host build, one core, {label}: {1e3 * dt:.1f} ms, {1e6 * dt / len(res.status):.2f} us a point")
  px = map_points(pair, cams, (200, 150))
  pts = grid_points(pair, px, [2.0], True)
  job = reconstruction.Job(range(2), 0, factors, pts)
  t = time.perf_counter()
  res = rl.on_host(reconstruction.run_jobs, pair.cameras, pair.poses, [job], 0.25, 0.0)
  dt = time.perf_counter() - t
  say(f"host build, one core, map: cameras 0 and 1 on a 200 x 150 grid, r = {r}: {1e3 * dt:.1f} ms, {1e6 * dt / len(res.status):.2f} us a point; "
      f"2000 x 1500 at that rate {3e6 * dt / len(res.status):.1f} s (extrapolated, not run)")


if __name__ == "__main__":
  if "--device" in sys.argv:
    device()
  if "--host" in sys.argv:
    host()
  if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "a") as f:
      f.write("\n".join(lines) + "\n")
