"""The corrected entry points at cfg3's 8 cameras: the forward warp of the whole observation table
(mcba_warp_points over its 2.59 M slots), a 2000 x 1500 corrected map per camera (mcba_undistort_maps_corrected), 8 x 16 images
through mcba_undistort_images_corrected, each next to the uncorrected call of the same shape (the difference is the price of the
Newton inverse), and one round of Calibration.refine_with_residual_field.  Kernel time by HIP events (mcba_debug_warp_ms /
mcba_debug_undistort_ms), the whole call by host clock, the wall time from Python.  Medians of 5 calls after 1 warm-up call.
`--cpu` times the g++ build of the same header on one core instead (needs no GPU; run from the repository root).

    python profiles/scripts/prof_residual_correction.py [--cpu]
"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from multical_amd import calibration, correction, synthetic, undistort   # noqa: E402
from multical_amd.correction import FieldCorrection                      # noqa: E402

MAP_SIZE, IMAGES_PER_CAMERA = (2000, 1500), 16


def med(f, n=5, warm=1):
  for _ in range(warm):
    f()
  out = []
  for _ in range(n):
    t0 = time.perf_counter()
    r = f()
    out.append([(time.perf_counter() - t0) * 1e3] + list(r or []))
  return np.median(np.array(out), axis=0)


def field_for(sizes, seed=3):
  rng = np.random.default_rng(seed)
  f = FieldCorrection(rng.normal(size=(len(sizes), 56, 2)), sizes, 5, 4)
  return FieldCorrection(f.coefficients * (0.1 / f.fold_bound().max()), sizes, 5, 4)


def main(cpu):
  rig = synthetic.make_rig("cfg3")
  c = calibration.from_rig(rig)
  cams = list(c.cameras)
  sizes = [tuple(int(v) for v in cam.image_size) for cam in cams]
  C, F, B, P = rig.valid.shape
  f = field_for(sizes)
  table = c.point_table
  of = np.repeat(np.arange(C), IMAGES_PER_CAMERA).astype(np.int32)
  images = np.random.default_rng(1).integers(0, 256, (len(of), MAP_SIZE[1], MAP_SIZE[0]), dtype=np.uint8)
  print(f"cfg3: {C} cameras, table {C} x {F} x {B} x {P} = {C * F * B * P} slots, fold bound {f.fold_bound().max():.3f}, maps {MAP_SIZE}, "
        f"{len(of)} images uint8 x 1")
  if cpu:
    sys.path.insert(0, "tests")
    import correction_host_lib as ch
    import undistort_host_lib as uh
    with uh.host_backend(), ch.host_backend():
      print(f"  g++ build, one core: correct_table wall {med(lambda: f.correct_table(table) and None, 2, 0)[0]:10.1f} ms")
      print(f"  g++ build, one core: corrected maps wall {med(lambda: undistort.undistort_maps(cams, MAP_SIZE, correction=f) is None, 2, 0)[0]:10.1f} ms"
            f"   plain maps wall {med(lambda: undistort.undistort_maps(cams, MAP_SIZE) is None, 2, 0)[0]:10.1f} ms")
    return

  def timed(call, last):
    def run():
      call()
      ms, _ = last()
      return [ms["kernel"], ms["call"]]
    w, kernel, whole = med(run)
    return f"kernel {kernel * 1e3:9.1f} us   call {whole:9.3f} ms   wall from Python {w:9.3f} ms"

  print(f"  correct_table (mcba_warp_points, forward, {C * F * B * P} slots)   {timed(lambda: f.correct_table(table), correction.last_call_ms)}")
  px = np.asarray(table.points, dtype=np.float64).reshape(-1, 2)
  cam_of = np.repeat(np.arange(C, dtype=np.int32), F * B * P)
  px = np.where(np.isfinite(px), px, 0.0)
  print(f"  mcba_warp_points inverse, same list                              {timed(lambda: f.uncorrect(px, cam_of), correction.last_call_ms)}")
  print(f"  mcba_undistort_maps_corrected {MAP_SIZE} x {C}                    {timed(lambda: undistort.undistort_maps(cams, MAP_SIZE, correction=f), correction.last_call_ms)}")
  print(f"  mcba_undistort_maps           {MAP_SIZE} x {C}                    {timed(lambda: undistort.undistort_maps(cams, MAP_SIZE), undistort.last_call_ms)}")
  print(f"  mcba_undistort_images_corrected {len(of)} images                      {timed(lambda: undistort.undistort_images(cams, images, of, correction=f), correction.last_call_ms)}")
  print(f"  mcba_undistort_images           {len(of)} images                      {timed(lambda: undistort.undistort_images(cams, images, of), undistort.last_call_ms)}")
  start = c.bundle_adjust(solver="native", tolerance=1e-8)
  sigma2 = start.covariance().sigma2
  t0 = time.perf_counter()
  out, records = start.refine_with_residual_field(rounds=1, sigma2=sigma2, solver="native", tolerance=1e-8)
  print(f"  one refine_with_residual_field round (fit + corrected table + bundle_adjust, native, tolerance 1e-8): wall "
        f"{(time.perf_counter() - t0) * 1e3:9.1f} ms; sse {records[0].sse:.3f} penalty {records[0].penalty:.6f}")


if __name__ == "__main__":
  main("--cpu" in sys.argv[1:])
