"""The undistortion calls (multical_amd/undistort.py) at the size of a real rig: 8 cameras x 16 images of 2000 x 1500 in one call,
uint8 grey and uint8 3-channel.  Prints, per format, the HIP-event kernel time (mcba_debug_undistort_ms; medians of 5 calls after 2
warm-up calls, the fused and the two-step route alternating inside one process) of

    fused        undistort_images: the map coordinate in registers
    two-step     undistort_maps (once per camera) + remap through the maps

the bytes each kernel must move (source + destination (+ map)) over that time, the upload / download share of the whole call, and
whether both routes returned the same bytes.  --host times the g++ build of the same header on one core (one image).

    python profiles/scripts/prof_undistort.py --device      # needs the GPU
    python profiles/scripts/prof_undistort.py --host        # host build, no GPU
    python profiles/scripts/prof_undistort.py --device --images 2 --size 400x300     # rehearsal sizes
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from multical_amd import undistort   # noqa: E402

COPY_RATE = 6.3e12      # measured device copy rate of the MI355X, bytes / s


def option(name, default):
  return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def cameras_at(size):
  """the eight fixture cameras of the undistortion tests, at image size `size`"""
  import undistort_host_lib as uh
  import pnp_host_lib
  out = []
  for name, index in uh.CAMERA_FIXTURES:
    full = pnp_host_lib.golden_rig(name).truth.cameras[index].image_size
    out.append(uh.fixture_camera(name, index).scale_image(size[0] / (uh.SCALE * full[0])).copy(image_size=size))
  return out


def images(n, size, channels):
  """n noise images (a 256 x 256 patch tiled: the values do not change what the kernel does)"""
  patch = np.random.default_rng(1).integers(0, 256, (256, 256, channels), dtype=np.uint8)
  one = np.tile(patch, (size[1] // 256 + 1, size[0] // 256 + 1, 1))[:size[1], :size[0]]
  return np.ascontiguousarray(np.broadcast_to(one if channels == 3 else one[..., 0], (n,) + one.shape[:2] + ((3,) if channels == 3 else ())))


def timed(call, repeats=5, warmup=2):
  """medians of the library's four phase times over `repeats` calls, and the last result"""
  rows = []
  for i in range(warmup + repeats):
    out = call()
    ms, count = undistort.last_call_ms()
    if i >= warmup:
      rows.append([ms["upload"], ms["kernel"], ms["download"], ms["call"]])
  return np.median(np.array(rows), axis=0), out, count


def rate(nbytes, ms):
  r = nbytes / (ms * 1e-3)
  return f"{r / 1e12:6.3f} TB/s ({100.0 * r / COPY_RATE:4.1f} % of the 6.3 TB/s copy rate)"


def main():
  size = tuple(int(v) for v in option("--size", "2000x1500").split("x"))
  per_camera = int(option("--images", "16"))
  cams = cameras_at(size)
  n = len(cams) * per_camera
  of = np.repeat(np.arange(len(cams), dtype=np.int32), per_camera)
  pixels = n * size[0] * size[1]
  print(f"{len(cams)} cameras x {per_camera} images of {size[0]} x {size[1]}: {pixels / 1e6:.0f} Mpixel a call")
  for channels in (1, 3):
    label = "uint8 grey" if channels == 1 else "uint8 3-channel"
    if "--device" in sys.argv:
      src = images(n, size, channels)
      image_bytes = 2 * pixels * channels                               # source read once + destination written once
      map_bytes = len(cams) * size[0] * size[1] * 8
      fused, out_fused, _ = timed(lambda: undistort.undistort_images(cams, src, of))
      maps_ms, maps, _ = timed(lambda: undistort.undistort_maps(cams, size))
      remap, out_two, _ = timed(lambda: undistort.remap(src, maps, of))
      again, _, _ = timed(lambda: undistort.undistort_images(cams, src, of), repeats=3, warmup=0)
      print(f"{label}: fused and two-step results identical: {out_fused.tobytes() == out_two.tobytes()}")
      print(f"  fused     kernel {fused[1]:9.3f} ms (repeat after the two-step runs {again[1]:9.3f} ms)  {rate(image_bytes, fused[1])}")
      print(f"            whole call {fused[3]:9.1f} ms: uploads {fused[0]:9.1f} ms ({100 * fused[0] / fused[3]:4.1f} %), downloads "
            f"{fused[2]:9.1f} ms ({100 * fused[2] / fused[3]:4.1f} %), kernel {100 * fused[1] / fused[3]:4.1f} %")
      print(f"  two-step  kernels {maps_ms[1] + remap[1]:9.3f} ms = maps {maps_ms[1]:9.3f} ms ({rate(map_bytes, maps_ms[1])}) + remap "
            f"{remap[1]:9.3f} ms ({rate(image_bytes + pixels * 8, remap[1])})")
      print(f"            whole calls {maps_ms[3] + remap[3]:9.1f} ms")
      print("  source taps: direct loads (the form in the library); the LDS-staged form is not built: **unmeasured**")
    if "--host" in sys.argv:
      import undistort_host_lib as uh
      one = images(1, size, channels)
      t0 = time.perf_counter()
      uh.on_host(undistort.undistort_images, cams[:1], one)
      t_fused = time.perf_counter() - t0
      maps = uh.on_host(undistort.undistort_maps, cams[:1], size)
      t0 = time.perf_counter()
      uh.on_host(undistort.remap, one, maps)
      t_remap = time.perf_counter() - t0
      print(f"{label}: host build of csrc/mcba_undistort.h (g++ -O2, one core), ONE image: fused {t_fused * 1e3:9.1f} ms, remap through a "
            f"given map {t_remap * 1e3:9.1f} ms; x {n} images = {t_fused * n:7.1f} s / {t_remap * n:7.1f} s a call")


if __name__ == "__main__":
  main()
