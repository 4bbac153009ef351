"""The corner refinement (multical_amd/subpix.py) at the size of a real rig: 8 cameras x 16 images of 2000 x 1500 (uint8) in one call,
window = 5 and the reference's criteria (30 iterations, eps = 1e-4).  The images are rendered checkers of 40 px squares, blurred
(sigma = 1) and shifted per image, with seeded noise of +-2 grey levels; the starts are the planted corners plus uniform noise of
1.5 px.  Two runs:

    frames       the corners of those 128 frames at the density of cfg3 (764 k corners over 4 000 images: 191 an image)
    north star   764 k corners spread over the same 128 images: the kernel at the north-star count without a 12 GB upload

Reports, per run, the HIP-event kernel time (mcba_debug_subpix_ms, median of 5 calls after 2 warm-up calls), the whole call with its
upload share, the mean iterations a corner and the statuses; as comparison the g++ build of the same header on one core over the
same input, and the numpy restatement (tests/subpix_reference.py) on a subset.  Nothing comparable exists before this feature: the
figures are what they are named, not a speed-up over an earlier state.

    python profiles/scripts/prof_subpix.py --out profiles/subpix_timing.txt       # needs the GPU
    python profiles/scripts/prof_subpix.py --images 4 --size 400x300 --host-only   # rehearsal, no GPU
"""
import os
import sys
import time

import numpy as np
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from multical_amd import subpix   # noqa: E402

SQUARE = 40
DENSITY = 764_000 / 4_000        # corners an image at cfg3
NORTH_STAR = 764_000


def option(name, default):
  return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def render(n, size, seed=1):
  """(images [n, H, W] uint8, corners of every image [n][k, 2]): one blurred checker, shifted per image, noise of +-2 per image"""
  W, H = size
  rng = np.random.default_rng(seed)
  sub = 2
  y, x = np.mgrid[0:(H + SQUARE) * sub, 0:(W + SQUARE) * sub]
  fine = np.where(((x // (SQUARE * sub)) + (y // (SQUARE * sub))) % 2 == 0, 40.0, 210.0)
  base = ndimage.gaussian_filter(fine.reshape(H + SQUARE, sub, W + SQUARE, sub).mean(axis=(1, 3)), 1.0, mode="nearest")
  images, corners = np.empty((n, H, W), dtype=np.uint8), []
  for i in range(n):
    dx, dy = rng.integers(0, SQUARE, size=2)
    noise = rng.integers(-2, 3, size=(H, W), dtype=np.int16)
    images[i] = np.clip(np.rint(base[dy:dy + H, dx:dx + W]).astype(np.int16) + noise, 0, 255).astype(np.uint8)
    # pixel (r, c) of the base holds the box average around (r, c): the corner k SQUARE of the fine grid lies at k SQUARE - 0.5
    gx = np.arange(SQUARE, W + SQUARE, SQUARE) - 0.5 - dx
    gy = np.arange(SQUARE, H + SQUARE, SQUARE) - 0.5 - dy
    gx, gy = gx[(gx > 12) & (gx < W - 13)], gy[(gy > 12) & (gy < H - 13)]
    corners.append(np.stack(np.meshgrid(gx, gy), axis=-1).reshape(-1, 2))
  return images, corners


def pick(corners, total, seed):
  """`total` starts spread evenly over the images: (truth [total, 2], starts, image_of_corner)"""
  rng = np.random.default_rng(seed)
  n = len(corners)
  per = [total // n + (1 if i < total % n else 0) for i in range(n)]
  truth = np.concatenate([c[rng.integers(0, len(c), size=k)] for c, k in zip(corners, per)])
  of = np.repeat(np.arange(n, dtype=np.int32), per)
  return truth, truth + rng.uniform(-1.5, 1.5, size=truth.shape), of


def statuses(st):
  names = ["ok", "max_iter", "singular", "left_image", "reverted", "invalid"]
  return ", ".join(f"{names[i]} {c}" for i, c in enumerate(np.bincount(st, minlength=6)) if c)


def main():
  n_images = int(option("--images", 128))
  size = tuple(int(v) for v in option("--size", "2000x1500").split("x"))
  host_only = "--host-only" in sys.argv
  out_path = option("--out", None)
  lines = []

  def say(text=""):
    print(text, flush=True)
    lines.append(text)

  import subpix_host_lib as shl
  import subpix_reference as ref
  t0 = time.time()
  images, corners = render(n_images, size)
  say(f"corner refinement, window 5, 30 iterations, eps 1e-4: {n_images} images of {size[0]} x {size[1]} uint8 "
      f"({images.nbytes / 1e6:.0f} MB), rendered in {time.time() - t0:.1f} s")
  scale = n_images / 128
  for label, total in (("frames", int(round(DENSITY * n_images))), ("north star", int(round(NORTH_STAR * scale)))):
    truth, start, of = pick(corners, total, seed=len(label))
    say(f"\n{label}: {total} corners")
    if not host_only:
      runs = []
      for _ in range(7):
        t = time.perf_counter()
        R, S, I, Q = subpix.refine_corners(images, start, of, window=5)
        wall = (time.perf_counter() - t) * 1e3
        ms, n = subpix.last_call_ms()
        runs.append((ms["kernel"], ms["upload"], ms["download"], ms["call"], wall))
      k, up, down, call, wall = np.median(np.array(runs[2:]), axis=0)
      err = np.linalg.norm(R - truth, axis=1)
      say(f"  device   kernel (HIP events) {k:9.3f} ms = {k * 1e3 / total:7.3f} us a corner; call {call:9.2f} ms of which upload {up:9.2f} ms "
          f"({100 * up / call:.0f} %), download {down:.2f} ms; python wall {wall:.1f} ms")
      say(f"           mean iterations {I.mean():.2f}, worst {I.max()}; {statuses(S)}; error to the planted corner: median {np.median(err):.4f} px, "
          f"worst {err.max():.4f} px")
    t = time.perf_counter()
    hR, hS, hI, hQ = shl.refine_on_host(images, start, of, window=5)
    host_s = time.perf_counter() - t
    say(f"  host     g++ build of the same header, one core: {host_s * 1e3:9.1f} ms = {host_s * 1e6 / total:7.3f} us a corner; "
        f"mean iterations {hI.mean():.2f}; {statuses(hS)}")
    if not host_only:
      say(f"           device - host build: positions {np.abs(R - hR).max():.2e} px, statuses differ at {(S != hS).sum()} corners, "
          f"iterations at {(I != hI).sum()}")
    sub = np.arange(0, total, max(1, total // 200))[:200]
    t = time.perf_counter()
    rR = np.concatenate([ref.refine(images[of[i]], start[i:i + 1], 5)[0] for i in sub])
    ref_s = time.perf_counter() - t
    say(f"  numpy    restatement on {len(sub)} corners: {ref_s * 1e6 / len(sub):9.1f} us a corner; host build - restatement "
        f"{np.abs(hR[sub] - rR).max():.2e} px")
  if out_path:
    with open(out_path, "w") as f:
      f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
