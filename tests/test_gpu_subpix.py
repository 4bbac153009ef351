"""k_refine_corners on the MI355X against the g++ build of the same header (tests/subpix_host): the wave and workgroup edges at four
corners a workgroup, both LDS instantiations (windows of up to 17 x 17 samples and beyond), window pixel counts from 9 to 961 against
64 lanes, both pixel types, the status cases of the host test, repeatability, the grid-stride rounds under a grid cap and the timing
getter.  The host build sums in the order of the device (64 lane partials, xor butterfly: shl.refine_in_wave_order) and neither
side contracts products into FMAs, so the two run the same arithmetic; asserted are the bounds of the feature's contract: at a fixed
count 1e-9 px and 1e-9 relative in the quality, with the reference's criteria eps and one iteration, equal statuses everywhere.

The half window (1, 1) has no stable fixed point on image A (a 3 x 3 window on a corner blurred over more than that: under the
restatement some 250 of 257 starts end REVERTED and a change of 1e-12 px of a start moves results by 0.7 px), so there the bounds hold
only because the arithmetic is the same; in row order the host build differs from the device by up to 0.5 in the relative quality
at that window and by at most rounding at every other."""
import functools

import numpy as np
import pytest

import subpix_host_lib as shl
import subpix_reference as ref
from multical_amd import _lib, subpix

pytestmark = pytest.mark.gpu

EPS = 1e-4
COUNTS = [1, 3, 4, 5, 257]
# (half window, image): 9, 25, 121, 105 window pixels in the small instantiation ((15, 1): 93, small too), 961 in the large one
WINDOWS = [((1, 1), "A"), ((2, 2), "A"), ((5, 5), "A"), ((7, 3), "A"), ((15, 15), "B"), ((15, 1), "B")]
RADIUS = {(1, 1): 0.4, (2, 2): 0.7, (5, 5): 2.0, (7, 3): 1.0, (15, 15): 2.0, (15, 1): 1.0}


@functools.lru_cache(maxsize=None)
def stack(image, dtype):
  """N = 3 copies of the planted image with distinct noise of +-2 grey levels"""
  base = (ref.image_a() if image == "A" else ref.image_b())[0].astype(np.int64)
  rng = np.random.default_rng(17)
  out = np.stack([base + rng.integers(-2, 3, size=base.shape) for _ in range(3)]).clip(0, 255).astype(np.dtype(dtype))
  out.setflags(write=False)
  return out


def corners_of(image, window, n):
  """n starts: the planted corners, cycled, each with noise of its own; the image of every corner"""
  truth = (ref.image_a() if image == "A" else ref.image_b())[1]
  cycled = truth[np.arange(n) % len(truth)]
  return ref.starts(cycled, RADIUS[window], seed=23), (np.arange(n) * 2 % 3).astype(np.int32)


def compare(dev, host, fixed):
  dR, dS, dI, dQ = dev
  hR, hS, hI, hQ = host
  assert np.array_equal(dS, hS)
  assert np.array_equal(np.isnan(dR), np.isnan(hR)) and np.array_equal(np.isnan(dQ), np.isnan(hQ))
  with np.errstate(invalid="ignore"):
    dpos, dq = np.nanmax(np.abs(dR - hR), initial=0.0), np.nanmax(np.abs(dQ - hQ) / np.maximum(np.abs(hQ), 1e-300), initial=0.0)
  if fixed:
    assert (dI == hI).all()
    assert dpos <= 1e-9, dpos
    assert dq <= 1e-9, dq
  else:
    assert dpos <= EPS, dpos
    assert np.abs(dI.astype(int) - hI).max() <= 1
  return dpos


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("window,image", WINDOWS)
def test_against_host_build(window, image, dtype):
  images = stack(image, dtype)
  for n in COUNTS:
    xy, of = corners_of(image, window, n)
    for fixed in (True, False):
      kw = dict(window=window, max_iter=30, eps=0.0 if fixed else EPS)
      mixed = n != 4 and not (n == 257 and fixed)                # image_of_corner mixed in some runs and NULL in others
      of_run = of if mixed else None
      dev = subpix.refine_corners(images, xy, of_run, **kw)
      host = shl.refine_in_wave_order(images, xy, of_run, **kw)
      print(f"{window} {dtype} n={n} {'fixed' if fixed else 'eps'}: statuses equal {np.array_equal(dev[1], host[1])}, "
            f"device - host build {np.nanmax(np.abs(dev[0] - host[0]), initial=0.0):.3e} px, statuses {np.bincount(host[1], minlength=6)}")
      compare(dev, host, fixed)
      if window in ((5, 5), (15, 15)) and not fixed:
        assert (dev[1] == subpix.OK).mean() > 0.9                # the planted corners converge on the noisy copies too


@pytest.mark.parametrize("case", shl.status_cases(), ids=lambda c: c[0])
def test_status_cases(case):
  name, img, corners, kw = case
  for dtype in (np.uint8, np.float32):
    images = ref.as_dtype(img, dtype)
    dev = subpix.refine_corners(images, corners, **kw)
    host = shl.refine_in_wave_order(images, corners, **kw)
    compare(dev, host, True)
    kept = np.isin(dev[1], [subpix.REVERTED, subpix.INVALID, subpix.SINGULAR])
    assert dev[0][kept].tobytes() == np.asarray(corners, dtype=np.float64)[kept].tobytes()
  if name == "constant":
    assert (dev[1] == subpix.SINGULAR).all() and (dev[3] == 0.0).all()
  if name == "invalid":
    assert (dev[1] == subpix.INVALID).all() and np.isnan(dev[3]).all() and (dev[2] == 0).all()


def test_zero_zone_and_refusals():
  images = stack("A", "uint8")
  xy, of = corners_of("A", (5, 5), 25)
  for zone in ((0, 0), (2, 1), (5, 5)):
    kw = dict(window=5, zero_zone=zone, max_iter=2, eps=0.0)
    compare(subpix.refine_corners(images, xy, of, **kw), shl.refine_in_wave_order(images, xy, of, **kw), True)
  with pytest.raises(_lib.McbaError, match="half window must be 1 .. 15"):
    subpix.refine_corners(images, xy, of, window=16)
  with pytest.raises(_lib.McbaError, match="max_iter must be 1 .. 100"):
    subpix.refine_corners(images, xy, of, max_iter=0)
  bad = of.copy()
  bad[11] = 3
  with pytest.raises(_lib.McbaError, match="corner 11 names image 3 of 3"):
    subpix.refine_corners(images, xy, bad)
  assert [len(a) for a in subpix.refine_corners(images, np.zeros((0, 2)))] == [0, 0, 0, 0]


def test_same_bytes_twice():
  for window, image in (((5, 5), "A"), ((15, 15), "B")):
    images = stack(image, "uint8")
    xy, of = corners_of(image, window, 257)
    first = subpix.refine_corners(images, xy, of, window=window)
    decoy = subpix.refine_corners(images, xy[::-1].copy(), of, window=window)      # (fills the cached output buffers with other values)
    assert decoy[0].tobytes() != first[0].tobytes()
    second = subpix.refine_corners(images, xy, of, window=window)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))


def test_grid_cap_rounds():
  """n = 9 corners are three workgroups: under a cap of 1 and 2 a workgroup takes a second and a third round and returns the bytes of
  the uncapped launch"""
  images = stack("A", "uint8")
  xy, of = corners_of("A", (5, 5), 9)
  try:
    _lib.set_grid_cap(0)
    base = subpix.refine_corners(images, xy, of)
    assert _lib.last_capped_grid() == 3
    assert (base[1] == subpix.OK).all()
    for cap in (1, 2):
      _lib.set_grid_cap(0)
      subpix.refine_corners(images, xy[::-1].copy(), of)                           # the decoy
      _lib.set_grid_cap(cap)
      got = subpix.refine_corners(images, xy, of)
      assert _lib.last_capped_grid() == min(cap, 3)
      assert all(a.tobytes() == b.tobytes() for a, b in zip(got, base)), cap
  finally:
    _lib.set_grid_cap(0)


def test_last_call_ms():
  images = stack("A", "uint8")
  xy, of = corners_of("A", (5, 5), 257)
  subpix.refine_corners(images, xy, of)
  ms, n = subpix.last_call_ms()
  assert n == 257 and list(ms) == ["upload", "kernel", "download", "call"]
  assert all(np.isfinite(v) and v >= 0.0 for v in ms.values())
  assert ms["call"] >= ms["kernel"] > 0.0
