"""The undistortion entry points on the device (k_point_ops, k_undistort_map, k_remap_cubic) against the g++ build of the same header
(undistort_host_lib): points within 1e-9 px, maps within 1 float32 ulp, images byte for byte."""
import numpy as np
import pytest

from multical_amd import camera as camera_module
from multical_amd import undistort

import undistort_host_lib as uh
import undistort_reference as ref

pytestmark = pytest.mark.gpu

CAMERAS = uh.fixture_cameras()
W, H = uh.IMAGE_SIZE
# (width, height): flat path x 4, row path x 5 -- one x-tile of 256 columns (256, 200), two (260: one group in the second; 512: both
# full) and three (516: one group in the third)
SIZES = [(1, 1), (3, 2), (255, 3), (256, 4), (257, 5), (200, 150), (260, 4), (512, 3), (516, 5)]
DTYPES = [np.uint8, np.float32]


def zoomed(cams, factor=0.5):
  return np.stack([uh.zoomed_out(c, factor) for c in cams])


# ---- points ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_points_match_host_build(n):
  rng = np.random.default_rng(100 + n)
  of = rng.integers(0, len(CAMERAS), n).astype(np.int32)            # (not monotone)
  X = np.concatenate([rng.uniform(-0.3, 0.3, (n, 2)), np.ones((n, 1))], axis=1) * rng.uniform(0.5, 3.0, (n, 1))
  uv = undistort.project_points(CAMERAS, X, of)
  assert np.abs(uv - uh.on_host(undistort.project_points, CAMERAS, X, of)).max() < 1e-9
  px = rng.uniform(0.0, 1.0, (n, 2)) * [W - 1, H - 1]
  fisheye = np.array([ref.is_fisheye(c) for c in CAMERAS])[of]
  px[fisheye & (np.arange(n) % 3 == 0)] = [5000.0, 4000.0]          # a fisheye camera cannot have produced this pixel
  R = np.stack([uh.small_rotation((1.0 + c, -2.0, 0.5 * c)) for c in range(len(CAMERAS))])
  fx = np.array([c.intrinsic[0, 0] for c in CAMERAS])[of][:, None]
  for kwargs, scale in ((dict(), fx), (dict(P=zoomed(CAMERAS, 1.0)), 1.0), (dict(R=R, P=zoomed(CAMERAS)), 1.0), (dict(R=R), fx)):
    got, status = undistort.undistort_points(CAMERAS, px, of, **kwargs)
    want, want_status = uh.on_host(undistort.undistort_points, CAMERAS, px, of, **kwargs)
    assert np.array_equal(status, want_status)
    ok = status == undistort.UNDISTORT_OK
    assert np.isnan(got[~ok]).all() and (np.abs(got[ok] - want[ok]) * (scale[ok] if np.ndim(scale) else scale)).max(initial=0.0) < 1e-9
  if n == 1000:
    assert (status != undistort.UNDISTORT_OK).any() and (status == undistort.UNDISTORT_OK).sum() > 800
  ms, count = undistort.last_call_ms()
  assert count == n and ms["kernel"] > 0.0 and ms["call"] >= ms["kernel"]


def test_no_points_is_no_launch():
  assert undistort.project_points(CAMERAS, np.zeros((0, 3))).shape == (0, 2)
  out, status = undistort.undistort_points(CAMERAS, np.zeros((0, 2)))
  assert out.shape == (0, 2) and status.shape == (0,)
  assert undistort.last_call_ms()[1] == 0


# ---- maps --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_maps_match_host_build(size):
  """every camera family in one call; the device contracts the FP64 projection to FMAs, the host build does not: an entry differs
  only where that difference straddles a float32 rounding boundary"""
  for label, kwargs in (("P=K", dict()), ("zoomed out", dict(P=zoomed(CAMERAS))),
                        ("rotated", dict(R=uh.small_rotation(), P=zoomed(CAMERAS, 0.8)))):
    got = undistort.undistort_maps(CAMERAS, size, **kwargs)
    want = uh.on_host(undistort.undistort_maps, CAMERAS, size, **kwargs)
    assert got.shape == (len(CAMERAS), size[1], size[0], 2) and got.dtype == np.float32
    d = uh.ulp_distance(got, want)
    print(f"{size} {label}: {int((d > 0).sum())} of {d.size} entries are not bit-identical, at most {int(d.max())} ulp")
    assert d.max() <= 1


# ---- remap through given maps --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "f32"])
def test_remap_is_byte_identical_to_host_build(dtype, channels):
  """source 130 x 70, random maps with the edge coordinates planted, N = 1 and 5 images over two maps"""
  hs, ws = 70, 130
  images = uh.noise_image(200 + channels, (5, hs, ws) + ((3,) if channels == 3 else ()), dtype)
  for wd, hd in SIZES:
    maps = uh.random_maps(300 + wd, 2, hd, wd, hs, ws)
    for n, of in ((1, [1]), (5, [1, 0, 1, 1, 0])):
      got = undistort.remap(images[:n], maps, of, border=6.0)
      want = uh.on_host(undistort.remap, images[:n], maps, of, border=6.0)
      assert got.shape == want.shape and got.dtype == want.dtype
      assert got.tobytes() == want.tobytes(), f"{wd} x {hd}, {n} images: {int((got != want).sum())} values differ"


def test_remap_identity_on_device():
  img = uh.noise_image(7, (2, 37, 52, 3), np.uint8)
  u, v = np.meshgrid(np.arange(52, dtype=np.float32), np.arange(37, dtype=np.float32))
  assert undistort.remap(img, np.stack([u, v], axis=-1)).tobytes() == img.tobytes()
  with pytest.raises(RuntimeError, match="channels"):
    undistort.remap(np.zeros((1, 4, 4, 2), dtype=np.uint8), np.zeros((4, 4, 2), dtype=np.float32))
  assert undistort.remap(np.zeros((0, 4, 4), dtype=np.uint8), np.zeros((4, 4, 2), dtype=np.float32)).shape == (0, 4, 4)


# ---- the fused form ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "f32"])
def test_fused_equals_remap_through_device_maps(dtype, channels):
  """undistort_images = remap(images, undistort_maps) byte for byte: every family, P = K and a zoomed-out P, two row-path sizes (one
  and three x-tiles) and a flat-path size, every camera with an image and one camera without; and the same call twice returns the
  same bytes"""
  n = len(CAMERAS) + 3
  of = (np.arange(n) * 5 % len(CAMERAS)).astype(np.int32)
  gap = np.where(of == 2, 6, of).astype(np.int32)                   # camera 2 has no image, camera 6 has those as well
  assert set(of) == set(range(len(CAMERAS))) and 2 not in gap and (gap == 6).sum() >= 2
  images = uh.noise_image(400 + channels, (n, H, W) + ((3,) if channels == 3 else ()), dtype)
  for size in ((W, H), (516, 5), (57, 5)):
    for kwargs in (dict(), dict(P=zoomed(CAMERAS))):
      maps = undistort.undistort_maps(CAMERAS, size, **kwargs)
      for index in (of, gap):
        two = undistort.remap(images, maps, index)
        fused = undistort.undistort_images(CAMERAS, images, index, image_size=size, **kwargs)
        assert fused.shape == two.shape and fused.tobytes() == two.tobytes()
        assert undistort.undistort_images(CAMERAS, images, index, image_size=size, **kwargs).tobytes() == fused.tobytes()
  ms, count = undistort.last_call_ms()
  assert count == n * 57 * 5 and ms["kernel"] > 0.0


# ---- end to end --------------------------------------------------------------------------------------------------------------
def checker_seen_by(cam, rows, cols):
  """what the camera sees of a checker whose edges are the lines v = rows[k], u = cols[k] of its undistorted image: the restatement
  projects every line into the (distorted) source image; a source pixel's cell is the number of edges above / left of it"""
  K = np.asarray(cam.intrinsic)
  s = np.linspace(-300.0, 500.0, 4001)
  x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
  above, left = np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64)
  for v0 in rows:
    c = ref.project(cam, np.stack([(s - K[0, 2]) / K[0, 0], np.full_like(s, (v0 - K[1, 2]) / K[1, 1]), np.ones_like(s)], axis=1))
    above += y[:, None] > np.interp(x, c[:, 0], c[:, 1])[None, :]
  for u0 in cols:
    c = ref.project(cam, np.stack([np.full_like(s, (u0 - K[0, 2]) / K[0, 0]), (s - K[1, 2]) / K[1, 1], np.ones_like(s)], axis=1))
    left += x[None, :] > np.interp(y, c[:, 1], c[:, 0])[:, None]
  return (((above + left) % 2) * 255).astype(np.uint8)


def test_end_to_end_straight_lines():
  cam = uh.fixture_camera("tiny_fisheye")
  rows, cols = [40.3, 75.2, 110.6], [50.4, 100.1, 150.7]
  img = checker_seen_by(cam, rows, cols)
  img2 = 255 - img
  out = camera_module.undistort_images([[img, img2]], [cam])
  assert len(out) == 1 and len(out[0]) == 2
  direct = undistort.undistort_images([cam], np.stack([img, img2]))
  assert np.array_equal(out[0][0], direct[0]) and np.array_equal(out[0][1], direct[1])
  assert np.array_equal(out[0][0], undistort.remap(img[None], cam.undistort_map)[0])
  # every projected edge is a straight line again: where a column of the result crosses mid-grey near row v0, it does so within 1 px
  und = out[0][0].astype(np.float64) - 127.5
  worst = 0.0
  for v0 in rows:
    lo = int(v0) - 4
    band = und[lo:lo + 10]
    for u in range(W):
      if min(abs(u - u0) for u0 in cols) < 4:
        continue
      flips = np.nonzero(band[:-1, u] * band[1:, u] < 0)[0]
      assert len(flips) == 1, (v0, u)
      r = flips[0]
      crossing = lo + r + band[r, u] / (band[r, u] - band[r + 1, u])
      worst = max(worst, abs(crossing - v0))
  print(f"largest distance of an undistorted edge from its line: {worst:.3f} px")
  assert worst <= 1.0
