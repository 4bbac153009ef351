"""The undistortion mathematics (csrc/mcba_undistort.h) in its g++ build, against an independent numpy / scipy restatement
(undistort_reference.py), and the Python layer on top of it driven through that build.  No GPU."""
import pickle

import numpy as np
import pytest

from multical_amd import camera as camera_module
from multical_amd import undistort
from multical_amd.camera import Camera

import host_build
import undistort_host_lib as uh
import undistort_reference as ref

CAMERAS = list(zip(uh.CAMERA_IDS, uh.fixture_cameras()))
W, H = uh.IMAGE_SIZE
PX_TOL = 1e-9            # the project's fixed-x bar for pixels


def grid_pixels(step):
  u, v = np.meshgrid(np.arange(0, W, step, dtype=np.float64), np.arange(0, H, step, dtype=np.float64))
  return np.stack([u.ravel(), v.ravel()], axis=1)


def homogeneous_pixels(K, xy):
  return xy * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]


# ---- points ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cam", CAMERAS, ids=uh.CAMERA_IDS)
def test_inverse_round_trip(name, cam):
  """undistort_points(project(X)) = K X / z within 1e-9 px on the 40-px grid of the full-size image (4 px here): all 1 900 pixels of
  every fixture camera invert, so the status is asserted on every one."""
  px = grid_pixels(4)
  assert len(px) == 1900
  xy, status = uh.on_host(undistort.undistort_points, [cam], px)
  assert (status == undistort.UNDISTORT_OK).all()
  z = np.random.default_rng(3).uniform(0.5, 4.0, (len(px), 1))
  X = np.concatenate([xy * z, z], axis=1)
  uv = uh.on_host(undistort.project_points, [cam], X)
  err_forward = np.abs(uv - px).max()
  back, status = uh.on_host(undistort.undistort_points, [cam], uv, P=cam.intrinsic)
  assert (status == undistort.UNDISTORT_OK).all()
  err_back = np.abs(back - homogeneous_pixels(cam.intrinsic, X[:, :2] / z)).max()
  print(f"{name}: project(undistort(px)) - px {err_forward:.2e} px, undistort(project(X)) - K X/z {err_back:.2e} px")
  assert err_forward < PX_TOL and err_back < PX_TOL
  # the methods of the camera are the same calls
  with uh.host_backend():
    assert np.array_equal(cam.project(X.reshape(38, 50, 3)), uv.reshape(38, 50, 2))
    assert np.array_equal(cam.undistort_points(uv.reshape(38, 50, 2)), back.reshape(38, 50, 2))


@pytest.mark.parametrize("name,cam", CAMERAS, ids=uh.CAMERA_IDS)
def test_inverse_matches_restatement(name, cam):
  """project against the restated cv2 projection, and the inverse against scipy's least squares on it, within 1e-9 px"""
  rng = np.random.default_rng(5)
  X = np.concatenate([rng.uniform(-0.3, 0.3, (200, 2)), np.ones((200, 1))], axis=1) * rng.uniform(0.5, 3.0, (200, 1))
  assert np.abs(uh.on_host(undistort.project_points, [cam], X) - ref.project(cam, X)).max() < PX_TOL
  px = grid_pixels(20)
  R, P = uh.small_rotation(), uh.zoomed_out(cam)
  for kwargs in (dict(P=cam.intrinsic), dict(R=R, P=P), dict()):
    got, status = uh.on_host(undistort.undistort_points, [cam], px, **kwargs)
    want = ref.undistort_points(cam, px, **kwargs)
    scale = 1.0 if kwargs else cam.intrinsic[0, 0]      # (normalised output: the bar in pixels through the focal length)
    err = np.abs(got - want).max() * scale
    print(f"{name} {sorted(kwargs)}: {err:.2e} px")
    assert (status == undistort.UNDISTORT_OK).all() and err < PX_TOL


def test_points_mixed_cameras_and_errors():
  cams = [c for _, c in CAMERAS]
  rng = np.random.default_rng(7)
  of = rng.integers(0, len(cams), 300).astype(np.int32)
  X = np.concatenate([rng.uniform(-0.25, 0.25, (300, 2)), np.ones((300, 1))], axis=1)
  uv = uh.on_host(undistort.project_points, cams, X, of)
  for c, cam in enumerate(cams):
    assert np.abs(uv[of == c] - ref.project(cam, X[of == c])).max() < PX_TOL
  assert uh.on_host(undistort.project_points, cams, np.zeros((0, 3))).shape == (0, 2)
  with pytest.raises(RuntimeError, match="names camera"):
    uh.on_host(undistort.project_points, cams, X, np.full(300, len(cams)))
  bad = Camera(image_size=(W, H), intrinsic=cams[0].intrinsic, dist=np.zeros(6))
  with pytest.raises(RuntimeError, match="unsupported camera family"):
    uh.on_host(undistort.project_points, [bad], X)
  # a pixel the model cannot have produced: NaN and a status, not a guess
  # (an equidistant fisheye maps the half space in front of it into the disc of radius f pi / 2)
  fish = uh.fixture_camera("tiny_fisheye").copy(dist=np.zeros(4))
  out, status = uh.on_host(undistort.undistort_points, [fish], np.array([[100.0, 75.0], [5000.0, 4000.0]]))
  assert list(status) == [undistort.UNDISTORT_OK, undistort.UNDISTORT_NOT_CONVERGED]
  assert np.isfinite(out[0]).all() and np.isnan(out[1]).all()


# ---- maps --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cam", CAMERAS, ids=uh.CAMERA_IDS)
def test_maps_match_restatement(name, cam):
  """the map is float32(restated projectPoints(iR [u v 1])) within 1 ulp of the coordinate: P = K, a zoomed-out P (the only one that
  looks past the source) and a rotation of a few degrees"""
  for label, kwargs in (("P=K", dict()), ("zoomed out", dict(P=uh.zoomed_out(cam))),
                        ("rotated", dict(R=uh.small_rotation(), P=uh.zoomed_out(cam, 0.8)))):
    got = uh.on_host(undistort.undistort_maps, [cam], (W, H), **kwargs)[0]
    want = ref.undistort_map(cam, (W, H), **kwargs)
    assert got.shape == (H, W, 2) and got.dtype == np.float32
    d = uh.ulp_distance(got, want)
    inside = np.isfinite(got).all(axis=-1) & (got[..., 0] >= 0) & (got[..., 0] <= W - 1) & (got[..., 1] >= 0) & (got[..., 1] <= H - 1)
    print(f"{name} {label}: {int((d > 0).sum())} of {d.size} entries differ, at most {int(d.max())} ulp; "
          f"{inside.mean():.3f} of the pixels read inside the source")
    assert d.max() <= 1
    if label == "P=K":
      assert inside.all()
    if label == "zoomed out":
      assert not inside.all()


# ---- remap -------------------------------------------------------------------------------------------------------------------
def identity_map(h, w, dx=0.0, dy=0.0):
  u, v = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
  return np.stack([u + np.float32(dx), v + np.float32(dy)], axis=-1)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("channels", [1, 3])
def test_remap_identity_and_shift_are_exact(dtype, channels):
  """t = 0 gives the weights (0, 1, 0, 0) exactly: an identity map returns the image bit for bit, an integer shift the shifted
  image with the border value outside"""
  shape = (2, 37, 53) + ((3,) if channels == 3 else ())
  img = uh.noise_image(11, shape, dtype)
  out = uh.on_host(undistort.remap, img, identity_map(37, 53))
  assert out.dtype == img.dtype and out.tobytes() == img.tobytes()
  out = uh.on_host(undistort.remap, img, identity_map(37, 53, dx=5, dy=-3), border=9.0)
  want = np.full_like(img, 9)
  want[:, 3:, :48] = img[:, :34, 5:]
  assert out.tobytes() == want.tobytes()


def test_remap_float32_parity():
  """float32 noise 0 .. 255 against the float64 restatement: 2e-3 grey levels = 255 x 1.375^2 x 64 x 2^-24 (the largest sum of
  |weights| of this kernel is 1.375 an axis; 64 roundings is generous)"""
  hs, ws = 70, 130
  img = uh.noise_image(13, (hs, ws, 3), np.float32)
  maps = uh.random_maps(17, 2, 60, 90, hs, ws)
  for m in range(2):
    got = uh.on_host(undistort.remap, img[None], maps[m], border=3.5)[0]
    want = ref.remap(img, maps[m], border=3.5)
    err = np.abs(got - want).max()
    print(f"map {m}: max |float32 - float64| = {err:.2e} grey levels, values {want.min():.1f} .. {want.max():.1f}")
    assert err < 2e-3


@pytest.mark.parametrize("channels", [1, 3])
def test_remap_uint8_is_rounded_saturated_float32(channels):
  """the uint8 path is clamp(rint(.)) of the same build's float32 path, byte for byte; the noise overshoots both ends"""
  hs, ws = 70, 130
  img = uh.noise_image(19, (1, hs, ws) + ((3,) if channels == 3 else ()), np.uint8)
  maps = uh.random_maps(23, 1, 60, 90, hs, ws)
  got = uh.on_host(undistort.remap, img, maps)
  f = uh.on_host(undistort.remap, img.astype(np.float32), maps)
  print(f"float32 path: {f.min():.1f} .. {f.max():.1f}")
  assert f.min() < -1 and f.max() > 256
  assert got.dtype == np.uint8 and np.array_equal(got, np.clip(np.rint(f), 0, 255).astype(np.uint8))


def test_remap_edge_coordinates():
  """W - 1, -0.5, -2, W + 1, NaN, +-inf, +-1e30, ... on both axes give the value of the definition"""
  hs, ws = 9, 11
  img = uh.noise_image(29, (hs, ws), np.float32)
  ex, ey = uh.edge_coordinates(ws), uh.edge_coordinates(hs)
  maps = np.stack(np.meshgrid(ex, ey), axis=-1).astype(np.float32)          # [len(ey), len(ex), 2]: every pair
  got = uh.on_host(undistort.remap, img[None], maps, border=-7.0)[0]
  want = ref.remap(img, maps, border=-7.0)
  assert np.abs(got - want).max() < 2e-3
  dead = ~np.isfinite(maps).all(axis=-1) | (np.abs(maps) > 1e20).any(axis=-1) | (maps[..., 0] == -2.5) | (maps[..., 1] == -2.5)
  assert dead.sum() > 0 and (got[dead] == np.float32(-7.0)).all()               # exactly the border: no arithmetic
  got8 = uh.on_host(undistort.remap, np.rint(img).astype(np.uint8)[None], maps, border=200.0)[0]
  assert (got8[dead] == 200).all()


def test_remap_refuses_what_it_does_not_serve():
  maps = identity_map(4, 4)
  with pytest.raises(RuntimeError, match="channels"):
    uh.on_host(undistort.remap, np.zeros((1, 4, 4, 2), dtype=np.uint8), maps)
  with pytest.raises(TypeError, match="uint8 or float32"):
    uh.on_host(undistort.remap, np.zeros((1, 4, 4), dtype=np.uint16), maps)
  with pytest.raises(RuntimeError, match="names camera / map"):
    uh.on_host(undistort.remap, np.zeros((1, 4, 4), dtype=np.uint8), maps, map_of_image=[1])
  assert uh.on_host(undistort.remap, np.zeros((0, 4, 4), dtype=np.uint8), maps).shape == (0, 4, 4)


def test_sanitized_stand_alone_run(tmp_path):
  """the host build inside a small program of its own under AddressSanitizer + UBSan (CPU only): exact-size heap images, edge
  coordinates on both axes, every format -- no tap is read and no pixel stored out of bounds, no float -> int conversion overflows"""
  r = host_build.sanitized_program("undistort_host", "undistort_sanitize_main.cpp", tmp_path)
  assert r.returncode == 0 and "undistort sanitize run: ok" in r.stdout, r.stdout + r.stderr


# ---- fused form and the Python layer -------------------------------------------------------------------------------------------
def test_fused_equals_two_step_on_host():
  cams = [uh.fixture_camera("tiny_tilted"), uh.fixture_camera("tiny_fisheye")]
  img = uh.noise_image(31, (3, H, W), np.uint8)
  of = [1, 0, 1]
  for kwargs in (dict(), dict(P=np.stack([uh.zoomed_out(c) for c in cams]))):
    maps = uh.on_host(undistort.undistort_maps, cams, (W, H), **kwargs)
    two = uh.on_host(undistort.remap, img, maps, of)
    fused = uh.on_host(undistort.undistort_images, cams, img, of, **kwargs)
    assert fused.tobytes() == two.tobytes()


def test_camera_methods_and_pickle():
  cam = uh.fixture_camera("tiny_fisheye").copy()
  with uh.host_backend():
    m = cam.undistort_map
    assert m.shape == (H, W, 2) and m.dtype == np.float32
    assert cam.undistort_map is m                                   # cached
  assert np.array_equal(m, ref.undistort_map(cam, (W, H))) or uh.ulp_distance(m, ref.undistort_map(cam, (W, H))).max() <= 1
  state = cam.__getstate__()
  assert sorted(state) == ["dist", "fix_aspect", "has_skew", "image_size", "intrinsic", "model"]
  back = pickle.loads(pickle.dumps(cam))
  assert "undistort_map" not in back.__dict__ and type(back) is type(cam)
  for attr in ("project", "undistort_points", "undistort_map"):
    assert hasattr(Camera, attr)


def test_undistort_images_groups_by_size_and_splits_per_camera(monkeypatch):
  """one fused call per distinct image size; the result is a list per camera, in the order of the input"""
  a, b = uh.fixture_camera("tiny"), uh.fixture_camera("tiny_fisheye")
  small = uh.fixture_camera("tiny_rational").scale_image(0.5).copy(image_size=(100, 75))
  cams = [a, small, b]
  images = [[uh.noise_image(40 + i, (H, W), np.uint8) for i in range(2)],
            [uh.noise_image(50, (75, 100), np.uint8)],
            [uh.noise_image(60 + i, (H, W), np.uint8) for i in range(3)]]
  calls = []
  inner = undistort.undistort_images
  monkeypatch.setattr(undistort, "undistort_images", lambda cameras, imgs, **kw: calls.append((len(cameras), np.asarray(imgs).shape)) or
                      inner(cameras, imgs, **kw))
  with uh.host_backend():
    out = camera_module.undistort_images(images, cams, j=3, chunksize=2)
    assert sorted(calls) == [(1, (1, 75, 100)), (2, (5, H, W))]
    assert [len(o) for o in out] == [2, 1, 3]
    for cam, cam_images, cam_out in zip(cams, images, out):
      for image, result in zip(cam_images, cam_out):
        want = inner([cam], image[None])[0]
        assert result.shape == image.shape and result.dtype == np.uint8 and np.array_equal(result, want)
        assert np.array_equal(want, undistort.remap(image[None], cam.undistort_map)[0])
