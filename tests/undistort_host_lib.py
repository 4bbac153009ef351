"""TEST INFRASTRUCTURE: ctypes wrapper of tests/undistort_host (g++ build of multical_amd/csrc/mcba_undistort.h, the mathematics of
the undistortion entry points) + the fixtures the undistortion tests share."""
import numpy as np

import host_build
from multical_amd import undistort
from multical_amd.camera import Camera, CameraFisheye

import pnp_host_lib

HERE = host_build.HERE
NAMES = ["project_points", "undistort_points", "undistort_maps", "remap", "undistort_images"]


_host = host_build.HostLib("undistort_host", "uh", NAMES, module=undistort)
lib, build, entry, host_backend, on_host = _host.lib, _host.build, _host.entry, _host.host_backend, _host.on_host


# ---- fixtures ------------------------------------------------------------------------------------------------------------
# (fixture, camera): 4, 5, 8, 12 and 14 Brown-Conrady coefficients, two Kannala-Brandt cameras
CAMERA_FIXTURES = [("tiny", 0), ("tiny_pin4", 0), ("tiny_rational", 0), ("tiny_thin_prism", 0), ("tiny_tilted", 0), ("tiny_fisheye", 0),
                   ("tiny_fishmix", 0), ("tiny_fishmix", 1)]
CAMERA_IDS = [f"{name}-{c}" for name, c in CAMERA_FIXTURES]
SCALE, IMAGE_SIZE = 0.1, (200, 150)
_cameras = {}


def fixture_camera(name, index=0):
  """Truth camera `index` of the golden rig, scaled to 200 x 150 (the distortion is unchanged: it acts on normalised points)."""
  key = (name, index)
  if key not in _cameras:
    t = pnp_host_lib.golden_rig(name).truth.cameras[index]
    cls = CameraFisheye if t.model == "fisheye" else Camera
    cam = cls(image_size=t.image_size, intrinsic=t.intrinsic, dist=t.dist, model="standard" if t.model == "fisheye" else t.model)
    _cameras[key] = cam.scale_image(SCALE).copy(image_size=IMAGE_SIZE)
  return _cameras[key]


def fixture_cameras():
  return [fixture_camera(*k) for k in CAMERA_FIXTURES]


def zoomed_out(camera, factor=0.5):
  """the camera's matrix with factor x the focal lengths: the undistorted image looks past the edge of the source"""
  P = np.array(camera.intrinsic, dtype=np.float64)
  P[0, 0] *= factor
  P[1, 1] *= factor
  return P


def small_rotation(deg=(3.0, -2.0, 1.5)):
  from scipy.spatial.transform import Rotation
  return Rotation.from_euler("xyz", deg, degrees=True).as_matrix()


def noise_image(seed, shape, dtype=np.float32):
  """uniform noise 0 .. 255: the strongest gradients an image can have, so the bicubic overshoot reaches both saturations"""
  rng = np.random.default_rng(seed)
  img = rng.uniform(0.0, 255.0, shape)
  return np.rint(img).astype(np.uint8) if dtype == np.uint8 else img.astype(np.float32)


def edge_coordinates(w):
  """the coordinates every remap test covers on an axis of w pixels"""
  return np.array([w - 1.0, -0.5, -0.25, -2.0, w + 1.0, np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, w - 0.5, -1.0, w + 0.0, -2.5,
                   w + 0.999], dtype=np.float32)


def random_maps(seed, M, hd, wd, hs, ws):
  """[M, hd, wd, 2] float32: coordinates around the source (some outside), with every pair of edge coordinates planted"""
  rng = np.random.default_rng(seed)
  maps = np.stack([rng.uniform(-4.0, ws + 3.0, (M, hd, wd)), rng.uniform(-4.0, hs + 3.0, (M, hd, wd))], axis=-1).astype(np.float32)
  ex, ey = edge_coordinates(ws), edge_coordinates(hs)
  pairs = np.array([(x, y) for x in ex for y in (ey[0], ey[1], ey[5], 3.25)] + [(7.5, y) for y in ey], dtype=np.float32)
  flat = maps.reshape(M, -1, 2)
  n = min(len(pairs), flat.shape[1])
  for m in range(M):
    where = rng.choice(flat.shape[1], n, replace=False)
    flat[m, where] = pairs[rng.permutation(len(pairs))[:n]]
  return flat.reshape(M, hd, wd, 2)


def ulp_distance(a, b):
  """distance of float32 arrays in units in the last place (NaN matches NaN)"""
  a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
  both_nan = np.isnan(a) & np.isnan(b)

  def ordered(x):
    i = x.view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)
  d = np.abs(ordered(a) - ordered(b))
  return np.where(both_nan, 0, np.where(np.isnan(a) | np.isnan(b), 1 << 40, d))
