"""TEST INFRASTRUCTURE: ctypes wrapper of tests/triangulate_host (g++ build of multical_amd/csrc/mcba_triangulate.h, the mathematics
of mcba_triangulate) + the converging rig the triangulation tests share.

The golden fisheye rigs are rings of cameras that do not overlap (tiny_fisheye: no corner is seen twice), so the tests synthesise
a rig of their own from undistort_host_lib.fixture_cameras(): 8 cameras of 200 x 150 of every family (4, 5, 8, 12 and 14
Brown-Conrady coefficients, two Kannala-Brandt cameras); camera c of a rig is fixture camera c % 8.

Observations are projected through undistort_reference.project, the restated cv2 projection: on seven of the eight cameras it is
multical_amd.synthetic._project to 3e-14 px, but synthetic._project has no tilt and lands 0.24 px away on the 14-coefficient camera,
which would put a model error of five times the noise into every point that camera sees.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
from scipy.spatial.transform import Rotation

import host_build
from multical_amd import _lib, synthetic, triangulate

import undistort_host_lib as uh
import undistort_reference as ref

HERE = host_build.HERE
NOISE_PX = 0.05
SHAPES = [(2, 1, 65, False), (3, 3, 65, False), (8, 2, 257, False), (8, 2, 130, True), (16, 1, 65, False)]   # C, F, M, rolling
SHAPE_IDS = ["2x1x65", "3x3x65", "8x2x257", "8x2x130-rolling", "16x1x65"]


_host = host_build.HostLib("triangulate_host", "th", ["triangulate"], module=triangulate)
lib, build, entry, host_backend, on_host = _host.lib, _host.build, _host.entry, _host.host_backend, _host.on_host


# ---- the converging rig ----------------------------------------------------------------------------------------------------
def rig_cameras(C):
  cams = uh.fixture_cameras()
  return [cams[c % len(cams)] for c in range(C)]


def header_round_trip(camera, uv):
  """[n] the header's Newton inverse takes the pixel back to itself within 1e-6 px (through the host build of the undistortion)"""
  xy, status = uh.on_host(uh.undistort.undistort_points, [camera], uv)
  ok = status == uh.undistort.UNDISTORT_OK
  back = ref.project(camera, np.concatenate([np.where(ok[:, None], xy, 0.0), np.ones((len(xy), 1))], axis=1))
  return ok & (np.abs(back - uv).max(axis=1) < 1e-6)


_rigs = {}


def make_rig(C, F, M, rolling=False, seed=1, noise=NOISE_PX):
  """struct of one synthetic call: cameras, camera_poses [C,4,4], rig_poses [F,4,4], rig_poses_end (rolling), views, views_end,
  truth [F,M,3], points [C,F,M,2], clean (the same without noise), valid [C,F,M].  Cached: the tests share it and leave it unchanged."""
  key = (C, F, M, rolling, seed, noise)
  if key in _rigs:
    return _rigs[key]
  rng = np.random.default_rng(seed)
  cameras = rig_cameras(C)
  camera_poses = np.zeros((C, 4, 4))
  for c in range(C):
    a = (c - (C - 1) / 2.0) * 0.12
    world_from_camera = np.eye(4)
    world_from_camera[:3, 3] = [a, rng.normal(0, 0.03), rng.normal(0, 0.03)]
    world_from_camera[:3, :3] = Rotation.from_euler("xyz", [rng.normal(0, 0.03), -0.6 * a + rng.normal(0, 0.03),
                                                            rng.normal(0, 0.05)]).as_matrix()
    camera_poses[c] = np.linalg.inv(world_from_camera)
  rig_poses = synthetic.to_matrix(rng.normal(0, 0.05, (F, 6)))
  rig_end = rig_poses @ synthetic.to_matrix(rng.normal(0, 5e-3, (F, 6))) if rolling else None
  truth = rng.uniform([-0.25, -0.2, 0.8], [0.25, 0.2, 2.0], (F, M, 3))
  views = triangulate.rig_views(camera_poses, rig_poses)
  views_end = triangulate.rig_views(camera_poses, rig_end) if rolling else None
  clean, valid = np.zeros((C, F, M, 2)), np.zeros((C, F, M), dtype=bool)
  for c, cam in enumerate(cameras):
    Xs = np.einsum('fij,fmj->fmi', views[c, :, :, :3], truth) + views[c, :, None, :, 3]
    Xc = Xs
    if rolling:
      Xe = np.einsum('fij,fmj->fmi', views_end[c, :, :, :3], truth) + views_end[c, :, None, :, 3]
      t = np.full((F, M, 1), 0.5)
      for _ in range(6):                                   # the observed row from six fixed-point passes
        Xc = (1.0 - t) * Xs + t * Xe
        t = ref.project(cam, Xc.reshape(-1, 3)).reshape(F, M, 2)[..., 1:] / cam.image_size[1]
      Xc = (1.0 - t) * Xs + t * Xe
    uv = ref.project(cam, Xc.reshape(-1, 3))
    w, h = cam.image_size
    inside = np.isfinite(uv).all(axis=1) & (uv[:, 0] >= 0) & (uv[:, 0] <= w - 1) & (uv[:, 1] >= 0) & (uv[:, 1] <= h - 1)
    ok = inside & (Xc.reshape(-1, 3)[:, 2] > 0.1)
    ok[ok] &= header_round_trip(cam, uv[ok])
    clean[c] = np.where(ok[:, None], uv, 0.0).reshape(F, M, 2)
    valid[c] = ok.reshape(F, M)
  valid &= rng.random((C, F, M)) < 0.8
  points = np.where(valid[..., None], clean + rng.normal(0, noise, clean.shape), 0.0)
  clean = np.where(valid[..., None], clean, 0.0)
  out = SimpleNamespace(cameras=cameras, camera_poses=camera_poses, rig_poses=rig_poses, rig_poses_end=rig_end, views=views,
                        views_end=views_end, truth=truth, points=points, clean=clean, valid=valid, shape=(C, F, M))
  _rigs[key] = out
  return out


def run(rig, backend=None, points=None, **kwargs):
  """triangulate the rig's table through the host build (backend=None) or through the library (backend="device")"""
  args = (rig.cameras, rig.views, rig.points if points is None else points, rig.valid)
  kw = dict(views_end=rig.views_end)
  kw.update(kwargs)
  if backend == "device":
    return triangulate.triangulate(*args, **kw)
  return on_host(triangulate.triangulate, *args, **kw)


def reference_problem(rig, points=None, **kwargs):
  import triangulate_reference as tr
  return tr.Problem(rig.cameras, rig.views, rig.points if points is None else points, rig.valid, views_end=rig.views_end, **kwargs)


# ---- the raw call (what the wrappers never send: NULL arrays, too many cameras) ------------------------------------------------
def raw_problem(rig, n_cameras=None):
  """(mcba_triangulate_problem, outputs dict, keep-alive list) of the rig's table; n_cameras: claim that many cameras (the camera
  blocks are repeated; the table arrays are NOT grown -- only for calls that are refused before anything is read)"""
  from multical_amd.undistort import CameraSetInputs
  cams = rig.cameras if n_cameras is None else [rig.cameras[c % len(rig.cameras)] for c in range(n_cameras)]
  inp = CameraSetInputs(cams)
  Cn, F, M = rig.shape
  views, points = np.ascontiguousarray(rig.views), np.ascontiguousarray(rig.points)
  valid = np.ascontiguousarray(rig.valid.astype(np.uint8))
  out = dict(X=np.zeros((F, M, 3)), status=np.zeros((F, M), dtype=np.uint8))
  p = _lib.TriangulateProblem()
  p.cams = inp.struct()
  p.F, p.M = F, M
  p.views, p.points, p.valid = _lib.dp(views), _lib.dp(points), _lib.up(valid)
  p.sigma_px, p.max_iterations = 0.0, 20
  return p, out, [inp, views, points, valid]


def raw_call(fn, p, out):
  """rc of fn(problem, X, NULL, NULL, NULL, NULL, status)"""
  return fn(C.byref(p), _lib.dp(out["X"]), None, None, None, None, _lib.up(out["status"]))


# ---- calibrations of the golden rigs with noise-free detections ------------------------------------------------------------------
def noise_free_table(rig):
  """(points [C,F,B,P,2], valid) of the golden rig re-synthesised without noise or outliers through synthetic._project at the slots
  the fixture observes -- through the ROLLING chain where the fixture has one (scan time from six fixed-point passes)"""
  tr = rig.truth
  Cn, F, B, P = rig.valid.shape
  padded = np.zeros((B, P, 3))
  for b, pts in enumerate(rig.board_points):
    padded[b, :len(pts)] = np.asarray(pts, dtype=np.float64)
  world = np.einsum('bij,bpj->bpi', tr.board_poses[:, :3, :3], padded) + tr.board_poses[:, None, :3, 3]
  rolling = rig.cfg["motion"] == "rolling"
  points = np.zeros((Cn, F, B, P, 2))
  for c in range(Cn):
    def local(rig_poses):
      T = tr.camera_poses[c][None] @ rig_poses
      return np.einsum('fij,bpj->fbpi', T[:, :3, :3], world) + T[:, None, None, :3, 3]
    Xs = local(tr.rig)
    Xc = Xs
    if rolling:
      Xe = local(tr.rig_end)
      t = np.full((F, B, P, 1), 0.5)
      for _ in range(6):
        t = synthetic._project(tr.cameras[c], (1.0 - t) * Xs + t * Xe)[..., 1:] / tr.cameras[c].image_size[1]
      Xc = (1.0 - t) * Xs + t * Xe
    points[c] = synthetic._project(tr.cameras[c], Xc)
  ok = rig.valid & np.isfinite(points).all(axis=-1)
  return np.where(ok[..., None], points, 0.0), ok


def truth_calibration(name, noise_free=True):
  """the golden rig `name` as a Calibration at its truth parameters, with its own detections or the noise-free ones"""
  import pnp_host_lib
  from multical_amd import calibration
  from multical_amd.structs import Table
  rig = pnp_host_lib.golden_rig(name)
  calib = calibration.from_rig(rig, "truth")
  if noise_free:
    points, ok = noise_free_table(rig)
    calib = calib.copy(point_table=Table.create(points=points, valid=ok))
  return calib
