"""TEST INFRASTRUCTURE: ctypes wrapper of tests/stereo_host (g++ build of multical_amd/csrc/mcba_stereo.h, the mathematics of
mcba_stereo_calibrate) + the cases the stereo tests share.

A case is a synthetic rig (multical_amd.synthetic.make_rig) at its TRUTH cameras with the start poses of every view from the host
build of the pose-table mathematics (pnp_host_lib.view_poses), so the same inputs reach the host build and the device and no test
of the host build needs a GPU.
"""
import contextlib
import ctypes as C
from types import SimpleNamespace

import numpy as np

import host_build
import pnp_host_lib
from multical_amd import stereo, synthetic

_host = host_build.HostLib("stereo_host", "sh", ["stereo_calibrate"], module=stereo, extra=dict(set_device_order=[C.c_int32]))
lib, build, entry, host_backend, on_host = _host.lib, _host.build, _host.entry, _host.host_backend, _host.on_host

_cases = {}


def make_case(name, frames=None, noise_free=False, noise=0.2, outlier_frac=0.01):
  """SimpleNamespace(cameras, board_points [list], points [C,F,B,P,2], valid, view_poses [C,F,B,4,4], view_valid, camera_poses
  (truth), rig).  noise_free: the static truth chain projected at the slots the rig observes.  Cached: the tests share it and leave
  it unchanged."""
  key = (name, frames, noise_free, noise, outlier_frac)
  if key in _cases:
    return _cases[key]
  rig = synthetic.make_rig(name, frames=frames, noise=noise, outlier_frac=outlier_frac)
  points, valid = pnp_host_lib.noise_free_points(rig) if noise_free else (rig.points, rig.valid)
  cameras = rig.truth.cameras
  board_points = [np.asarray(b, dtype=np.float64) for b in rig.board_points]
  poses, _, _, status, _ = pnp_host_lib.view_poses(points, valid, board_points, cameras)
  out = SimpleNamespace(name=name, cameras=cameras, board_points=board_points, points=points, valid=np.asarray(valid).astype(bool),
                        view_poses=poses, view_valid=status == 0, camera_poses=rig.truth.camera_poses, rig=rig)
  _cases[key] = out
  return out


def with_tables(case, **changes):
  out = SimpleNamespace(**vars(case))
  for k, v in changes.items():
    setattr(out, k, v)
  return out


def all_pairs(case):
  n = len(case.cameras)
  return [(i, j) for i in range(n) for j in range(i + 1, n)]


def truth_relative(case, i, j):
  """left-camera frame -> right-camera frame of the truth"""
  return case.camera_poses[j] @ np.linalg.inv(case.camera_poses[i])


def common_counts(case, i, j, min_common=4):
  """(views, points) of pair (i, j) as the plan counts them"""
  n = (case.valid[i] & case.valid[j]).sum(axis=-1)
  use = (n >= min_common) & case.view_valid[i] & case.view_valid[j]
  return int(use.sum()), int(n[use].sum())


@contextlib.contextmanager
def device_order(on=True):
  _host.check(lib().sh_set_device_order(1 if on else 0))
  try:
    yield
  finally:
    _host.check(lib().sh_set_device_order(0))


def run(case, pairs=None, backend=None, order=False, **kwargs):
  """stereo.calibrate_pairs on the case through the host build (backend=None; order: the device's summation order) or through the
  library (backend="device")"""
  pairs = all_pairs(case) if pairs is None else pairs
  args = (case.cameras, case.board_points, case.points, case.valid, case.view_poses, case.view_valid, pairs)
  if backend == "device":
    return stereo.calibrate_pairs(*args, **kwargs)
  with device_order(order):
    return on_host(stereo.calibrate_pairs, *args, **kwargs)


def params(T):
  """[n, 6] global rotation vector | translation of [n, 4, 4]"""
  from scipy.spatial.transform import Rotation
  T = np.asarray(T).reshape(-1, 4, 4)
  return np.concatenate([Rotation.from_matrix(T[:, :3, :3]).as_rotvec(), T[:, :3, 3]], axis=1)


def pose_gap(a, b):
  """max of rotation angle [rad] and translation difference [m] between two poses"""
  ang, d = pnp_host_lib.pose_distance(a, b)
  return float(max(ang.max(), d.max()))


def wide_case(angle_deg, draws, noise=0.2, views=10, seed=7):
  """`draws` independent noisy copies of ONE two-camera rig whose cameras are angle_deg apart, as cameras (2 k, 2 k + 1) of one
  table [2 draws, views, 1, 81]: both look at a board about 1.2 m away, from angle_deg / 2 to either side of its normal (every corner
  is kept: the cost does not ask which side of the board a camera sees).  Start poses: the truth.  Returns (case, T_rel)."""
  from scipy.spatial.transform import Rotation
  base = make_case("tiny", frames=16)
  rng = np.random.default_rng(seed)
  board = base.board_points[0]
  centre, c = board.mean(axis=0), np.array([0.0, 0.0, 1.2])
  half = np.deg2rad(angle_deg) / 2.0
  T_rel = np.eye(4)
  T_rel[:3, :3] = Rotation.from_rotvec([0.02, -2.0 * half, 0.03]).as_matrix()
  T_rel[:3, 3] = c - T_rel[:3, :3] @ c + [0.01, -0.02, 0.03]
  left = np.tile(np.eye(4), (views, 1, 1))
  for v in range(views):
    R = (Rotation.from_rotvec([0.0, half, 0.0]) * Rotation.from_rotvec(rng.normal(0, 0.2, 3))).as_matrix()
    left[v, :3, :3] = R
    left[v, :3, 3] = c + rng.normal(0, 0.05, 3) - R @ centre
  right = T_rel @ left
  cams = [base.cameras[0], base.cameras[1]]
  clean = np.stack([synthetic._project(cams[s], board @ T[:, :3, :3].transpose(0, 2, 1) + T[:, None, :3, 3])
                    for s, T in enumerate((left, right))])                                  # [2, views, 81, 2]
  assert np.isfinite(clean).all()
  points = np.tile(clean[:, :, None], (draws, 1, 1, 1, 1)) + rng.normal(0, noise, (2 * draws, views, 1, len(board), 2))
  poses = np.tile(np.stack([left, right])[:, :, None], (draws, 1, 1, 1, 1))
  case = SimpleNamespace(name=f"wide{angle_deg}", cameras=cams * draws, board_points=[board], points=points,
                         valid=np.ones(points.shape[:4], dtype=bool), view_poses=poses, view_valid=np.ones(points.shape[:3], dtype=bool),
                         camera_poses=None, rig=None)
  return case, T_rel
