"""TEST INFRASTRUCTURE: ctypes wrapper of tests/pnp_host (g++ build of multical_amd/csrc/mcba_pnp.h, the per-view pose
mathematics of mcba_view_poses) + the fixtures the pose-table tests share."""
import ctypes as C
import os

import numpy as np

import host_build
from multical_amd import _lib, synthetic, tables

HERE = host_build.HERE


_host = host_build.HostLib("pnp_host", "pnp", extra=dict(
    view_poses=[C.POINTER(_lib.ViewPoseProblem), _lib.c_double_p, _lib.c_double_p, _lib.c_int32_p, _lib.c_uint8_p, C.c_int32],
    undistort=[_lib.c_double_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, _lib.c_double_p]))
lib, build = _host.lib, _host.build


def view_poses(points, valid, board_points, cameras, view_mask=None, init_poses=None, max_iterations=0, pairwise=False):
  """The host build behind tables.view_poses' signature; pairwise: the device's reduction order instead of table order."""
  inp = tables.ViewPoseInputs(points, valid, board_points, cameras, view_mask, init_poses, max_iterations)
  poses, sse, n_used, status = inp.outputs()
  s = inp.struct()
  _host.check(lib().pnp_view_poses(C.byref(s), _lib.dp(poses), _lib.dp(sse), _lib.ip(n_used), _lib.up(status), 1 if pairwise else 0))
  return poses, sse, n_used, status, inp.lm_iterations


def undistort(camera, uv):
  """[n, 2] pixels -> ([n, 2] normalised points, [n] converged) through the header's Newton inversion."""
  block = np.ascontiguousarray(np.concatenate([[camera.intrinsic[0, 0], camera.intrinsic[1, 1], camera.intrinsic[0, 2],
                                                camera.intrinsic[1, 2], 0.0], np.asarray(camera.dist, dtype=np.float64)]))
  fish = 1 if tables._is_fisheye(camera) else 0
  out, ok = np.zeros((len(uv), 2)), np.zeros(len(uv), dtype=bool)
  xy = (C.c_double * 2)()
  for i, (u, v) in enumerate(np.asarray(uv, dtype=np.float64)):
    ok[i] = lib().pnp_undistort(_lib.dp(block), int(np.asarray(camera.dist).size), fish, 0, float(u), float(v), xy) != 0
    out[i] = xy[0], xy[1]
  return out, ok


# ---- fixtures ------------------------------------------------------------------------------------------------------------
FIXTURES = ["tiny", "tiny_pin4", "tiny_rational", "tiny_thin_prism", "tiny_tilted", "tiny_fisheye", "tiny_fishmix", "tiny_bigboard",
            "tiny_mixed", "cfg5_40", "tiny_edge"]
_rigs = {}


def golden_rig(name):
  """The fixture's rig (tests/golden/<name>.npz): detections with noise and outliers, truth poses and cameras."""
  if name not in _rigs:
    g = dict(np.load(os.path.join(HERE, "golden", f"{name}.npz"), allow_pickle=False))
    # (the reduced BASELINE configurations are stored as their results only: the rig is re-synthesised from the configuration's name)
    _rigs[name] = synthetic.rig_from_arrays(g) if "meta_json" in g else synthetic.make_rig(str(g["config"]))
  return _rigs[name]


def truth_chain(rig):
  tr = rig.truth
  return tr.camera_poses[:, None, None] @ tr.rig[None, :, None] @ tr.board_poses[None, None, :]


def noise_free_points(rig):
  """The rig's detections re-synthesised WITHOUT noise or outliers: the truth chain camera . rig . board projected through
  synthetic._project at the slots the fixture observes (static chain: a rolling-shutter fixture becomes its start pose)."""
  C_, F, B, P = rig.valid.shape
  chain = truth_chain(rig)
  padded = np.zeros((B, P, 3))
  for b, pts in enumerate(rig.board_points):
    padded[b, :len(pts)] = np.asarray(pts, dtype=np.float64)
  points = np.zeros((C_, F, B, P, 2))
  for c in range(C_):
    X = np.einsum('fbij,bpj->fbpi', chain[c, :, :, :3, :3], padded) + chain[c, :, :, None, :3, 3]
    points[c] = synthetic._project(rig.truth.cameras[c], X)
  ok = rig.valid & np.isfinite(points).all(axis=-1)
  return np.where(ok[..., None], points, 0.0), ok


def pose_distance(a, b):
  """(rotation angle of a^-1 b [rad], translation difference [m]) per pose."""
  from scipy.spatial.transform import Rotation
  a, b = np.asarray(a).reshape(-1, 4, 4), np.asarray(b).reshape(-1, 4, 4)
  rel = np.swapaxes(a[:, :3, :3], -1, -2) @ b[:, :3, :3]
  ang = np.linalg.norm(Rotation.from_matrix(rel).as_rotvec(), axis=1)
  return ang, np.linalg.norm(a[:, :3, 3] - b[:, :3, 3], axis=1)
