"""TEST INFRASTRUCTURE: ctypes wrapper of tests/intrinsic_host (g++ build of multical_amd/csrc/mcba_intrinsic.h, the mathematics of
mcba_calibrate_intrinsics) behind tables.calibrate_intrinsics' signature, + the rigs the intrinsic tests share."""
import ctypes as C

import numpy as np

import host_build
from multical_amd import _lib, synthetic, tables
from multical_amd.structs import struct


_host = host_build.HostLib("intrinsic_host", "intrinsic", extra=dict(
    calibrate=[C.POINTER(_lib.IntrinsicProblem), _lib.c_double_p, _lib.c_double_p, _lib.c_double_p, _lib.c_int32_p, _lib.c_uint8_p,
               _lib.c_uint8_p, C.c_int32]))
lib, build = _host.lib, _host.build


def calibrate_intrinsics(point_table, boards, image_sizes, model='standard', fix_aspect=False, view_mask=None, init=None,
                         free_dist=None, max_iterations=0, device_order=False):
  """The host build behind tables.calibrate_intrinsics' signature; device_order: the device's summation order, not table order."""
  boards_pts = [np.asarray(getattr(b, "points", b)) for b in boards]
  valid = np.asarray(point_table.valid).astype(bool)
  if view_mask is None:
    view_mask = tables.min_detections_mask(valid, boards)
  inp = tables.IntrinsicInputs(point_table.points, valid, boards_pts, image_sizes, model, fix_aspect, view_mask, init, free_dist,
                               max_iterations)
  rc, out = inp.call(lib().intrinsic_calibrate, 1 if device_order else 0)
  _host.check(rc)
  return out


# ---- rigs and the restatement's view of them -----------------------------------------------------------------------------------
import intrinsic_reference as R          # noqa: E402
import pnp_host_lib                       # noqa: E402  (truth_chain, noise_free_points, pose_distance)

MODEL_OF = dict(standard='standard', rational='rational', thin_prism='thin_prism', tilted='tilted', fisheye='fisheye', pin4='pin4')
_rigs = {}


def rig(name, frames=16, outlier_frac=0.0, model=None):
  """synthetic.make_rig(name, frames, ...) with 0.2 px noise, cached; model: replace the configuration's camera model."""
  key = (name, frames, outlier_frac, model)
  if key not in _rigs:
    cfg = dict(synthetic.CONFIGS[name])
    if model is not None:
      cfg["model"] = model
    r = synthetic.make_rig(cfg, frames=frames, outlier_frac=outlier_frac)
    models = cfg["model"] if isinstance(cfg["model"], (list, tuple)) else [cfg["model"]] * cfg["cameras"]
    r.models = [MODEL_OF[m] for m in models]
    r.name = name
    r.image_sizes = [c.image_size for c in r.truth.cameras]
    _rigs[key] = r
  return _rigs[key]


def table_of(r, points=None, valid=None):
  return struct(points=r.points if points is None else points, valid=r.valid if valid is None else valid)


def camera_views(r, c, points=None, valid=None, view_mask=None):
  """[(frame, board)] and the restatement's views [(observed [n, 2], board points [n, 3])] of camera c: slots of 4 corners or more."""
  points, valid = r.points if points is None else points, r.valid if valid is None else valid
  slots, views = [], []
  for f in range(valid.shape[1]):
    for b in range(valid.shape[2]):
      v = valid[c, f, b]
      if v.sum() >= 4 and (view_mask is None or view_mask[c, f, b]):
        n = len(r.board_points[b])
        slots.append((f, b))
        views.append((points[c, f, b][v], np.asarray(r.board_points[b], dtype=np.float64)[v[:n]]))
  return slots, views


def truth_block(cam, fix_aspect=False):
  K = cam.intrinsic
  return np.concatenate([[K[0, 0], K[0, 0] if fix_aspect else K[1, 1], K[0, 2], K[1, 2], 0.0], np.asarray(cam.dist, dtype=np.float64)])


def truth_poses(r, c, slots):
  chain = pnp_host_lib.truth_chain(r)
  return np.array([R.pose_params(chain[c, f, b]) for f, b in slots])


def perturbed(block, poses, seed=0):
  """The second start of the well-posedness probe: focal + 1 %, poses perturbed by 1e-3."""
  rng = np.random.default_rng(seed)
  b = np.array(block, dtype=np.float64)
  b[:2] *= 1.01
  return b, poses + rng.normal(0, 1e-3, poses.shape)


def host_poses(out, c, slots):
  return np.array([R.pose_params(out.poses[c, f, b]) for f, b in slots])


def pose_gap(pa, pb):
  """(largest rotation angle [rad], largest translation difference) between two [V, 6] pose lists."""
  ang, tr = pnp_host_lib.pose_distance([R.pose_matrix(p) for p in pa], [R.pose_matrix(p) for p in pb])
  return float(ang.max()), float(tr.max())
