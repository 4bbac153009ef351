"""calibration.json -> cameras and camera poses: the reader of what multical_amd.export writes (multical's export format, FORMAT.md).

Written against the file, not against a module of the reference (which builds its own classes from it):

  cameras       {name: {model, image_size [w, h], K [3, 3], dist [..]}}
  camera_poses  {name: {R [3, 3], T [3]}}            an absolute pose, rig -> camera
                {"a_to_b": {R, T}}                   a relative pose M = T_a T_b^-1 (what export_relative writes for a master b: the
                                                     calibration re-gauged so that b sits at the origin): T_a = M T_b, T_b = M^-1 T_a

Poses are propagated over the graph of relative entries from every absolute one.  A product with an exact identity is not formed (it
is the factor itself), so a file written with a master at the exact origin comes back bit for bit.  The file does not say whether a
camera is a Kannala-Brandt fisheye: `fisheye` names those that are (default: a camera whose model is "fisheye" or one of the
fisheye-only "fix_k*" names).
"""
import json

import numpy as np

from .camera import Camera, CameraFisheye
from .structs import struct

LOOP_TOLERANCE = 1e-8       # two routes to one camera agree to this (entries of the 4 x 4 matrix)


def import_camera(data, fisheye=None):
  """One entry of `cameras`"""
  model = data.get("model", "standard")
  if fisheye is None:
    fisheye = model == "fisheye" or model.startswith("fix_k")
  K, dist = np.array(data["K"], dtype=np.float64), np.array(data["dist"], dtype=np.float64)
  size = tuple(int(v) for v in data["image_size"])
  if fisheye:
    return CameraFisheye(size, K, dist, model=model if model in CameraFisheye.model_names else "standard")
  return Camera(size, K, dist, model=model)


def import_transform(data):
  """{R, T} -> [4, 4]"""
  M = np.eye(4)
  M[:3, :3] = np.array(data["R"], dtype=np.float64)
  M[:3, 3] = np.array(data["T"], dtype=np.float64).reshape(3)
  return M


def _times(A, B):
  """A B, with an exact identity taken as it is"""
  eye = np.eye(4)
  if np.array_equal(B, eye):
    return A.copy()
  if np.array_equal(A, eye):
    return B.copy()
  return A @ B


def import_camera_poses(data, names):
  """{name: [4, 4]} for every camera of `names` from the entries of `camera_poses`"""
  names = list(names)
  known, relative = {}, {}
  for key, value in data.items():
    M = import_transform(value)
    if key in names:
      known[key] = M
      continue
    ends = [(a, b) for a in names for b in names if key == f"{a}_to_{b}"]
    if len(ends) != 1:
      raise ValueError(f"import_calib: camera pose entry {key!r} names no camera of {names}")
    a, b = ends[0]
    relative.setdefault(b, []).append((a, M, False))          # T_a = M T_b
    relative.setdefault(a, []).append((b, M, True))           # T_b = M^-1 T_a
  poses, queue = {}, list(known.items())
  while queue:
    name, T = queue.pop(0)
    if name in poses:
      if not np.allclose(T, poses[name], rtol=0.0, atol=LOOP_TOLERANCE):
        raise ValueError(f"import_calib: inconsistent camera poses: two routes to {name!r} differ by "
                         f"{np.abs(T - poses[name]).max():.3g}")
      continue
    poses[name] = T
    for other, M, inverse in relative.get(name, []):
      queue.append((other, _times(np.linalg.inv(M), T) if inverse else _times(M, T)))
  missing = [n for n in names if n not in poses]
  if missing:
    raise ValueError(f"import_calib: no camera pose for {missing}: neither an absolute entry nor a chain of relative entries to one")
  return poses


def import_cameras(data, fisheye=None):
  """The cameras and camera poses of a decoded calibration.json: struct(names, cameras (Camera / CameraFisheye), camera_poses
  [C, 4, 4] rig -> camera, in the order of the file; correction (a correction.FieldCorrection) if the file has a
  `residual_correction` block).  fisheye: names (or a dict name -> bool) of the Kannala-Brandt cameras."""
  names = list(data["cameras"].keys())
  if fisheye is not None and not isinstance(fisheye, dict):
    fisheye = {n: n in set(fisheye) for n in names}
  cameras = [import_camera(data["cameras"][n], None if fisheye is None else bool(fisheye.get(n, False))) for n in names]
  poses = import_camera_poses(data.get("camera_poses", {}), names)
  out = struct(names=names, cameras=cameras, camera_poses=np.stack([poses[n] for n in names]))
  if "residual_correction" in data:       # (written by multical_amd.export for a corrected calibration only: `correction` is absent else)
    from .correction import FieldCorrection
    block = data["residual_correction"]
    if list(block.get("cameras", names)) != names:
      raise ValueError(f"import_calib: the residual correction is for cameras {block['cameras']}, the file has {names}")
    out = out._extend(correction=FieldCorrection.from_dict(block))
  return out


def load_calibration(filename, fisheye=None):
  """import_cameras of a calibration.json file"""
  with open(filename) as f:
    return import_cameras(json.load(f), fisheye)
