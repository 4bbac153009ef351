"""TEST INFRASTRUCTURE: ctypes wrapper of tests/recon_host (g++ build of multical_amd/csrc/mcba_recon.h, the mathematics of
mcba_reconstruction_uncertainty) + the converging rigs the reconstruction-uncertainty tests share: the nine cameras of
uncertainty_host_lib (4, 5, 8, 12, 14-tilted Brown-Conrady, fisheye, the mixed pair, the 5-coefficient camera under fix_aspect),
200 x 150 pixels, dealt to the slots of a group 12 cm apart and toed in, as triangulate_host_lib places them."""
import ctypes as C
import os
import subprocess

import numpy as np
from scipy.spatial.transform import Rotation

import host_build
from multical_amd import _lib, guidance, reconstruction, transform, uncertainty
from multical_amd.undistort import CameraSetInputs

import uncertainty_host_lib as ul

_ROWS = [C.POINTER(_lib.CameraSet), _lib.c_double_p, C.POINTER(_lib.ReconJob), _lib.c_double_p, C.c_uint64, C.c_double, _lib.c_double_p,
         C.POINTER(C.c_int32)]
_host = host_build.HostLib("recon_host", "rch", ["reconstruction_uncertainty"], extra=dict(query_rows=_ROWS), module=reconstruction)
lib, build, entry, host_backend, on_host = _host.lib, _host.build, _host.entry, _host.host_backend, _host.on_host
CAMERA_IDS = list(ul.uh.CAMERA_IDS) + ["tiny-0-fix_aspect"]
SPACING = 0.12
ALL = ~np.uint64(0)
_rigs = {}


def fast_entry():
  """the -ffp-contract=fast build, in a library of its own name: what stands in for reconstruction._entry"""
  path = os.path.join(host_build.HERE, "recon_host", "_build", "libmcba_recon_host_fast.so")
  src = os.path.join(host_build.HERE, "recon_host", "recon_host.cpp")
  lib()
  if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(host_build.path("recon_host")):
    subprocess.check_call(["g++"] + host_build.BASE_FLAGS + ["-ffp-contract=fast", "-mfma", "-shared", "-o", path, src])
  h = C.CDLL(path)
  fn = h.rch_reconstruction_uncertainty
  fn.restype, fn.argtypes = C.c_int32, dict((n, a) for n, _, a in _lib.SYMBOLS)["mcba_reconstruction_uncertainty"]
  h.rch_last_error.restype = C.c_char_p

  def call(name):
    def run(*args):
      if fn(*args) != 0:
        raise RuntimeError(h.rch_last_error().decode())
    return run
  return call


def group_rig(first, G, seed=3, members=None):
  """(RigModel, source cameras) of the G cameras first, first + 1, .. (mod 9) of the nine -- or of `members` --, slot s at
  (s - (G - 1) / 2) x 12 cm along x and toed in (shared, unchanged by the tests)"""
  key = (first, G, seed, members)
  if key not in _rigs:
    ul.rig()
    nine = ul.source_cameras()
    cams = [nine[(first + s) % len(nine)] for s in range(G)] if members is None else [nine[c] for c in members]
    rng = np.random.default_rng(seed + 10 * first + G)
    poses = np.zeros((G, 4, 4))
    for s in range(G):
      a = (s - (G - 1) / 2.0) * SPACING
      rig_from_camera = np.eye(4)
      rig_from_camera[:3, 3] = [a, rng.normal(0, 0.02), rng.normal(0, 0.02)]
      rig_from_camera[:3, :3] = Rotation.from_euler("xyz", [rng.normal(0, 0.03), -0.1 * a + rng.normal(0, 0.02), rng.normal(0, 0.05)]).as_matrix()
      poses[s] = np.linalg.inv(rig_from_camera)
    rt = transform.from_matrix(poses).reshape(-1, 6)
    _rigs[key] = (uncertainty.RigModel(cams, transform.to_matrix(rt), rt), cams)
  return _rigs[key]


def stored_maps(model):
  """[M_c [24, 5 + nd + 6]]: the device columns of every camera from its stored block (camera | pose)"""
  return [guidance.rig_device_factor(model, c, np.eye(5 + model.n_dist[c] + 6))[0] for c in range(len(model.cameras))]


def random_factors(model, r, seed, scale=1e-4):
  """factors[c] = (W_c [24, r], False) = M_c F_c of a random factor F over the stored parameters, and F [p, r]"""
  rng = np.random.default_rng(seed)
  maps = stored_maps(model)
  F = [scale * rng.normal(size=(M.shape[1], r)) for M in maps]
  return [(M @ f, False) for M, f in zip(maps, F)], np.concatenate(F) if F else np.zeros((0, r))


def factors_of(model, F):
  """factors from a factor F [p, r] over the stored parameters (camera | pose per slot)"""
  out, at = [], 0
  for M in stored_maps(model):
    out.append((M @ F[at:at + M.shape[1]], False))
    at += M.shape[1]
  return out


def _job_record(model, reference, margin):
  G = len(model.cameras)
  job = _lib.ReconJob()
  job.G, job.reference, job.r, job.n = G, -1 if reference is None else reference, 0, 0
  for s in range(G):
    job.cameras[s] = s
    job.image_w[s], job.image_h[s] = [float(x) for x in model.cameras[s].image_size]
  return job


def query_rows(model, reference, X, mask=ALL, margin=0.0):
  """(G [3, 24 G] of the point X over the device columns, status)"""
  inp = CameraSetInputs(model.cameras)
  cs = inp.struct()
  job = _job_record(model, reference, margin)
  poses = np.ascontiguousarray(model.poses[:, :3, :])
  X = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
  out, st = np.zeros((3, 24 * len(model.cameras))), C.c_int32()
  _host.check(lib().rch_query_rows(C.byref(cs), _lib.dp(poses), C.byref(job), _lib.dp(X), int(mask), float(margin), _lib.dp(out), C.byref(st)))
  return out, st.value


def stored_rows(model, reference, X, mask=ALL, margin=0.0):
  """(J [3, p] over the STORED parameters -- the header's columns times the stored maps --, status)"""
  Gm, status = query_rows(model, reference, X, mask, margin)
  maps = stored_maps(model)
  return np.concatenate([Gm[:, 24 * c:24 * c + 24] @ M for c, M in enumerate(maps)], axis=1), status


def run(model, jobs, sigma2=1.0, margin=0.0, backend=None):
  """the raw outputs through the host build (None), its contracted twin ("fast") or the library ("device")"""
  args = (model.cameras, model.poses, jobs, sigma2, margin)
  if backend == "device":
    return reconstruction.run_jobs(*args)
  if backend == "fast":
    saved = reconstruction._entry
    reconstruction._entry = fast_entry()
    try:
      return reconstruction.run_jobs(*args)
    finally:
      reconstruction._entry = saved
  return on_host(reconstruction.run_jobs, *args)


def job_of(model, reference, factors, points, masks=None):
  return reconstruction.Job(list(range(len(model.cameras))), reference, factors, points, masks)


def field_points(model, distances=(0.12, 1.2)):
  """[2 len(distances), 3] in the rig frame: on the axis of the group and towards the edge of the common field (16 degrees up), at the
  distances (metres from the rig origin, which lies between the cameras)"""
  out = []
  for d in distances:
    out += [[0.0, 0.0, d], [0.02 * d, 0.29 * d, d]]
  return np.array(out)


def whitened_difference(got, want):
  """|L^-1 (C_got - C_want) L^-T|_F per point with L L^T = C_want, [n, 3, 3] blocks; a direction whose variance is below 1e-6 of the
  largest one is whitened by that floor; 0 where both are NaN"""
  out = np.zeros(len(want))
  for i, (g, w) in enumerate(zip(got, want)):
    if not np.isfinite(w).all():
      out[i] = 0.0 if not np.isfinite(g).any() else np.inf
      continue
    lam, V = np.linalg.eigh(w)
    if lam.max() <= 0.0:
      out[i] = 0.0 if np.array_equal(g, w) else np.inf
      continue
    s = 1.0 / np.sqrt(np.maximum(lam, max(1e-6 * lam.max(), 1e-300)))
    Li = (V * s).T
    out[i] = np.linalg.norm(Li @ (g - w) @ Li.T)
  return out


def stored_steps(model):
  """[p] the scale of every stored parameter (camera | pose per slot): the steps of the restatement's differences"""
  import reconstruction_uncertainty_reference as rr
  return np.concatenate([rr.slot_steps(n) for n in model.n_dist])


def meaning_case(d=1.5):
  """(model, factors, points [2, 3], reference): the two-camera group, a covariance of every stored parameter scaled by its step
  (camera 0's pose held, no skew), and the points at d and 2 d on the optical axis of camera 0"""
  m, _ = group_rig(0, 2)
  steps = stored_steps(m)
  p = len(steps)
  sigma = 1e-6 * ul.random_spd(p, 31, 1.0) * np.outer(steps, steps) / steps.max() ** 2
  dead = [4, 5 + m.n_dist[0] + 6 + 4] + list(range(5 + m.n_dist[0], 5 + m.n_dist[0] + 6))
  sigma[dead, :] = 0.0
  sigma[:, dead] = 0.0
  T = np.linalg.inv(m.poses[0])
  pts = np.array([T[:3, :3] @ [0.0, 0.0, k * d] + T[:3, 3] for k in (1.0, 2.0)])
  return m, factors_of(m, uncertainty.factor(sigma)), pts, 0


def range_lateral(model, reference, out, pts):
  """(range_std, lateral_std) of the calibration part of raw outputs"""
  res = reconstruction.finish(out, model.poses, reference, pts, 0)
  return res.range_std_cal, res.lateral_std_cal
