"""TEST INFRASTRUCTURE: ctypes wrapper of tests/uncertainty_host (g++ build of multical_amd/csrc/mcba_uncertainty.h, the mathematics
of mcba_projection_uncertainty) + the rig the projection-uncertainty tests share: the eight cameras of
undistort_host_lib.CAMERA_FIXTURES (4, 5, 8, 12, 14-tilted Brown-Conrady, fisheye, the mixed pair) and a ninth, the 5-coefficient
camera under fix_aspect, on an arc; 200 x 150 pixels."""
import ctypes as C

import numpy as np

import host_build
from multical_amd import _lib, transform, uncertainty

import undistort_host_lib as uh

_host = host_build.HostLib("uncertainty_host", "unh", ["projection_uncertainty"], extra=dict(
    query_rows=[C.POINTER(_lib.CameraSet), _lib.c_double_p, C.POINTER(_lib.UncertaintyJob), C.c_double, C.c_double, _lib.c_double_p,
                C.POINTER(C.c_int32)]), module=uncertainty)
lib, build, entry, host_backend, on_host = _host.lib, _host.build, _host.entry, _host.host_backend, _host.on_host
FIX_ASPECT = 8                   # index of the fix_aspect camera
W_IMG, H_IMG = uh.IMAGE_SIZE
_rig = []


def fast_lib():
  """the -ffp-contract=fast build, in a library of its own name"""
  import os
  import subprocess
  path = os.path.join(host_build.HERE, "uncertainty_host", "_build", "libmcba_uncertainty_host_fast.so")
  src = os.path.join(host_build.HERE, "uncertainty_host", "uncertainty_host.cpp")
  if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(host_build.path("uncertainty_host")):
    lib()
    subprocess.check_call(["g++"] + host_build.BASE_FLAGS + ["-ffp-contract=fast", "-mfma", "-shared", "-o", path, src])
  h = C.CDLL(path)
  fn = h.unh_projection_uncertainty
  fn.restype, fn.argtypes = C.c_int32, dict((n, a) for n, _, a in _lib.SYMBOLS)["mcba_projection_uncertainty"]
  h.unh_last_error.restype = C.c_char_p

  def call(name):
    def run(*args):
      if fn(*args) != 0:
        raise RuntimeError(h.unh_last_error().decode())
    return run
  return call


def on_fast(fn, *args, **kwargs):
  saved = uncertainty._entry
  uncertainty._entry = fast_lib()
  try:
    return fn(*args, **kwargs)
  finally:
    uncertainty._entry = saved


def rig():
  """RigModel of the nine cameras (shared, unchanged by the tests)"""
  if not _rig:
    cams = uh.fixture_cameras()
    cams.append(cams[0].copy(fix_aspect=True))
    rng = np.random.default_rng(7)
    rt = np.zeros((len(cams), 6))
    for c in range(len(cams)):
      a = (c - 4) * 0.1
      rt[c] = [rng.normal(0, 0.05), -0.4 * a + rng.normal(0, 0.03), rng.normal(0, 0.08), -a + rng.normal(0, 0.02), rng.normal(0, 0.03),
               rng.normal(0, 0.03)]
    rt[0, :3] = 0.0                                   # (an identity rotation: the series branch of the left Jacobian)
    _rig.append(uncertainty.RigModel(cams, transform.to_matrix(rt), rt))
    _rig.append(cams)
  return _rig[0]


def source_cameras():
  rig()
  return _rig[1]


def edge_pixels():
  """centre, the four edges and the four corners of the image"""
  w, h = W_IMG - 1.0, H_IMG - 1.0
  return np.array([[w / 2, h / 2], [0, h / 2], [w, h / 2], [w / 2, 0], [w / 2, h], [0, 0], [w, 0], [0, h], [w, h]], dtype=np.float64)


def random_spd(p, seed, scale=1e-6):
  rng = np.random.default_rng(seed)
  A = rng.normal(size=(p, p))
  return scale * (A @ A.T + 0.1 * np.eye(p))


def query_rows(model, b, a, rho, uv):
  """(J [n, 2, p] over the STORED parameters of the job -- the header's columns times RigModel.stored_map --, status [n])"""
  from multical_amd.undistort import CameraSetInputs
  inp = CameraSetInputs(model.cameras)
  cs = inp.struct()
  M = model.stored_map(b, a)
  job = _lib.UncertaintyJob()
  job.camera, job.reference, job.inv_distance, job.K, job.r = b, -1 if a is None else a, rho, M.shape[0], 0
  uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
  J, status = np.zeros((len(uv), 2, M.shape[1])), np.zeros(len(uv), dtype=np.int32)
  buf, st = np.zeros((2, M.shape[0])), C.c_int32()
  for i, (u, v) in enumerate(uv):
    _host.check(lib().unh_query_rows(C.byref(cs), _lib.dp(model.poses), C.byref(job), float(u), float(v), _lib.dp(buf), C.byref(st)))
    J[i], status[i] = buf @ M, st.value
  return J, status


def run(model, jobs, backend=None):
  """(cov [n, 3], std, status) through the host build (None), its contracted twin ("fast") or the library ("device")"""
  if backend == "device":
    return uncertainty.run_jobs(model, jobs)
  if backend == "fast":
    return on_fast(uncertainty.run_jobs, model, jobs)
  return on_host(uncertainty.run_jobs, model, jobs)


def whitened_difference(got, want):
  """|L^-1 (C_got - C_want) L^-T|_F per query with L L^T = C_want, [n, 3] blocks; a direction whose variance is below 1e-6 of the
  larger one (a covariance of rank one) is whitened by that floor"""
  out = np.zeros(len(want))
  for i, (g, w) in enumerate(zip(got, want)):
    Cw = np.array([[w[0], w[1]], [w[1], w[2]]])
    D = np.array([[g[0] - w[0], g[1] - w[1]], [g[1] - w[1], g[2] - w[2]]])
    lam, V = np.linalg.eigh(Cw)
    s = 1.0 / np.sqrt(np.maximum(lam, max(1e-6 * lam.max(), 1e-300)))
    Li = (V * s).T
    out[i] = np.linalg.norm(Li @ D @ Li.T)
  return out
