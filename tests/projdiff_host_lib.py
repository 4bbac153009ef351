"""TEST INFRASTRUCTURE: ctypes wrapper of tests/projdiff_host (g++ build of multical_amd/csrc/mcba_projdiff.h, the mathematics of
mcba_projection_diff) + the two calibrations the projection-difference tests share: the nine-camera rig of uncertainty_host_lib as
calibration 0, and calibration 1 = the same rig perturbed (focal lengths +-0.1 %, principal point +-3 px, coefficients +-5 %, camera
poses +-2 mrad / +-1 mm, seeded)."""
import ctypes as C

import numpy as np

import host_build
from multical_amd import _lib, compare, transform, uncertainty
from multical_amd.undistort import CameraSetInputs

import uncertainty_host_lib as ul

_host = host_build.HostLib("projdiff_host", "phd", ["projection_diff"], extra=dict(
    fit_planted=[C.POINTER(_lib.CameraSet), C.POINTER(_lib.CameraSet), C.POINTER(_lib.ProjDiffJob), _lib.c_double_p, _lib.c_double_p,
                 _lib.c_uint8_p]), module=compare)
lib, build, entry, host_backend, on_host = _host.lib, _host.build, _host.entry, _host.host_backend, _host.on_host
W_IMG, H_IMG = ul.W_IMG, ul.H_IMG
IMAGE_SIZE = (W_IMG, H_IMG)
_rigs = []


def perturbed(model, source, seed=11):
  """RigModel of calibration 1 (and its source cameras)"""
  rng = np.random.default_rng(seed)
  cams = []
  for c in source:
    K = np.array(c.intrinsic, dtype=np.float64)
    K[0, 0] *= 1.0 + rng.uniform(-1e-3, 1e-3)
    K[1, 1] *= 1.0 + rng.uniform(-1e-3, 1e-3)
    K[0, 2] += rng.uniform(-3.0, 3.0)
    K[1, 2] += rng.uniform(-3.0, 3.0)
    dist = np.asarray(c.dist, dtype=np.float64) * (1.0 + rng.uniform(-0.05, 0.05, np.asarray(c.dist).shape))
    cams.append(c.copy(intrinsic=K, dist=dist))
  rt = model.rtvecs.copy()
  rt[:, :3] += rng.uniform(-2e-3, 2e-3, rt[:, :3].shape)
  rt[:, 3:] += rng.uniform(-1e-3, 1e-3, rt[:, 3:].shape)
  return uncertainty.RigModel(cams, transform.to_matrix(rt), rt), cams


def rigs():
  """(rig0, rig1): RigModels of the two calibrations (shared, unchanged by the tests)"""
  if not _rigs:
    rig0 = ul.rig()
    rig1, cams1 = perturbed(rig0, ul.source_cameras())
    _rigs.extend([rig0, rig1, cams1])
  return _rigs[0], _rigs[1]


def spread_pixels(n, seed=0, margin=0.0):
  """n pixels over the image, the nine edge pixels first"""
  rng = np.random.default_rng(seed)
  px = np.concatenate([ul.edge_pixels(), rng.uniform([margin, margin], [W_IMG - 1 - margin, H_IMG - 1 - margin], (max(n, 9), 2))])
  return np.ascontiguousarray(px[:n])


def inner_pixels(n, seed=0):
  """n pixels of the inner image (every camera of the rig is monotone there under both calibrations)"""
  rng = np.random.default_rng(seed)
  return np.ascontiguousarray(rng.uniform([30.0, 25.0], [W_IMG - 31.0, H_IMG - 26.0], (n, 2)))


def fit_job(b, distance, mode, fit_pixels=None, focus=None, **where):
  """an intrinsics job with a fit set of its own (default: the 60 x 40 grid)"""
  sets = dict(fit_pixels=fit_pixels) if fit_pixels is not None else dict(fit_grid=uncertainty.grid_of(IMAGE_SIZE, (60, 40)))
  if not where:
    where = dict(grid=uncertainty.grid_of(IMAGE_SIZE, (16, 12)))
  return compare.Job(b, None, distance, mode, focus=focus, **sets, **where)


def run(jobs, backend=None, pair=None):
  """compare.run_jobs through the host build (None) or the library ("device")"""
  rig0, rig1 = rigs() if pair is None else pair
  if backend == "device":
    return compare.run_jobs(rig0, rig1, jobs)
  return on_host(compare.run_jobs, rig0, rig1, jobs)


def fit_planted(job, planted, pair=None):
  """(fit record [12], valid [m]) of the header's fit function on targets project_b^1(R(omega*) n + rho tau*)"""
  rig0, rig1 = rigs() if pair is None else pair
  inp0, inp1 = CameraSetInputs(rig0.cameras), CameraSetInputs(rig1.cameras)
  rec = _lib.ProjDiffJob()
  rec.camera, rec.reference, rec.inv_distance, rec.fit = job.camera, -1, job.rho, job.fit
  m = job.fit_pixel_array()
  if job.fit_pixels is not None:
    rec.fit_n, rec.fit_uv = len(job.fit_pixels), _lib.dp(job.fit_pixels)
  else:
    rec.fit_grid_w, rec.fit_grid_h, rec.fit_u0, rec.fit_v0, rec.fit_du, rec.fit_dv = job.fit_grid
  rec.focus_u, rec.focus_v, rec.focus_radius = job.focus
  planted = np.ascontiguousarray(np.asarray(planted, dtype=np.float64))
  fit, valid = np.zeros(12), np.zeros(len(m), dtype=np.uint8)
  _host.check(lib().phd_fit_planted(C.byref(inp0.struct()), C.byref(inp1.struct()), C.byref(rec), _lib.dp(planted), _lib.dp(fit),
                                    _lib.up(valid)))
  return fit, valid.astype(bool)


def bytes_of(r):
  return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in ("transform", "fit_info", "diff", "magnitude", "landing", "status"))
