"""TEST INFRASTRUCTURE: ctypes wrapper of tests/guidance (g++ build of multical_amd/csrc/mcba_guidance.h, the mathematics of
mcba_view_information) + what the view-information tests share: the nine cameras of uncertainty_host_lib (200 x 150 pixels), planar
boards of any point count, poses that put them in front of a camera, and random factors W = M F."""
import ctypes as C
import os
import subprocess

import numpy as np

import host_build
from multical_amd import _lib, guidance, uncertainty

import uncertainty_host_lib as ul

_host = host_build.HostLib("guidance", "gdh", ["view_information"], module=guidance)
lib, build, entry, host_backend, on_host = _host.lib, _host.build, _host.entry, _host.host_backend, _host.on_host
W_IMG, H_IMG = ul.W_IMG, ul.H_IMG


def fast_lib():
  """the -ffp-contract=fast build, in a library of its own name"""
  path = os.path.join(host_build.HERE, "guidance", "_build", "libmcba_guidance_fast.so")
  src = os.path.join(host_build.HERE, "guidance", "guidance.cpp")
  if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(host_build.path("guidance")):
    lib()
    subprocess.check_call(["g++"] + host_build.BASE_FLAGS + ["-ffp-contract=fast", "-mfma", "-shared", "-o", path, src])
  h = C.CDLL(path)
  fn = h.gdh_view_information
  fn.restype, fn.argtypes = C.c_int32, dict((n, a) for n, _, a in _lib.SYMBOLS)["mcba_view_information"]
  h.gdh_last_error.restype = C.c_char_p

  def call(name):
    def run(*args):
      if fn(*args) != 0:
        raise RuntimeError(h.gdh_last_error().decode())
    return run
  return call


def on_fast(fn, *args, **kwargs):
  saved = guidance._entry
  guidance._entry = fast_lib()
  try:
    return fn(*args, **kwargs)
  finally:
    guidance._entry = saved


def cameras():
  """the nine cameras as the device reads them (fx = fy under fix_aspect)"""
  return ul.rig().cameras


def n_dist(c):
  return ul.rig().n_dist[c]


def fix_aspect(c):
  return ul.rig().fix_aspect[c]


def board(P, spacing=0.012):
  """P points of a planar grid about 9 wide, centred, z = 0 (the last row may be short)"""
  i = np.arange(P)
  w = int(np.ceil(np.sqrt(max(P, 1))))
  pts = np.stack([(i % w) * spacing, (i // w) * spacing, np.zeros(P)], axis=1)
  return pts - 0.5 * (pts.max(axis=0) + pts.min(axis=0)) if P else pts


def pose(seed, distance=0.45, tilt=0.35, shift=0.04):
  """board-in-camera pose [4, 4]: in front of the camera, tilted and shifted at random"""
  from scipy.spatial.transform import Rotation
  rng = np.random.default_rng(seed)
  T = np.eye(4)
  T[:3, :3] = Rotation.from_rotvec(rng.uniform(-tilt, tilt, 3)).as_matrix()
  T[:3, 3] = [rng.uniform(-shift, shift), rng.uniform(-shift, shift), distance * rng.uniform(0.9, 1.3)]
  return T


def stored_factor(c, r, seed, scale=3e-4, held=()):
  """F [5 + n_dist, r] over the stored block fx fy cx cy skew dist.. of camera c: random, the entries in the units of their
  parameters, zero rows for the skew (no residual depends on it) and for `held`"""
  rng = np.random.default_rng(seed)
  p = 5 + n_dist(c)
  F = rng.normal(size=(p, r)) * scale
  F[:4] *= 1e3
  F[4] = 0.0
  F[list(held)] = 0.0
  return F


def device_factor(c, F):
  """(W [KI_c, r], unconstrained=False) of a stored factor"""
  return np.ascontiguousarray(uncertainty.camera_map(n_dist(c), fix_aspect(c)) @ F), False


def empty_factors():
  return [(np.zeros((4 + n_dist(c), 0)), False) for c in range(len(cameras()))]


def run(factors, boards, views, foci=None, backend=None, **kwargs):
  """view_information through the host build (None), its contracted twin ("fast") or the library ("device")"""
  args = (cameras(), factors, boards, views, foci)
  if backend == "device":
    return guidance.view_information(*args, **kwargs)
  if backend == "fast":
    return on_fast(guidance.view_information, *args, **kwargs)
  return on_host(guidance.view_information, *args, **kwargs)
