"""TEST INFRASTRUCTURE: ctypes wrapper of tests/rigview (g++ build of multical_amd/csrc/mcba_rigview.h, the mathematics of
mcba_rig_view_information) + what the rig-view tests share: groups of the nine cameras of uncertainty_host_lib on their arc, boards
and board-in-rig poses that several of them see, and random joint factors over the stored camera and pose blocks."""
import ctypes as C
import os
import subprocess

import numpy as np

import host_build
from multical_amd import _lib, guidance, uncertainty

import guidance_host_lib as gl
import uncertainty_host_lib as ul

_host = host_build.HostLib("rigview", "rvh", ["rig_view_information"], module=guidance)
lib, build, entry, host_backend, on_host = _host.lib, _host.build, _host.entry, _host.host_backend, _host.on_host
board = gl.board


def fast_lib():
  """the -ffp-contract=fast build, in a library of its own name"""
  path = os.path.join(host_build.HERE, "rigview", "_build", "libmcba_rigview_fast.so")
  src = os.path.join(host_build.HERE, "rigview", "rigview.cpp")
  if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(host_build.path("rigview")):
    lib()
    subprocess.check_call(["g++"] + host_build.BASE_FLAGS + ["-ffp-contract=fast", "-mfma", "-shared", "-o", path, src])
  h = C.CDLL(path)
  fn = h.rvh_rig_view_information
  fn.restype, fn.argtypes = C.c_int32, dict((n, a) for n, _, a in _lib.SYMBOLS)["mcba_rig_view_information"]
  h.rvh_last_error.restype = C.c_char_p

  def call(name):
    def run(*args):
      if fn(*args) != 0:
        raise RuntimeError(h.rvh_last_error().decode())
    return run
  return call


def on_fast(fn, *args, **kwargs):
  saved = guidance._entry
  guidance._entry = fast_lib()
  try:
    return fn(*args, **kwargs)
  finally:
    guidance._entry = saved


def group(members):
  """uncertainty.RigModel of the cameras `members` of the nine (device cameras, poses and stored pose parameters)"""
  full = ul.rig()
  members = list(members)
  return uncertainty.RigModel([ul.source_cameras()[c] for c in members], full.poses[members], full.rtvecs[members])


def rig_pose(rig, seed, distance=0.6, tilt=0.3, shift=0.03, towards=None):
  """board-in-rig pose [4, 4]: in front of camera `towards` of the group (default: its middle camera), tilted and shifted at random"""
  c = len(rig.cameras) // 2 if towards is None else towards
  return np.linalg.inv(rig.poses[c]) @ gl.pose(seed, distance, tilt, shift)


def stored_rows(rig):
  """rows[c]: the rows of camera c (stored camera block | pose) in the joint factor"""
  rows, at = [], 0
  for c in range(len(rig.cameras)):
    n = 5 + rig.n_dist[c] + 6
    rows.append(np.arange(at, at + n))
    at += n
  return rows, at


def stored_factor(rig, r, seed, held_poses=(0,), scale=3e-4):
  """F [p, r] over the stored blocks (camera | pose per camera) of the group: random as gl.stored_factor, the entries in the units of
  their parameters, zero rows for the skews, for the second focal length under fix_aspect and for the poses of `held_poses`"""
  rng = np.random.default_rng(seed)
  rows, p = stored_rows(rig)
  F = rng.normal(size=(p, r)) * scale
  for c, idx in enumerate(rows):
    F[idx[:4]] *= 1e3
    F[idx[4]] = 0.0
    if rig.fix_aspect[c]:
      F[idx[1]] = 0.0
    if c in held_poses:
      F[idx[-6:]] = 0.0
  return F


def device_factors(rig, F, loose=()):
  rows, _ = stored_rows(rig)
  out = [guidance.rig_device_factor(rig, c, F[rows[c]]) for c in range(len(rig.cameras))]
  return [(W, c in loose) for c, (W, _) in enumerate(out)]


def run(rig, factors, boards, views, focus=None, backend=None, **kwargs):
  """rig_view_information through the host build (None), its contracted twin ("fast") or the library ("device")"""
  args = (rig.cameras, rig.poses, factors, boards, views, focus)
  if backend == "device":
    return guidance.rig_view_information(*args, **kwargs)
  if backend == "fast":
    return on_fast(guidance.rig_view_information, *args, **kwargs)
  return on_host(guidance.rig_view_information, *args, **kwargs)
