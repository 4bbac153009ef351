"""TEST INFRASTRUCTURE: ctypes wrapper of tests/length_host (g++ build of the pair mathematics of multical_amd/csrc/mcba_recon.h behind
the signature of mcba_reconstruction_pairs) and what the length-uncertainty tests share.  Rigs, factors and the long-double rows come
from reconstruction_uncertainty_host_lib."""
import ctypes as C
import os
import subprocess

import numpy as np

import host_build
from multical_amd import _lib, reconstruction

import reconstruction_uncertainty_host_lib as rl

_host = host_build.HostLib("length_host", "lph", ["reconstruction_pairs"], module=reconstruction)
lib, build, entry, host_backend, on_host = _host.lib, _host.build, _host.entry, _host.host_backend, _host.on_host
RAW = ("cov_diff_cal", "cross_cal", "cov_diff_noise", "length", "length_var_cal", "length_var_noise", "views_a", "views_b", "status")
COVARIANCES = ("cov_diff_cal", "cross_cal", "cov_diff_noise", "length_var_cal", "length_var_noise")


def fast_entry():
  """the -ffp-contract=fast build, in a library of its own name: what stands in for reconstruction._entry"""
  path = os.path.join(host_build.HERE, "length_host", "_build", "libmcba_length_host_fast.so")
  src = os.path.join(host_build.HERE, "length_host", "length_host.cpp")
  lib()
  if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(host_build.path("length_host")):
    subprocess.check_call(["g++"] + host_build.BASE_FLAGS + ["-ffp-contract=fast", "-mfma", "-shared", "-o", path, src])
  h = C.CDLL(path)
  fn = h.lph_reconstruction_pairs
  fn.restype, fn.argtypes = C.c_int32, dict((n, a) for n, _, a in _lib.SYMBOLS)["mcba_reconstruction_pairs"]
  h.lph_last_error.restype = C.c_char_p

  def call(name):
    def run(*args):
      if fn(*args) != 0:
        raise RuntimeError(h.lph_last_error().decode())
    return run
  return call


def run(model, jobs, pairs, sigma2=1.0, margin=0.0, backend=None):
  """the raw outputs of run_pair_jobs through the host build (None), its contracted twin ("fast") or the library ("device")"""
  args = (model.cameras, model.poses, jobs, pairs, sigma2, margin)
  if backend == "device":
    return reconstruction.run_pair_jobs(*args)
  if backend == "fast":
    saved = reconstruction._entry
    reconstruction._entry = fast_entry()
    try:
      return reconstruction.run_pair_jobs(*args)
    finally:
      reconstruction._entry = saved
  return on_host(reconstruction.run_pair_jobs, *args)


def raw_bytes(out):
  return b"".join(np.asarray(out[k]).tobytes() for k in RAW)


def cross_difference(got, want, cov_a, cov_b):
  """max_ij |got - want|_ij / sqrt(C_a,ii C_b,jj) per pair (cross_cal is not symmetric: no Cholesky whitening); [K, 3, 3] blocks, cov_a
  and cov_b the [K, 3, 3] cov_cal of the two ends; 0 where both are NaN, inf where one is"""
  out = np.zeros(len(want))
  for i, (g, w) in enumerate(zip(got, want)):
    if not np.isfinite(w).all():
      out[i] = 0.0 if not np.isfinite(g).any() else np.inf
      continue
    scale = np.sqrt(np.outer(np.diag(cov_a[i]), np.diag(cov_b[i])))
    if scale.max() <= 0.0:
      out[i] = 0.0 if np.array_equal(g, w) else np.inf
      continue
    out[i] = (np.abs(g - w) / np.maximum(scale, 1e-6 * scale.max())).max()
  return out


def bar_points(model, camera, d, separation, along):
  """[2, 3] in the rig frame: the ends of a bar of length `separation` centred on the optical axis of `camera` at distance d, across
  the line of sight (along x of the camera) or along it"""
  T = np.linalg.inv(model.poses[camera])
  h = 0.5 * separation
  ends = [[0.0, 0.0, d - h], [0.0, 0.0, d + h]] if along else [[-h, 0.0, d], [h, 0.0, d]]
  return np.array([T[:3, :3] @ e + T[:3, 3] for e in ends])
