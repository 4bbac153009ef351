"""TEST INFRASTRUCTURE: the one builder, loader and binder of the g++ test libraries (tests/<name>/<name>.cpp: host builds of the
product's __host__ __device__ headers), and the compile line of the stand-alone sanitiser programs.  The *_lib.py wrappers state
their library, prefix and entries; the rule of when to rebuild and how an entry is bound and called lives here."""
import contextlib
import ctypes as C
import os
import subprocess

from multical_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "multical_amd", "csrc")
BASE_FLAGS = ["-O2", "-std=c++17", "-fPIC"]
# the plain IEEE evaluation of the formulas (the device contracts FP64 expressions to FMAs; the float32 interpolation of the
# undistortion is written in explicit fmaf and must not change with this flag)
IEEE = ["-ffp-contract=off"]


def path(name):
  return os.path.join(HERE, name, "_build", f"libmcba_{name}.so")


def build(name, source, flags, force=False):
  """g++ tests/<name>/<source> -> tests/<name>/_build/libmcba_<name>.so when it is older than the source, include/mcba.h or any
  header of csrc/."""
  lib, src = path(name), os.path.join(HERE, name, source)
  os.makedirs(os.path.dirname(lib), exist_ok=True)
  deps = [src, os.path.join(ROOT, "include", "mcba.h")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
  if force or not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
    subprocess.check_call(["g++"] + BASE_FLAGS + list(flags) + ["-shared", "-o", lib, src])
  return lib


def load(name, prefix):
  """The built library with <prefix>_last_error wired."""
  h = C.CDLL(path(name))
  getattr(h, prefix + "_last_error").restype = C.c_char_p
  return h


class HostLib(object):
  """tests/<name>/<name>.cpp as a library: built on demand, loaded once, <prefix>_last_error wired.  names: <prefix>_<name> has the
  signature of the mcba_<name> entry of _lib.SYMBOLS; extra: {name: argtypes} of the entries with an argument of their own (they
  return int32).  module: the multical_amd wrapper module whose `_entry` the host build can stand in for."""

  def __init__(self, name, prefix, names=(), extra=None, flags=IEEE, module=None):
    self.name, self.prefix, self.names, self.extra, self.flags, self.module = name, prefix, names, extra or {}, flags, module
    self._h = None

  def build(self, force=False):
    return build(self.name, self.name + ".cpp", self.flags, force)

  def lib(self):
    if self._h is None:
      self.build()
      h = load(self.name, self.prefix)
      signatures = {name: (restype, argtypes) for name, restype, argtypes in _lib.SYMBOLS}
      bound = {name: signatures["mcba_" + name] for name in self.names}
      bound.update({name: (C.c_int32, argtypes) for name, argtypes in self.extra.items()})
      for name, (restype, argtypes) in bound.items():
        fn = getattr(h, f"{self.prefix}_{name}")
        fn.restype, fn.argtypes = restype, argtypes
      self._h = h
    return self._h

  def check(self, rc):
    if rc != 0:
      raise RuntimeError(getattr(self.lib(), self.prefix + "_last_error")().decode())

  def entry(self, name):
    """the wrapper module's _entry of the host build"""
    fn = getattr(self.lib(), f"{self.prefix}_{name}")
    return lambda *args: self.check(fn(*args))

  @contextlib.contextmanager
  def host_backend(self):
    """the wrapper module (and what sits on it) served by the host build"""
    saved = self.module._entry
    self.module._entry = self.entry
    try:
      yield self.module
    finally:
      self.module._entry = saved

  def on_host(self, fn, *args, **kwargs):
    with self.host_backend():
      return fn(*args, **kwargs)


def sanitized_program(name, source, tmp_path):
  """g++ tests/<name>/<source> as a stand-alone executable under AddressSanitizer + UBSan (CPU only; nothing is loaded into Python,
  nothing is preloaded), run once: the finished process"""
  exe = str(tmp_path / os.path.splitext(source)[0])
  subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
                         "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(HERE, name, source)])
  return subprocess.run([exe], capture_output=True, text=True)
