"""TEST INFRASTRUCTURE: the one builder and loader of the g++ test libraries (tests/<name>/<name>.cpp: host builds of the product's
__host__ __device__ headers).  The *_lib.py wrappers state their source and flags; the rule of when to rebuild lives here."""
import ctypes as C
import os
import subprocess

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
