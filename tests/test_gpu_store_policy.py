"""GPU (MI355X): the store policy of the hand-off buffers (csrc/mcba_device.h: store_through, debug switch MCBA_STORE_THROUGH)
changes where the bytes travel, never the bytes: every result must be BIT-IDENTICAL with the switch on (default) and off.
What could go wrong is a store that lands at another address or is dropped (the 16-byte form stores through a bounded buffer
resource per view): the fixtures cover every record length, the partial last 64-lane pass of a record, empty views, views of
fewer than 64 observations and rigs without eliminated frame parameters (DF == 0).  k_assemble reads back what the same thread
stored write-through in two places -- a frame with more active views than staging slots (`sum += *dst`) and a chunk of more than
64 frames (`s0 = out[e0]`): a second pair of runs forces both (MCBA_ASM_STAGE_KB=4: one or two views per pass; MCBA_NCHUNK_TARGET=1
at 264 frames: four chunks of 66)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDENS = ["tiny", "tiny_rolling", "tiny_handeye", "tiny_fisheye", "tiny_edge", "tiny_pin4", "tiny_tilted", "tiny_softl1",
           "tiny_bigboard", "cfg1"]
SOLVED = ["tiny_rolling", "cfg1"]

CODE = r"""
import sys, json, os, numpy as np
sys.path.insert(0, "."); sys.path.insert(0, "tests")
from util import load_golden, mirror
from multical_amd.backend import Handle
from multical_amd import _lib, synthetic, calibration
if os.environ.get("TEST_STORE_THROUGH") is not None:
  _lib.set_switch("MCBA_STORE_THROUGH", os.environ["TEST_STORE_THROUGH"])
forced = os.environ.get("TEST_FORCED") == "1"
if forced:
  _lib.set_switch("MCBA_ASM_STAGE_KB", "4")
  _lib.set_switch("MCBA_NCHUNK_TARGET", "1")
out, meta = {}, {}
def record(key, h, x):
  cost, grad, diag = h.normal_equations(x)
  out[key + "/cost"] = np.array([cost]); out[key + "/grad"] = grad; out[key + "/diag"] = diag; out[key + "/H"] = h.dense_hessian()
for name in ([] if forced else json.loads(os.environ["TEST_GOLDENS"])):
  g, rig = load_golden(name)
  with Handle(mirror(rig)) as h:
    record(name, h, g["x0"])
    if name in json.loads(os.environ["TEST_SOLVED"]):
      for solver in ("exact", "lsmr"):
        res = h.solve(g["x0"], tr_solver=solver)
        out[name + "/x_" + solver] = res.x
        meta[name + "/" + solver] = [int(res.nfev), int(h.lsmr_iterations()) if solver == "lsmr" else 0]
frames = 264 if forced else 40
c = calibration.from_rig(synthetic.make_rig("cfg3", frames=frames))
with Handle(c) as h:
  record("cfg3_%d" % frames, h, c.param_vec)
np.savez(os.environ["TEST_OUT"], **out)
print("RESULT" + json.dumps(meta))
"""


@pytest.fixture(scope="module")
def both_policies(tmp_path_factory):
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  base = {k: v for k, v in os.environ.items() if not k.startswith("MCBA_") and not k.startswith("TEST_")}
  base.update(TEST_GOLDENS=json.dumps(GOLDENS), TEST_SOLVED=json.dumps(SOLVED))
  tmp = tmp_path_factory.mktemp("store_policy")
  res = {}
  for label, switch, forced in (("on", None, "0"), ("off", "0", "0"), ("on_forced", None, "1"), ("off_forced", "0", "1")):
    path = str(tmp / (label + ".npz"))
    env = dict(base, TEST_OUT=path, TEST_FORCED=forced)
    if switch is not None:
      env["TEST_STORE_THROUGH"] = switch
    p = subprocess.run([sys.executable, "-c", CODE], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    meta = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT")][0][6:])
    with np.load(path) as z:
      res[label] = ({k: z[k] for k in z.files}, meta)
  return res


@pytest.mark.parametrize("name", GOLDENS + ["cfg3_40"])
def test_normal_equations_are_bit_identical_under_both_store_policies(both_policies, name):
  on, off = both_policies["on"][0], both_policies["off"][0]
  for q in ("cost", "grad", "diag", "H"):
    a, b = on[name + "/" + q], off[name + "/" + q]
    assert a.size > 0 and np.all(np.isfinite(a)), (name, q)
    assert a.shape == b.shape and np.array_equal(a, b), (name, q)
  assert np.abs(on[name + "/H"]).max() > 0.0 and np.abs(on[name + "/grad"]).max() > 0.0, name


def test_read_back_paths_of_k_assemble_are_bit_identical_under_both_store_policies(both_policies):
  """several staging passes per frame and several 64-frame passes per chunk (forced): the thread re-reads its own earlier store"""
  on, off, plain = both_policies["on_forced"][0], both_policies["off_forced"][0], both_policies["on"][0]
  for q in ("cost", "grad", "diag", "H"):
    a, b = on["cfg3_264/" + q], off["cfg3_264/" + q]
    assert a.size > 0 and np.all(np.isfinite(a)), q
    assert a.shape == b.shape and np.array_equal(a, b), q
  n40, n264 = plain["cfg3_40/grad"].size, on["cfg3_264/grad"].size
  assert n264 > n40 and np.abs(on["cfg3_264/H"]).max() > 0.0   # (the larger rig really ran)


@pytest.mark.parametrize("name", SOLVED)
@pytest.mark.parametrize("solver", ["exact", "lsmr"])
def test_solves_are_identical_under_both_store_policies(both_policies, name, solver):
  (on, mon), (off, moff) = both_policies["on"], both_policies["off"]
  assert np.array_equal(on[name + "/x_" + solver], off[name + "/x_" + solver]), (name, solver)
  assert mon[name + "/" + solver] == moff[name + "/" + solver], (name, solver)   # nfev, lsmr_iterations
  if solver == "lsmr":
    assert mon[name + "/" + solver][1] > 0
