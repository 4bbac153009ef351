"""Frame sharding behind the drop-in API: multical_amd.distributed.sharding() / dropin.install(shard=True) route the solves and the
outlier loop of Calibration (and so Workspace.calibrate) to frame-sharded handles.  CPU: the switch, the shard plan and its
cross-rank agreement over gloo.  GPU: 2 - 4 ranks sharing one MI355X over gloo -- the gathered inlier mask (mcba_gather_inliers), the
sharded order statistics, Workspace.calibrate and the drop-in against a single handle and the reference's goldens, and the
collectives of a sharded outlier round."""
import datetime
import json
import os
import socket
import sys
import types

import numpy as np
import pytest

from multical_amd import calibration, distributed as mdist, dropin
from util import GOLDEN, load_golden, mirror

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = datetime.timedelta(seconds=60)


def _free_port():
  s = socket.socket()
  s.bind(("127.0.0.1", 0))
  p = s.getsockname()[1]
  s.close()
  return p


def _load(name):
  if name == "cfg5_40":
    from multical_amd import synthetic
    g = dict(np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False))
    return g, synthetic.make_rig(str(g["config"]))
  return load_golden(name)


def _golden_mask(g, rig):
  if "ao_inliers" in g:
    return g["ao_inliers"].astype(bool)
  return np.unpackbits(g["ao_inliers_packed"])[:rig.valid.size].reshape(rig.valid.shape).astype(bool)


def _init(rank, world, port, device=True):
  sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
  import faulthandler
  faulthandler.dump_traceback_later(300, exit=True)      # a deadlocked collective ends the test with a traceback
  import torch
  import torch.distributed as dist
  os.environ["MASTER_ADDR"] = "127.0.0.1"
  os.environ["MASTER_PORT"] = str(port)
  if device:
    torch.cuda.set_device(0)                             # the ranks share the one GPU of the test box (gloo: host-staged sums)
  dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)
  return dist


def _finish(dist, rank, out, result):
  """every rank's result to rank 0, which saves them all"""
  got = [None] * dist.get_world_size()
  dist.all_gather_object(got, result)
  if rank == 0:
    np.save(out, np.array(got, dtype=object), allow_pickle=True)
  dist.destroy_process_group()


def _spawn(fn, world, *args):
  import torch.multiprocessing as mp
  mp.spawn(fn, args=(world, _free_port()) + args, nprocs=world, join=True)


def _results(out):
  return list(np.load(out, allow_pickle=True))


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_sharding_is_off_by_default_and_needs_a_process_group():
  assert not mdist.sharding_enabled()
  assert mdist.shard_config() is None
  with pytest.raises(RuntimeError, match="process group"):
    with mdist.sharding():
      pass
  with pytest.raises(RuntimeError, match="process group"):
    mdist.enable_sharding()
  assert not mdist.sharding_enabled()


def test_world_size_one_has_no_shard_plan():
  g, rig = load_golden("cfg1")
  c = mirror(rig)
  assert mdist.shard_plan(c, 1) is None
  plan = mdist.shard_plan(c, 2)
  assert plan[0][0] == 0 and plan[-1][1] == rig.valid.shape[1] and plan[0][1] == plan[1][0]


def test_install_with_shard_patches_and_uninstall_restores(monkeypatch):
  class Plain(calibration.Calibration):
    def bundle_adjust(self, tolerance=1e-4, f_scale=1.0, max_iterations=100, loss='linear'):
      raise AssertionError("un-patched")
  original = Plain.bundle_adjust
  mod = types.SimpleNamespace(Calibration=Plain)
  try:
    assert dropin.install(calibration_module=mod, shard=True) is Plain
    assert Plain.bundle_adjust is dropin.bundle_adjust and dropin._shard["on"]
    dropin.uninstall(calibration_module=mod)
    assert Plain.bundle_adjust is original and not dropin._shard["on"]
    monkeypatch.setenv("MULTICAL_BACKEND", "hip-native")
    monkeypatch.setenv("MULTICAL_SHARD", "1")
    monkeypatch.setattr(dropin, "install", lambda **k: k)      # (install_from_env patches the real multical module)
    assert dropin.install_from_env() == dict(mode="native", shard=True)
    monkeypatch.setenv("MULTICAL_SHARD", "0")
    assert dropin.install_from_env() == dict(mode="native", shard=False)
    monkeypatch.setenv("MULTICAL_BACKEND", "hip")
    assert dropin.install_from_env() == dict(shard=False)
  finally:
    dropin.uninstall(calibration_module=mod)
  assert Plain.bundle_adjust is original


def _plan_worker(rank, world, port, out, disagree):
  dist = _init(rank, world, port, device=False)
  g, rig = load_golden("cfg1")
  c = mirror(rig)
  F = rig.valid.shape[1]
  w = c.inliers.sum(axis=(0, 2, 3)).astype(np.float64)
  if disagree and rank == 1:
    w[:F // 2] *= 10.0                     # another Calibration on this rank: another plan
  plan = mdist.frame_shards(F, world, w)
  try:
    mdist.agree_on_plan(plan, None)
    result = ("agreed", plan)
  except RuntimeError as e:
    result = ("raised", str(e))
  _finish(dist, rank, out, result)


@pytest.mark.parametrize("disagree", [False, True])
def test_ranks_agree_on_the_plan_or_all_raise_gloo(disagree, tmp_path):
  import time
  out = str(tmp_path / "plan.npy")
  t0 = time.time()
  _spawn(_plan_worker, 2, out, disagree)
  assert time.time() - t0 < TIMEOUT.total_seconds()
  res = _results(out)
  if disagree:
    assert all(r[0] == "raised" and "differ" in r[1] for r in res), res
  else:
    assert all(r[0] == "agreed" for r in res) and res[0][1] == res[1][1]
    g, rig = load_golden("cfg1")
    assert [tuple(s) for s in res[0][1]] == [tuple(s) for s in mdist.shard_plan(mirror(rig), 2)]


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: mcba_gather_inliers + sharded order statistics
# ---------------------------------------------------------------------------------------------------------------------------------
QS = (0, 0.25, 0.5, 0.75, 1)


def _shards(kind, F, world):
  if kind == "uneven":
    return [(0, 3), (3, F)] if world == 2 else None
  if kind == "empty":                       # rank 1 owns nothing
    a, b = F // 3, 2 * F // 3
    return [(0, a), (a, a), (a, b), (b, F)] if world == 4 else [(0, F)] + [(F, F)] * (world - 1)
  return None


def _threshold(c):
  from multical_amd.backend import Handle
  with Handle(c) as h:                      # replicated: every rank derives the same threshold
    _, _, q, _ = h.error_stats(c.param_vec, quantiles=[0.5])
  return 2.0 * float(q[0])


def _gather_worker(rank, world, port, out, name, kind):
  dist = _init(rank, world, port)
  g, rig = load_golden(name)
  c = mirror(rig)
  x = c.param_vec
  thr = _threshold(c)
  h = mdist.sharded_handle(c, shards=_shards(kind, rig.valid.shape[1], world))
  h.set_allreduce_trace(1 << 16)
  h.allreduce_stats(reset=True)
  stats_all = h.error_stats(x, quantiles=QS)
  n_in, n_valid = h.reject_outliers(x, thr)
  stats_inl = h.error_stats(x, quantiles=QS, inliers_only=True)
  before = h.allreduce_stats(reset=True)[2]
  mask = h.gather_inliers()
  gather_sizes = h.allreduce_stats(reset=True)[2]
  result = dict(frame_range=h.frame_range, mask=mask, part=h.get_inliers(), n_in=n_in, n_valid=n_valid, stats_all=stats_all,
                stats_inl=stats_inl, sizes=before, gather_sizes=gather_sizes, thr=thr)
  h.close()
  _finish(dist, rank, out, result)


@pytest.mark.gpu
@pytest.mark.parametrize("name,world,kind", [("cfg1", 2, None), ("cfg1", 4, None), ("cfg1", 2, "uneven"), ("cfg1", 4, "empty"),
                                             ("tiny_boards", 2, None)])
def test_gathered_mask_and_sharded_statistics_equal_a_single_handle(name, world, kind, tmp_path):
  """mcba_gather_inliers: the complete [C,F,B,P] mask on every rank, bit for bit the single handle's after the same rejection --
  shard boundaries inside a 32-bit word of the packed message (cfg1: P = 315), an empty shard, boards=True.  Sharded error_stats:
  the same exact order statistics (same quantiles bit for bit), the same n, the sum of squares to 1e-13."""
  from multical_amd.backend import Handle
  out = str(tmp_path / "gather.npy")
  _spawn(_gather_worker, world, out, name, kind)
  res = _results(out)
  g, rig = load_golden(name)
  c = mirror(rig)
  x = c.param_vec
  C_, F, B, P = rig.valid.shape
  with Handle(c) as h:
    ref_all = h.error_stats(x, quantiles=QS)
    n_in, n_valid = h.reject_outliers(x, res[0]["thr"])
    ref_mask = h.get_inliers()
    ref_inl = h.error_stats(x, quantiles=QS, inliers_only=True)
  assert 0 < n_in < n_valid                                    # the rejection removes something and keeps something
  if name == "cfg1":                                           # a shard boundary falls inside a 32-bit word of the message
    starts = [r["frame_range"][0] for r in res if 0 < r["frame_range"][0] < F]
    assert any((s * B * P) % 32 != 0 for s in starts), starts
  if kind == "empty":
    assert any(r["frame_range"][0] == r["frame_range"][1] for r in res)
  words = -(-C_ * F * B * P // 32)
  for r in res:
    assert np.array_equal(r["mask"], ref_mask)
    f0, f1 = r["frame_range"]                                  # mcba_get_inliers keeps its documented behaviour
    assert np.array_equal(r["part"][:, f0:f1], ref_mask[:, f0:f1]) and not r["part"][:, :f0].any() and not r["part"][:, f1:].any()
    assert (r["n_in"], r["n_valid"]) == (n_in, n_valid)
    assert r["gather_sizes"] == [words]                        # ONE collective
    for got, ref in ((r["stats_all"], ref_all), (r["stats_inl"], ref_inl)):
      assert got[3] == ref[3]
      assert np.array_equal(np.asarray(got[2]), np.asarray(ref[2]))
      assert got[0] == pytest.approx(ref[0], rel=1e-13)
    assert 1 not in r["sizes"] and -1 not in r["sizes"]        # no per-statistic pair of 1-double reductions


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: Workspace.calibrate under sharding()
# ---------------------------------------------------------------------------------------------------------------------------------
def _calibrate(rig, g, num_adjustments=3):
  from multical_amd import Workspace
  kw = json.loads(str(g["ao_kwargs_json"])) if "ao_kwargs_json" in g else {}
  return Workspace(mirror(rig)).calibrate(cameras=rig.optimize["cameras"], camera_poses=rig.optimize["camera_poses"],
                                          loss=kw.get("loss", "linear"), auto_scale=kw.get("auto_scale", None),
                                          num_adjustments=num_adjustments)


def _calibrate_worker(rank, world, port, out, name, solver, frames):
  dist = _init(rank, world, port)
  from util import sub_rig
  g, rig = _load(name)
  if frames:
    rig = sub_rig(rig, frames)
  calibration.set_solver(solver)
  created = []
  orig = mdist.sharded_handle
  mdist.sharded_handle = lambda *a, **k: created.append(1) or orig(*a, **k)
  with mdist.sharding():
    o = _calibrate(rig, g)
    rms_inl = o.error_statistics(True).rms
    stats = o.error_statistics()
  mdist.sharded_handle = orig
  assert not calibration.handle_cache.sharded                 # leaving sharding() closes the group's handles
  _finish(dist, rank, out, dict(x=o.param_vec, mask=o.inliers, rms_inl=rms_inl, n=stats.n, created=len(created)))


@pytest.mark.gpu
@pytest.mark.parametrize("name,world,solver,frames", [("cfg1", 2, "lsmr", None), ("tiny_rolling", 2, "lsmr", None),
                                                      ("tiny_handeye", 2, "lsmr", None), ("tiny_autoscale", 2, "lsmr", None),
                                                      ("cfg5_40", 2, "lsmr", None), ("cfg1", 2, "native", None),
                                                      ("tiny_rolling", 4, "lsmr", 3)])
def test_sharded_workspace_calibrate(name, world, solver, frames, tmp_path):
  """Workspace.calibrate inside distributed.sharding(): every rank returns the same parameter vector (bits) and inlier mask; against
  the reference's golden within the tolerances of the single-GPU test; against a single-handle run of the same call the mask is
  identical wherever that run's errors lie more than 1e-9 px from the threshold of the last rejection.  (frames = 3 with 4 ranks:
  fewer frames than ranks -- one shard is empty.)"""
  from util import sub_rig
  out = str(tmp_path / "calibrate.npy")
  _spawn(_calibrate_worker, world, out, name, solver, frames)
  res = _results(out)
  for r in res[1:]:
    assert np.array_equal(r["x"], res[0]["x"]) and r["x"].tobytes() == res[0]["x"].tobytes()
    assert np.array_equal(r["mask"], res[0]["mask"])
  assert res[0]["created"] >= 1                                # the loop DID run on sharded handles
  g, rig = _load(name)
  if frames:
    rig = sub_rig(rig, frames)
  prev = calibration.set_solver(solver)
  try:
    single = _calibrate(rig, g)
    two = _calibrate(rig, g, 2)                 # x of the last rejection and (its final report) that round's threshold
  finally:
    calibration.set_solver(prev)
  e, v = two._errors()
  thr = two.error_statistics().quantiles[3] * 5.0
  clear = v & (np.abs(e - thr) > 1e-9)
  assert np.array_equal(single.inliers[clear], res[0]["mask"][clear]), int((single.inliers[clear] != res[0]["mask"][clear]).sum())
  assert res[0]["n"] == single.error_statistics().n
  if frames is None:
    allowed = int(g["ao_pert_mask_diff"].max()) if "ao_pert_mask_diff" in g else 0
    assert int((res[0]["mask"] != _golden_mask(g, rig)).sum()) <= allowed
    spread = float(np.abs(g["ao_pert_rms_inliers"] - g["ao_rms_inliers"]).max())
    assert abs(res[0]["rms_inl"] - float(g["ao_rms_inliers"])) <= max(1e-6, 3 * spread), (res[0]["rms_inl"], float(g["ao_rms_inliers"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the collectives of a sharded outlier round
# ---------------------------------------------------------------------------------------------------------------------------------
def _budget_worker(rank, world, port, out, frames):
  dist = _init(rank, world, port)
  from util import sub_rig
  g, rig = load_golden("cfg1")
  if frames:
    rig = sub_rig(rig, frames)
  c = mirror(rig)
  h = mdist.sharded_handle(c)
  h.set_allreduce_trace(1 << 20)
  # the solve alone, then the same solve inside a 1-round outlier loop: the difference is what the round adds
  h.allreduce_stats(reset=True)
  res = h.solve(c.param_vec)
  solve_sizes = h.allreduce_stats(reset=True, cap=1 << 20)[2]
  h.set_inliers(None)
  x, rounds, mask = h.adjust_outliers(c.param_vec, 1, outlier=(0.75, 5.0), tr_solver="exact")
  loop_sizes = h.allreduce_stats(reset=True, cap=1 << 20)[2]
  h.close()
  _finish(dist, rank, out, dict(solve=solve_sizes, loop=loop_sizes, n=res.x.size, shape=rig.valid.shape))


@pytest.mark.gpu
def test_collectives_of_a_sharded_outlier_round(tmp_path):
  """Apart from the solve's messages, a sharded round issues the report scalars (2, and 4 with the inlier sums riding along), the
  histogram passes (2048 k), one 2 nsel W tail message per selection batch and the 2-double rejection totals -- no 1-double
  reductions per statistic -- and exactly one ceil(C F B P / 32) mask message per call.  Nothing else depends on F: the same on
  the rig cut to 12 frames."""
  world = 2
  seen = {}
  for frames in (None, 12):
    out = str(tmp_path / f"budget{frames}.npy")
    _spawn(_budget_worker, world, out, frames)
    r = _results(out)[0]
    C_, F, B, P = r["shape"]
    n_motion = 6 * F
    words = -(-C_ * F * B * P // 32)
    ns = r["n"] - n_motion
    solve_set = {2 * ns + 6, ns * ns + ns, 4 * world, 3 * world + 1, 4, n_motion}
    assert set(r["solve"]) <= solve_set
    round_msgs = {2, 4} | {2048 * k for k in range(1, 7)} | {2 * k * world for k in range(1, 7)}
    loop = list(r["loop"])
    assert loop.count(words) == 1 and loop[-1] == words, loop[-5:]
    body = loop[:-1]
    assert set(body) <= solve_set | round_msgs, sorted(set(body) - solve_set - round_msgs)
    assert 1 not in loop and not any(v < 0 for v in loop)
    assert 2048 in body and any(v in body for v in (2 * k * world for k in range(1, 7)))
    # the report in front of the round and the final report: each = {2 (n) | 4 (sums + inlier sums) | 2048 ... | tail}
    seen[frames] = sorted(set(body) - {n_motion, 2 * ns + 6, ns * ns + ns})
  assert seen[None] == seen[12], seen


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: drop-in with shard=True
# ---------------------------------------------------------------------------------------------------------------------------------
class _RefShapedCalibration(calibration.Calibration):
  """A reference-shaped Calibration whose own bundle_adjust must never run (install() replaces it); its adjust_outliers is the
  step-by-step loop that calls self.bundle_adjust, as the reference's does."""

  def bundle_adjust(self, tolerance=1e-4, f_scale=1.0, max_iterations=100, loss='linear'):
    raise AssertionError("the un-patched bundle_adjust was called")

  def copy(self, **k):
    d = self.__getstate__()
    d.update(k)
    return _RefShapedCalibration(**d)


def _dropin_worker(rank, world, port, out):
  dist = _init(rank, world, port)
  os.environ["MULTICAL_AMD_FUSED_LOOP"] = "0"                 # the step-by-step loop: report / reject / patched bundle_adjust
  created = []
  orig = mdist.sharded_handle
  mdist.sharded_handle = lambda *a, **k: created.append(1) or orig(*a, **k)
  mod = types.SimpleNamespace(Calibration=_RefShapedCalibration)
  try:
    dropin.install(calibration_module=mod, shard=True)
    g, rig = load_golden("cfg1")
    c = _RefShapedCalibration(**mirror(rig).__getstate__())
    ao = c.adjust_outliers(num_adjustments=3, select_outliers=calibration.select_threshold(0.75, 5.0))
    result = dict(x=ao.param_vec, mask=ao.inliers, rms_inl=calibration.error_stats(ao.reprojection_inliers).rms, created=len(created))
  finally:
    dropin.uninstall(calibration_module=mod)
    mdist.sharded_handle = orig
  _finish(dist, rank, out, result)


@pytest.mark.gpu
def test_dropin_install_shard_runs_adjust_outliers_sharded(tmp_path):
  out = str(tmp_path / "dropin.npy")
  _spawn(_dropin_worker, 2, out)
  res = _results(out)
  g, rig = load_golden("cfg1")
  assert res[0]["created"] == 3 and res[1]["created"] == 3     # every bundle_adjust on a frame-sharded handle
  for r in res:
    assert r["x"].tobytes() == res[0]["x"].tobytes()
    assert np.array_equal(r["mask"], g["ao_inliers"])
    assert abs(r["rms_inl"] - float(g["ao_rms_inliers"])) < 1e-6
