"""Frame sharding.  CPU: shard planning + world_size-2 `gloo` reduction of per-shard normal equations
(computed by the product's device functions compiled for the host) equals the unsharded result.  GPU: two ranks sharing
one MI355X over gloo run the sharded HIP solve and reproduce the single-handle solve."""
import os
import socket
import sys

import numpy as np
import pytest

from multical_amd import distributed as mdist
from util import load_golden, mirror

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
  s = socket.socket()
  s.bind(("127.0.0.1", 0))
  p = s.getsockname()[1]
  s.close()
  return p


def test_frame_shards_cover_and_balance():
  for F, W in [(500, 8), (20, 3), (5, 8), (1, 2)]:
    sh = mdist.frame_shards(F, W)
    assert len(sh) == W and sh[0][0] == 0 and sh[-1][1] == F
    assert all(a[1] == b[0] for a, b in zip(sh, sh[1:]))
    assert max(b - a for a, b in sh) - min(b - a for a, b in sh) <= 1 or F < W
  w = np.zeros(100); w[:10] = 50; w[10:] = 1
  sh = mdist.frame_shards(100, 4, w)
  loads = [w[a:b].sum() for a, b in sh]
  assert max(loads) <= 2.5 * w.sum() / 4
  assert mdist.frame_shards(7, 2, np.zeros(7)) == [(0, 3), (3, 7)] or mdist.frame_shards(7, 2, np.zeros(7))[1][1] == 7


def _cpu_worker(rank, world, port, name, out):
  sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
  import torch
  import torch.distributed as dist
  from hostmath_lib import HostMath
  os.environ["MASTER_ADDR"] = "127.0.0.1"
  os.environ["MASTER_PORT"] = str(port)
  dist.init_process_group("gloo", rank=rank, world_size=world, timeout=__import__("datetime").timedelta(seconds=180))
  g, rig = load_golden(name)
  c = mirror(rig)
  F = rig.valid.shape[1]
  shard = mdist.frame_shards(F, world, c.inliers.sum(axis=(0, 2, 3)).astype(float))[rank]
  hm = HostMath(c, frame_range=shard)
  H, grad, cost = hm.normal_equations(g["x0"])
  buf = torch.from_numpy(np.concatenate([H.ravel(), grad, [cost, hm.m]]))
  dist.all_reduce(buf)                      # the same sum the GPU path performs through mcba_allreduce_fn
  if rank == 0:
    np.save(out, buf.numpy())
  dist.destroy_process_group()


@pytest.mark.parametrize("name", ["tiny_rolling", "cfg1"])
def test_sharded_normal_equations_sum_gloo(name, tmp_path):
  import torch.multiprocessing as mp
  from hostmath_lib import HostMath
  out = str(tmp_path / "reduced.npy")
  mp.spawn(_cpu_worker, args=(2, _free_port(), name, out), nprocs=2, join=True)
  red = np.load(out)
  g, rig = load_golden(name)
  hm = HostMath(mirror(rig))
  H, grad, cost = hm.normal_equations(g["x0"])
  n = hm.n
  assert np.abs(red[:n * n].reshape(n, n) - H).max() <= 1e-12 * np.abs(H).max()
  assert np.abs(red[n * n:n * n + n] - grad).max() <= 1e-12 * np.abs(grad).max()
  assert red[-2] == pytest.approx(cost, rel=1e-13)
  assert red[-1] == hm.m                                           # shards partition the residual vector


def _cpu_lsmr_worker(rank, world, port, name, out):
  sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
  import torch
  import torch.distributed as dist
  from hostmath_lib import HostMath
  os.environ["MASTER_ADDR"] = "127.0.0.1"
  os.environ["MASTER_PORT"] = str(port)
  dist.init_process_group("gloo", rank=rank, world_size=world)
  g, rig = load_golden(name)
  c = mirror(rig)
  F = rig.valid.shape[1]
  f0, f1 = mdist.frame_shards(F, world, c.inliers.sum(axis=(0, 2, 3)).astype(float))[rank]
  hm = HostMath(c, frame_range=(f0, f1))
  rng = np.random.default_rng(12)                      # the same v, u on every rank
  x = g["x0"] + 1e-3 * rng.normal(size=g["x0"].size)
  v = rng.normal(size=g["x0"].size)
  u = rng.normal(size=g["r0"].size)
  # rows of this shard in the reference's residual order (C-order over (c, f, b, p) restricted to the inliers)
  frame_of_row = np.repeat(np.nonzero(c.inliers)[1], 2)
  mine = (frame_of_row >= f0) & (frame_of_row < f1)
  assert mine.sum() == hm.m
  jv_local, jtu_local = hm.lsmr_products(x, v, u[mine])
  # J v: every row is computed by the rank that owns its frame -- no collective; J^T u: a sum over views, i.e. over the ranks
  jv = np.zeros(u.size)
  jv[mine] = jv_local
  tj, tt = torch.from_numpy(jv), torch.from_numpy(jtu_local.copy())
  dist.all_reduce(tj)                                   # (an all-gather written as a sum of disjoint supports)
  dist.all_reduce(tt)                                   # the GPU path reduces the SHARED entries only; the frame entries stay with the owner
  if rank == 0:
    np.savez(out, jv=tj.numpy(), jtu=tt.numpy(), x=x, v=v, u=u)
  dist.destroy_process_group()


@pytest.mark.parametrize("name", ["tiny_rolling", "tiny_boards", "cfg1"])
def test_sharded_lsmr_products_sum_gloo(name, tmp_path):
  """The decomposition the frame-sharded lsmr mode rests on, with the product's device functions on the CPU and a world-size-2 gloo
  group: J v is local to the owner of a frame, J^T u is the sum of the ranks' partial products (shared entries: a sum over all ranks,
  frame entries: non-zero on the owner only).  (The device kernels themselves: test_sharded_lsmr_solve_two_ranks_one_gpu.)"""
  import torch.multiprocessing as mp
  from hostmath_lib import HostMath
  out = str(tmp_path / "lsmr_products.npz")
  mp.spawn(_cpu_lsmr_worker, args=(2, _free_port(), name, out), nprocs=2, join=True)
  r = np.load(out)
  g, rig = load_golden(name)
  hm = HostMath(mirror(rig))
  J = hm.jacobian(r["x"])
  A = abs(J)
  assert np.abs(r["jv"] - J @ r["v"]).max() <= 1e-12 * (A @ np.abs(r["v"])).max()
  assert np.abs(r["jtu"] - J.T @ r["u"]).max() <= 1e-12 * (A.T @ np.abs(r["u"])).max()


def _gpu_worker(rank, world, port, name, out, empty_last=False, frames=None):
  sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
  import torch
  import torch.distributed as dist
  from util import sub_rig
  os.environ["MASTER_ADDR"] = "127.0.0.1"
  os.environ["MASTER_PORT"] = str(port)
  torch.cuda.set_device(0)                  # both ranks share the one GPU of the test box (gloo: host-staged sums)
  dist.init_process_group("gloo", rank=rank, world_size=world, timeout=__import__("datetime").timedelta(seconds=180))
  g, rig = load_golden(name)
  if frames is not None:
    rig = sub_rig(rig, frames)
  c = mirror(rig)
  x0 = c.param_vec
  F = rig.valid.shape[1]
  # empty_last: rank 0 owns every frame, the other ranks own nothing (legal: frame_shards does that when F < world)
  h = mdist.sharded_handle(c, shards=[(0, F)] + [(F, F)] * (world - 1) if empty_last else None)
  h.allreduce_stats(reset=True)
  cost, grad, diag = h.normal_equations(x0)
  ne_sizes = h.allreduce_stats(reset=True)[2]
  res = h.solve(x0)
  ar_calls, ar_doubles, ar_sizes = h.allreduce_stats(reset=True)
  e, v = h.reprojection_error(res.x)
  sq = torch.tensor([float((e[v] ** 2).sum()), float(v.sum())], dtype=torch.float64)
  dist.all_reduce(sq)
  if rank == 0:
    np.savez(out, cost=cost, grad=grad, diag=diag, x=res.x, nfev=res.nfev, status=res.status, final_cost=res.cost,
             rms=float(np.sqrt(sq[0] / sq[1])), ar_calls=ar_calls, ar_doubles=ar_doubles, ar_sizes=np.array(ar_sizes),
             njev=res.njev, ne_sizes=np.array(ne_sizes))
  h.close()
  dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("name,empty_last,frames", [("tiny_rolling", False, None), ("tiny_handeye", False, None), ("cfg1", False, None),
                                                    ("tiny_rolling", True, None), ("cfg1", True, None), ("cfg1", False, 12)])
def test_sharded_solve_two_ranks_one_gpu(name, empty_last, frames, tmp_path):
  """empty_last: one rank owns all frames and the other an EMPTY shard -- both must issue the same sequence of
  collectives (the decision to reduce anything may not depend on the local shard size).  frames: the same rig cut to fewer
  frames -- no message of the iteration may depend on the frame count."""
  import torch.multiprocessing as mp
  from multical_amd.backend import Handle
  from util import sub_rig
  out = str(tmp_path / "sharded.npz")
  world = 2
  mp.spawn(_gpu_worker, args=(world, _free_port(), name, out, empty_last, frames), nprocs=world, join=True)
  sh = np.load(out)
  g, rig = load_golden(name)
  if frames is not None:
    rig = sub_rig(rig, frames)
  c = mirror(rig)
  x0 = c.param_vec
  with Handle(c) as h:
    cost, grad, diag = h.normal_equations(x0)
    res = h.solve(x0)
    e, v = h.reprojection_error(res.x)
  assert float(sh["cost"]) == pytest.approx(cost, rel=1e-13)
  assert np.abs(sh["grad"] - grad).max() <= 1e-12 * np.abs(grad).max()
  assert np.abs(sh["diag"] - diag).max() <= 1e-12 * np.abs(diag).max()
  assert int(sh["nfev"]) == res.nfev and int(sh["status"]) == res.status
  assert float(sh["final_cost"]) == pytest.approx(res.cost, rel=1e-10)
  assert abs(float(sh["rms"]) - float(np.sqrt(np.mean(e[v] ** 2)))) < 1e-9
  # (two shards sum H and the partial arrays in a different order than one handle; weakly determined gauge directions
  #  amplify the last-bit differences)
  assert np.abs(sh["x"] - res.x).max() < 1e-7
  # ---- the chain of collectives of the sharded trust-region iteration, in issue order ----------------
  #   G = shared entries of [g | diag] + {cost, count} + step norms (2 ns + 6)  ->  norms + Cauchy curvature per rank (4 W)
  #   ->  reduced Schur system (ns^2 + ns)  ->  dots of the 2-D subspace per rank + pivot flag (3 W + 1)  ->  the next G, which
  #   carries the trial cost and the step norms of the accepted step: FOUR dependent reductions per accepted iteration, NONE
  #   of which grows with the number of frames (round 3: 2 n + 2 and n_motion).  A retry after a rejected step costs one
  #   4-double message; the complete x every rank returns is ONE n_motion message per solve.
  sizes = [int(v) for v in sh["ar_sizes"]]
  n = res.x.size
  motion = rig.cfg["motion"]
  F = rig.valid.shape[1]
  n_motion = {"static": 6, "rolling": 12}.get(motion, 0) * F
  ns = n - n_motion
  G, S, M2, M4 = 2 * ns + 6, ns * ns + ns, 4 * world, 3 * world + 1
  assert int(sh["ar_calls"]) == len(sizes) and int(sh["ar_doubles"]) == sum(abs(v) for v in sizes)
  # host-boundary evaluation: the message of the linearisation, then the frame entries of g and of diag for the CALLER
  assert [int(v) for v in sh["ne_sizes"]] == [G] + ([n_motion, n_motion] if n_motion else [])
  assert sizes[0] == G
  if n_motion:
    assert sizes[-1] == n_motion and sizes.count(n_motion) == (1 if n_motion not in (G, S, M2, M4, 4) else sizes.count(n_motion))
    body = sizes[:-1]
  else:
    body = sizes
  assert set(body) <= {G, S, M2, M4, 4}, sizes                   # nothing else, i.e. nothing that scales with F
  at = [i for i, v in enumerate(body) if v == S]
  assert len(at) >= 1
  for i in at:
    assert body[i - 1] == M2                                   # norms + curvature right before the Schur system
    assert body[i + 1] == M4                                   # dots right behind the back substitution
    assert body[i + 2] == G, sizes                             # speculative linearisation: trial cost + step norms ride along
  # round 4: message 2 of a TRIAL point goes out speculatively right behind its linearisation's message -- also behind that of a
  # step which is then rejected (the retry's 4-double message follows it), where the host used to decide first
  for i, v in enumerate(body[:-1]):
    if v == G and G not in (M2, 4):
      assert body[i + 1] == M2, (i, sizes)
  retries = sum(1 for v in body if v == 4) if 4 not in (M2, M4) else None
  if retries is not None:
    assert retries == res.nfev - 1 - len(at)                   # one 4-double message per RETRY only
  assert body.count(G) >= int(sh["njev"])                      # (+ one per re-linearisation after a rejected step)


def _gpu_lsmr_worker(rank, world, port, name, out, empty_last=False, boards=False):
  sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
  import faulthandler
  faulthandler.dump_traceback_later(240, exit=True)      # a deadlocked collective must end the test with a traceback, not stall it
  import torch
  import torch.distributed as dist
  os.environ["MASTER_ADDR"] = "127.0.0.1"
  os.environ["MASTER_PORT"] = str(port)
  torch.cuda.set_device(0)
  dist.init_process_group("gloo", rank=rank, world_size=world, timeout=__import__("datetime").timedelta(seconds=60))
  from multical_amd import _lib
  _lib.set_switch("MCBA_SOLVE_TRACE", "1")       # per-rank solver lines on stderr: shown when the test fails
  g, rig = load_golden(name)
  c = mirror(rig)
  x0 = c.param_vec
  F = rig.valid.shape[1]
  h = mdist.sharded_handle(c, shards=[(0, F)] + [(F, F)] * (world - 1) if empty_last else None)
  h.set_allreduce_trace(1 << 20)
  h.allreduce_stats(reset=True)
  import json
  kw = json.loads(str(g["ba_kwargs_json"])) if "ba_kwargs_json" in g else {}
  res = h.solve(x0, tr_solver="lsmr", loss=kw.get("loss", "linear"), f_scale=kw.get("f_scale", 1.0))
  ar_calls, ar_doubles, ar_sizes = h.allreduce_stats(reset=True, cap=1 << 20)
  lsmr_itn = h.lsmr_iterations()
  e, v = h.reprojection_error(res.x)
  sq = torch.tensor([float((e[v] ** 2).sum()), float(v.sum())], dtype=torch.float64)
  dist.all_reduce(sq)
  xs = [None] * world
  dist.all_gather_object(xs, res.x)
  if rank == 0:
    np.savez(out, x=res.x, nfev=res.nfev, status=res.status, final_cost=res.cost, rms=float(np.sqrt(sq[0] / sq[1])),
             ar_sizes=np.array(ar_sizes), njev=res.njev, lsmr_itn=lsmr_itn, x_equal=all(np.array_equal(xs[0], xr) for xr in xs))
  h.close()
  dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("name,empty_last,world", [("cfg1", False, 2), ("tiny_rolling", False, 2), ("tiny_handeye", False, 2),
                                                   ("tiny_boards", False, 2), ("cfg1", True, 2), ("cfg1", False, 4), ("tiny_rolling", True, 4),
                                                   ("tiny_softl1", False, 2), ("tiny_fisheye", False, 3)])
def test_sharded_lsmr_solve_ranks_on_one_gpu(name, empty_last, world, tmp_path):
  """solver = "lsmr" on a frame-sharded problem: J v is local, J^T u is a sum over views.  Since round 6 an LSMR iteration
  carries ONE collective of ns + 5 doubles -- [shared sums of J^T uhat | |uhat|^2 | |x|^2 | a | b | c] (k_lsmr_shard_pack2 /
  k_lsmr_shard_finish2) -- and the ranks enqueue iterations in chunks of 8, two chunks ahead, instead of in lockstep.  2 or 4 ranks on
  one GPU (gloo; also with every frame on rank 0 and the other shards empty) must take the single handle's trust-region trajectory
  (nfev, status) and land on its end point to the resolution LSMR-truncated steps are defined to; every rank returns the same x;
  nothing grows with the number of frames."""
  import torch.multiprocessing as mp
  from multical_amd.backend import Handle
  out = str(tmp_path / "sharded_lsmr.npz")
  mp.spawn(_gpu_lsmr_worker, args=(world, _free_port(), name, out, empty_last), nprocs=world, join=True)
  sh = np.load(out)
  g, rig = load_golden(name)
  c = mirror(rig)
  import json
  kw = json.loads(str(g["ba_kwargs_json"])) if "ba_kwargs_json" in g else {}
  with Handle(c) as h:
    res = h.solve(c.param_vec, tr_solver="lsmr", loss=kw.get("loss", "linear"), f_scale=kw.get("f_scale", 1.0))
    itn = h.lsmr_iterations()
    calls = len(h.lsmr_trace())
    e, v = h.reprojection_error(res.x)
  rms = float(np.sqrt(np.mean(e[v] ** 2)))
  spread = float(np.abs(g["ba_pert_rms"] - g["ba_rms"]).max())
  assert bool(sh["x_equal"])
  assert int(sh["status"]) == res.status
  if name in ("cfg1", "tiny_handeye"):          # reference end point defined to < 1e-6 px: same trajectory, same end point
    assert int(sh["nfev"]) == res.nfev
    assert abs(float(sh["rms"]) - rms) <= 1e-6
    assert float(sh["final_cost"]) == pytest.approx(res.cost, rel=1e-6)
  else:                                         # (the shards sum in another order: the end point moves inside the reference's spread)
    # (flat-valley fixtures: the reference's own perturbed re-runs take different numbers of evaluations -- tiny_fisheye 13 ... 20)
    assert abs(int(sh["nfev"]) - res.nfev) <= max(2, int(np.abs(g["ba_pert_nfev"] - g["ba_nfev"]).max()))
    assert abs(float(sh["rms"]) - rms) <= max(1e-6, 3 * spread)
  # ---- collectives, in issue order --------------------------------------------------------------------------------
  sizes = [int(v) for v in sh["ar_sizes"]]
  n = res.x.size
  F = rig.valid.shape[1]
  n_motion = {"static": 6, "rolling": 12}.get(rig.cfg["motion"], 0) * F
  ns = n - n_motion
  G = 2 * ns + 6
  M = ns + 5                                    # the message of one LSMR iteration
  allowed = {G, 4 * world, 1, ns, 6, 4, M} | ({n_motion} if n_motion else set())
  assert set(sizes) <= allowed, sorted(set(sizes) - allowed)
  # ONE message per LSMR iteration; a call that stops at step s has enqueued (s // 8 + 2) * 8 of them (chunks of 8, two ahead)
  per_iteration = sizes.count(M)
  lsmr_calls = int(sh["njev"]) if int(sh["nfev"]) == res.nfev else None
  assert int(sh["lsmr_itn"]) <= per_iteration <= int(sh["lsmr_itn"]) + 16 * (int(sh["nfev"]) + 1), (per_iteration, int(sh["lsmr_itn"]))
  assert 2 not in sizes                                          # (the [|u|^2, |x|^2] message of round 5 is gone)
  assert sizes.count(ns) <= 2 * res.nfev + 2 if ns != M else True   # the ns-message only in the prologue of a call (A^T b)
  print(f"{name} x {world}: sharded nfev {int(sh['nfev'])} / single {res.nfev}, LSMR iterations {int(sh['lsmr_itn'])} / {itn} in {calls} calls, "
        f"rms {float(sh['rms']):.9f} / {rms:.9f}, {len(sizes)} collectives, {per_iteration} iteration messages")


def _rccl_single_rank_worker(rank, out_path):
  import numpy as np
  from multical_amd.backend import Handle
  g, rig = load_golden("tiny_rolling")
  c = mirror(rig)
  with Handle(c) as h0:
    ref = h0.solve(g["x0"])
  with Handle(c) as h:
    uid = Handle.rccl_unique_id()
    assert len(uid) == 128
    h.rccl_init(uid, 0, 1)
    h.set_shard_root(True)
    cost, grad, diag = h.normal_equations(g["x0"])
    res = h.solve(g["x0"])
    h.rccl_shutdown()
  np.savez(out_path, nfev=[res.nfev, ref.nfev], status=[res.status, ref.status], cost=[res.cost, ref.cost], x=res.x,
           x_ref=ref.x)


@pytest.mark.gpu
def test_native_rccl_single_rank_communicator(tmp_path):
  """The library's own RCCL path (mcba_rccl_*): a one-rank communicator on this GPU; every reduction of the sharded
  driver then goes through ncclAllReduce on the handle's stream and the solve must equal the plain single-GPU solve
  (same tolerance as the two-rank test).  Runs in a fresh process: RCCL's communicator bootstrap is sensitive to what the
  calling process has done to the device before (it failed behind a long pytest session, not in a fresh interpreter)."""
  import torch.multiprocessing as mp
  out = str(tmp_path / "rccl1.npz")
  mp.spawn(_rccl_single_rank_worker, args=(out,), nprocs=1, join=True)
  r = np.load(out)
  assert r["nfev"][0] == r["nfev"][1] and r["status"][0] == r["status"][1]
  assert r["cost"][0] == pytest.approx(r["cost"][1], rel=1e-10)
  assert np.abs(r["x"] - r["x_ref"]).max() < 1e-7


def _rccl_one_gpu_worker(rank, world, port, out):
  sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
  import faulthandler
  faulthandler.dump_traceback_later(150, exit=True)
  import torch
  import torch.distributed as dist
  os.environ["MASTER_ADDR"] = "127.0.0.1"
  os.environ["MASTER_PORT"] = str(port)
  torch.cuda.set_device(0)                  # BOTH ranks on the one GPU of the test box
  dist.init_process_group("gloo", rank=rank, world_size=world, timeout=__import__("datetime").timedelta(seconds=60))
  g, rig = load_golden("cfg1")
  c = mirror(rig)
  h = mdist.sharded_handle(c, native=True)  # asks for the library's own RCCL communicator; falls back to the hook if any rank fails
  res = h.solve(c.param_vec)
  if rank == 0:
    np.savez(out, native=bool(h.native_allreduce), nfev=res.nfev, status=res.status, cost=res.cost)
  h.close()
  dist.destroy_process_group()


@pytest.mark.gpu
def test_native_rccl_with_two_ranks_on_one_gpu_falls_back_or_works(tmp_path):
  """The native RCCL path has only ever run with ONE rank (one GPU per test box).  Two ranks on the SAME device: RCCL (NCCL 2.x ABI)
  refuses a communicator whose ranks share a GPU ("duplicate GPU"), so `init_native_allreduce` must report failure on EVERY rank
  (MIN over the success flags) and the handle must fall back to the torch.distributed hook -- the solve still matches the single
  handle.  Should a future RCCL accept it, the native path must produce the same solve.  Either way: no hang, no silent divergence."""
  import torch.multiprocessing as mp
  from multical_amd.backend import Handle
  out = str(tmp_path / "rccl_one_gpu.npz")
  mp.spawn(_rccl_one_gpu_worker, args=(2, _free_port(), out), nprocs=2, join=True)
  sh = np.load(out)
  g, rig = load_golden("cfg1")
  c = mirror(rig)
  with Handle(c) as h:
    res = h.solve(c.param_vec)
  print("native RCCL with two ranks on one device:", "accepted" if bool(sh["native"]) else "refused -> torch.distributed hook")
  assert int(sh["nfev"]) == res.nfev and int(sh["status"]) == res.status
  assert float(sh["cost"]) == pytest.approx(res.cost, rel=1e-10)


def _rccl_world_worker(rank, world, port, name, out):
  sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
  import torch
  import torch.distributed as dist
  os.environ["MASTER_ADDR"] = "127.0.0.1"
  os.environ["MASTER_PORT"] = str(port)
  torch.cuda.set_device(rank)
  dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
  g, rig = load_golden(name)
  c = mirror(rig)
  h = mdist.sharded_handle(c)               # backend nccl -> the library's own RCCL communicator
  assert h.native_allreduce, "native RCCL initialisation failed"
  cost, grad, diag = h.normal_equations(g["x0"])
  res = h.solve(g["x0"])
  e, v = h.reprojection_error(res.x)
  sq = torch.tensor([float((e[v] ** 2).sum()), float(v.sum())], dtype=torch.float64, device="cuda")
  dist.all_reduce(sq)
  if rank == 0:
    np.savez(out, cost=cost, grad=grad, diag=diag, x=res.x, nfev=res.nfev, status=res.status, final_cost=res.cost,
             rms=float(torch.sqrt(sq[0] / sq[1]).item()))
  h.close()
  dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny_rolling", "cfg1"])
def test_native_rccl_two_gpus(name, tmp_path):
  """one rank per GPU over xGMI: the library's own RCCL communicator (mcba_rccl_*) with world_size 2.  Needs two visible
  GPUs: skipped on the single-GPU test box, exercised by the driver's 8-GPU node."""
  import torch
  if torch.cuda.device_count() < 2:
    pytest.skip("needs two GPUs")
  import torch.multiprocessing as mp
  from multical_amd.backend import Handle
  out = str(tmp_path / "rccl2.npz")
  mp.spawn(_rccl_world_worker, args=(2, _free_port(), name, out), nprocs=2, join=True)
  sh = np.load(out)
  g, rig = load_golden(name)
  with Handle(mirror(rig)) as h:
    cost, grad, diag = h.normal_equations(g["x0"])
    res = h.solve(g["x0"])
  assert float(sh["cost"]) == pytest.approx(cost, rel=1e-13)
  assert np.abs(sh["grad"] - grad).max() <= 1e-12 * np.abs(grad).max()
  assert int(sh["nfev"]) == res.nfev and int(sh["status"]) == res.status
  assert float(sh["final_cost"]) == pytest.approx(res.cost, rel=1e-10)
  assert np.abs(sh["x"] - res.x).max() < 1e-7


def _run_bench(extra_env, *args, timeout=900):
  import subprocess
  env = dict(os.environ)
  env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
  env.update(extra_env)
  return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), env=env, capture_output=True,
                        text=True, timeout=timeout, cwd=ROOT)


def test_bench_self_launches_its_ranks_and_fails_loudly_without_a_gpu():
  """`python bench.py --gpus 2` with no launcher around it must start its own ranks (torch.distributed.run on the
  loopback address).  On the GPU-less build box every rank then stops with the product's own message -- there is no CPU
  path -- and the launcher returns non-zero."""
  from util import gpu_available
  if gpu_available():
    pytest.skip("GPU box: covered by test_bench_two_ranks_on_one_gpu")
  r = _run_bench({"MCBA_BENCH_BACKEND": "gloo"}, "--gpus", "2", "--steps", "2", "--warmup", "1", "--no-cpu-baseline")
  assert r.returncode != 0
  assert "[bench rank 0/2]" in r.stderr and "[bench rank 1/2]" in r.stderr, r.stderr[-2000:]
  assert "GPU-only" in r.stderr
  assert not r.stdout.strip().startswith("{")                      # no JSON line from a run that measured nothing


@pytest.mark.gpu
def test_bench_two_ranks_on_one_gpu():
  """The N > 1 path of bench.py end to end, self-launched (no torchrun on the command line): two ranks share the one
  GPU of the test box with host-staged gloo all-reduces.  `value` must be evaluations/s of the FIXED 8 x 500 x 2 rig of the north
  star (250 frames per rank, "scaling": "strong"), the weak-scaling figure rides along, and `parity_route` -- the lsmr solve of
  the frame-sharded rig -- lands on the committed end point of the unmodified reference."""
  import json
  r = _run_bench({"MCBA_BENCH_BACKEND": "gloo"}, "--gpus", "2", "--steps", "5", "--warmup", "2", "--repeats", "2",
                 "--no-cpu-baseline", "--full")
  assert r.returncode == 0, r.stderr[-3000:]
  assert "[bench rank 0/2]" in r.stderr and "[bench rank 1/2]" in r.stderr and "native_rccl=false" in r.stderr
  line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
  out = json.loads(line)
  assert out["n_gpus"] == 2 and out["steps"] == 5 and out["warmup"] == 2 and out["scaling"] == "strong"
  assert out["metric"] == "residual+Jacobian evals/sec" and out["dtype"] == "f64" and out["value"] > 0
  assert out["config"]["n_observations"] == 763957 and out["config"]["native_rccl"] is False
  assert "[250, 250]" in out["config"]["parallelism"] and "gloo" in out["config"]["parallelism"]
  assert out["weak_scaling"]["frames_per_gpu"] == 500 and out["weak_scaling"]["value"] > 0
  assert out["roofline"]["frac"] > 0 and out["obs_per_s"] > 0 and 0 < out["step_roofline_frac"] < 1
  assert 2.5 < out["final_rms_px"] < 3.5                     # 1 % gross outliers stay in: ~3 px (single GPU: 3.03)
  pr = out["parity_route"]
  assert pr["solver"] == "lsmr" and pr["nfev"] == pr["reference_nfev"] and pr["status"] == pr["reference_status"]
  assert pr["abs_delta_px"] <= max(1e-6, 3 * (pr["reference_spread_px"] or 0.0)), pr


def test_bench_refuses_ranks_that_share_a_device(monkeypatch):
  """backend nccl with more ranks than visible GPUs = ranks silently sharing a device: bench.py must exit non-zero (no JSON line).
  Runs wherever fewer than two GPUs are visible (build box: 0 -> the GPU-only exit; single-GPU test box: the sharing exit)."""
  import torch
  if torch.cuda.device_count() >= 2:
    pytest.skip("two GPUs visible")
  r = _run_bench({}, "--gpus", "2", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-solve")
  assert r.returncode != 0
  assert "refusing to measure" in r.stderr or "GPU-only" in r.stderr, r.stderr[-2000:]
  assert not r.stdout.strip().startswith("{")


def _cpu_one_message_worker(rank, world, port, name, out):
  """One LSMR solve of the frame-sharded default solver, walked through on the CPU: the rank's rows of J through the product's device
  functions (tests/hostmath), the scalar recurrences of csrc/mcba_lsmr.h, and per iteration ONE gloo all-reduce of the message
  [shared sums of J^T uhat | |uhat|^2 | |x|^2 | a | b | c] (csrc/mcba_solver_kernels.h: k_lsmr_shard_pack2 / k_lsmr_shard_finish2)."""
  sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
  import torch
  import torch.distributed as dist
  from hostmath_lib import HostMath
  from lsmr_emulation import LsmrState
  os.environ["MASTER_ADDR"] = "127.0.0.1"
  os.environ["MASTER_PORT"] = str(port)
  dist.init_process_group("gloo", rank=rank, world_size=world)

  def allsum(a):
    t = torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1).copy())
    dist.all_reduce(t)
    return t.numpy()
  g, rig = load_golden(name)
  c = mirror(rig)
  F = rig.valid.shape[1]
  shards = mdist.frame_shards(F, world - 1, c.inliers.sum(axis=(0, 2, 3)).astype(float)) + [(F, F)]     # the last rank owns NOTHING
  f0, f1 = shards[rank]
  hm = HostMath(c, frame_range=(f0, f1))
  x0 = g["x0"]
  n = x0.size
  J, f = hm.jacobian(x0), hm.residuals(x0)                      # this rank's rows
  # parameter layout: camera_poses | board_poses | motion | cameras ...: the frame entries are the motion block (static 6 F, rolling 2 x 6 F)
  per = {"static": 6, "rolling": 12}[rig.cfg["motion"]]
  C_, B_ = rig.valid.shape[0], rig.valid.shape[2]
  off = 6 * C_ + 6 * B_
  frame_of = np.full(n, -1)
  for blk in range(per // 6):
    for fr in range(F):
      frame_of[off + blk * 6 * F + 6 * fr: off + blk * 6 * F + 6 * fr + 6] = fr
  shared = frame_of < 0
  own = (frame_of >= f0) & (frame_of < f1)
  weight = np.where(shared, 1.0 if rank == 0 else 0.0, own.astype(float))      # Dims::entry_weight
  col2 = np.asarray(J.power(2).sum(axis=0)).ravel()
  col2[shared] = allsum(col2[shared])                            # (the linearisation's message carries the shared part of diag)
  si = np.sqrt(np.where(shared | own, col2, 1.0))
  si[si == 0] = 1
  d = 1 / si
  damp = 0.02
  JT = J.T.tocsr()

  def jtu_raw(u):                                                # raw sums over THIS rank's views, own-frame + shared entries
    return JT @ u
  # ---- prologue (lsmr_solve): collectives as the device issues them there (not per iteration)
  normb = float(np.sqrt(allsum([f @ f])[0]))
  u = f / normb
  s = jtu_raw(u)
  s[shared] = allsum(s[shared])
  v = np.where(shared | own, d * s, 0.0)
  alpha = float(np.sqrt(allsum([np.sum(weight * v * v)])[0]))
  v = v / alpha
  st = LsmrState()
  st.init(alpha, normb, damp, normb, float(min(int(allsum([f.size])[0]), n)))
  h, hbar, x = v.copy(), np.zeros(n), np.zeros(n)
  vstore, uhat, pending, vsq, messages = v, u, False, 0.0, 0
  trace = []
  while True:
    # k_lsmr_fused2: head (alpha from the |v_raw|^2 the last finish formed), product, tail
    alpha, inv_alpha, inv_beta_old = st.slot("alpha"), st.slot("inv_alpha"), st.slot("inv_beta")
    if pending:
      inv_alpha = 1.0
      if st.slot("skipv") == 0.0:
        alpha = np.sqrt(vsq)
        inv_alpha = 1.0 / alpha if alpha > 0 else 1.0
    vn = vstore * inv_alpha
    uhat = J @ (d * vn) - alpha * (uhat * inv_beta_old)
    if pending:
      st.rotate(vsq)
      hbar = st.slot("c_hbar") * hbar + h
      x = x + st.slot("c_x") * hbar
      h = st.slot("c_h") * h + vstore * st.slot("inv_alpha")
    # k_lsmr_gather3 (raw sums) + k_lsmr_shard_pack2
    s = jtu_raw(uhat)
    t = d * s
    msg = np.concatenate([s[shared], [uhat @ uhat, np.sum(weight * x * x), np.sum((t * t)[own]), np.sum((t * vn)[own]), np.sum((vn * vn)[own])]])
    msg = allsum(msg)                                            # THE collective of this iteration
    messages += 1
    # k_lsmr_shard_finish2
    ns = int(shared.sum())
    u2, x2, a, b, cc = msg[ns:]
    istop = st.test(x2) if st.slot("itn") > 0 else 0
    if istop != 0:
      break
    st.beta(u2)
    beta, inv_beta = st.slot("beta"), st.slot("inv_beta")
    vraw = np.zeros(n)
    vraw[shared] = d[shared] * (msg[:ns] * inv_beta) - beta * vn[shared]
    vraw[own] = d[own] * (s[own] * inv_beta) - beta * vn[own]
    vsq = float(np.sum(vraw[shared] ** 2) + max((a * inv_beta) * inv_beta - 2.0 * b + (beta * beta) * cc, 0.0))
    exact = float(allsum([np.sum(weight * vraw * vraw)])[0])     # (what round 5 spent a third collective on: only compared here)
    trace.append(abs(vsq - exact) / exact)
    vstore, pending = vraw, True
  # the complete solution: shared entries are replicated, frame entries live with their owner
  xs = np.where(shared, x if rank == 0 else 0.0, np.where(own, x, 0.0))
  x_full = allsum(xs)
  d_full = allsum(np.where(shared, d if rank == 0 else 0.0, np.where(own, d, 0.0)))
  states = [None] * world
  dist.all_gather_object(states, (st.L.tobytes(), x[shared].tobytes()))
  if rank == 0:
    np.savez(out, x=x_full, istop=istop, itn=int(st.slot("itn")), messages=messages, identical=all(s_ == states[0] for s_ in states),
             vsq_err=max(trace), d=d_full, damp=damp)
  dist.destroy_process_group()


@pytest.mark.parametrize("name", ["cfg1", "tiny_rolling"])
def test_one_message_lsmr_iteration_gloo_world_4(name, tmp_path):
  """The protocol of the frame-sharded default solver since round 6 -- ONE all-reduce per LSMR iteration, |v_raw|^2 recovered from
  a / beta^2 - 2 b + beta^2 c -- on the CPU with a world-size-4 gloo group whose last rank owns an EMPTY shard: the solve stops for scipy's
  reason within two iterations of scipy's count on the whole Jacobian, lands on scipy's solution, one message per iteration (+ the one that
  carries the stop), the recovered |v_raw|^2 equals the directly summed one to 1e-12, and state + shared entries are bit-identical on all
  ranks (what lets every rank take the same stopping / chunk decisions)."""
  import torch.multiprocessing as mp
  from scipy.sparse.linalg import lsmr
  from hostmath_lib import HostMath
  from lsmr_emulation import scaled_operator
  out = str(tmp_path / "one_message.npz")
  mp.spawn(_cpu_one_message_worker, args=(4, _free_port(), name, out), nprocs=4, join=True)
  r = np.load(out)
  g, rig = load_golden(name)
  hm = HostMath(mirror(rig))
  J, f = hm.jacobian(g["x0"]), hm.residuals(g["x0"])
  si = np.asarray(J.power(2).sum(axis=0)).ravel() ** 0.5
  si[si == 0] = 1
  assert np.abs(r["d"] * si - 1).max() <= 1e-12
  ref = lsmr(scaled_operator(J, 1 / si), f, damp=float(r["damp"]))
  assert bool(r["identical"])
  assert int(r["istop"]) == ref[1] and abs(int(r["itn"]) - ref[2]) <= 2, (int(r["istop"]), int(r["itn"]), ref[1:3])
  assert int(r["messages"]) == int(r["itn"]) + 1
  assert float(r["vsq_err"]) <= 1e-12
  Jh = J @ __import__("scipy.sparse", fromlist=["diags"]).diags(1 / si)
  objective = lambda p: 0.5 * (np.sum((f - Jh @ p) ** 2) + float(r["damp"]) ** 2 * (p @ p))
  # the same damped problem solved to the same level (a call that runs into maxiter, istop 7, is not converged: tiny_rolling)
  assert abs(objective(r["x"]) - objective(ref[0])) <= (1e-9 if ref[1] in (1, 2) else 1e-4) * objective(ref[0])
  if name == "cfg1":                                                                     # (well conditioned: the solutions coincide)
    assert np.linalg.norm(r["x"] - ref[0]) <= 1e-5 * np.linalg.norm(ref[0])


def test_bench_dry_run_eight_ranks_gloo():
  """`python bench.py --gpus 8 --config cfg4 --dry-run` on the GPU-less box: the launcher the driver uses, eight gloo ranks on the
  loopback address, the frame-shard plan of BASELINE configs[3] (cut to 14 frames: seven ranks with one to three frames each, balanced by inlier count, and one EMPTY shard),
  one all-reduce of 2 n_s + 6 doubles per step with the real message layout, barrier + MAX-over-ranks timing, the watchdog armed, ONE JSON
  line from rank 0 -- and the reduced [g | diag | cost, count] equal to the unsharded evaluation.  (The 8-GPU run itself is the driver's.)"""
  import json
  r = _run_bench({}, "--gpus", "8", "--config", "cfg4", "--dry-run", "--steps", "2", "--warmup", "1", timeout=600)
  assert r.returncode == 0, r.stderr[-3000:]
  for k in range(8):
    assert f"[bench rank {k}/8] dry run" in r.stderr
  lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
  assert len(lines) == 1
  out = json.loads(lines[0])
  assert out["dry_run"] is True and out["n_gpus"] == 8 and out["steps"] == 2 and out["warmup"] == 1 and out["scaling"] == "strong"
  assert out["metric"] == "residual+Jacobian evals/sec" and out["dtype"] == "f64"
  counts = out["config"]["observations_per_rank"]
  assert len(counts) == 8 and counts[-1] == 0 and all(c > 0 for c in counts[:-1])
  plan = json.loads(out["config"]["parallelism"].split("(")[1].split(" frames")[0])
  assert len(plan) == 8 and sum(plan) == 14 and plan[-1] == 0 and min(plan[:-1]) >= 1     # balanced by inlier count; the last shard is empty
  ns = out["config"]["n_shared"]
  assert out["step_collectives"]["message_doubles"] == [2 * ns + 6]
  assert out["reduced_message_rel_error"] <= 1e-12
