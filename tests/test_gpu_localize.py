"""mcba_rig_poses on the device (k_rig_pose) against the g++ build of the same header (localize_host_lib): equal statuses, observation
counts and NaN / identity slots, poses within 1e-8 px of whitened distance (100 x the stop rule: both sides stop within 1e-10 px of
the optimum, and the device contracts to FMAs while the host build does not), covariances to 1e-6 relative, sse and per-slot errors
to 1e-8; and against the bundle adjustment, whose per-frame optimum a localisation of the same table must reach.

A frame's solution depends on every observation of the frame, so the host build runs once per (rig, size); it takes milliseconds."""
import ctypes as C
import functools

import numpy as np
import pytest

from multical_amd import _lib, localize

import localize_host_lib as lh

pytestmark = pytest.mark.gpu

N_EDGES = [3, 4, 63, 64, 65, 255, 256, 257, 513]      # lane, wave-chunk and workgroup-pass edges
KEYS = ("poses", "poses_end", "cov", "sse", "n_obs", "iters", "error", "status")


_figures = []


def note(line):
  print(line)
  _figures.append(line)


def tobytes(r, k):
  return b"" if r[k] is None else np.ascontiguousarray(r[k]).tobytes()


def compare(got, want, label, valid):
  """valid [C,F,B,P]: the observations of the call"""
  assert np.array_equal(got.status, want.status) and np.array_equal(got.n_obs, want.n_obs), (label, got.status, want.status)
  assert np.array_equal(np.isnan(got.cov), np.isnan(want.cov)) and got.error.shape == want.error.shape, label
  none = (got.status == localize.TOO_FEW) | (got.status == localize.DEGENERATE)
  assert np.array_equal(got.poses[none], np.broadcast_to(np.eye(4), got.poses[none].shape)) and (got.sse[none] == 0).all(), label
  assert (got.poses_end is None) == (want.poses_end is None)
  # errors are 0 where nothing entered: outside the call's observations and in frames without a result.  (Where an observation did
  # enter, an error may be 0 too: three observations determine a static pose exactly, and a residual then rounds to 0 on one side.)
  entered = np.asarray(valid, dtype=bool) & ~none[None, :, None, None]
  assert (got.error[~entered] == 0).all() and (want.error[~entered] == 0).all(), label
  ok = got.status == localize.OK
  result = ~none & ~ok
  p, q = lh.result_params(got), lh.result_params(want)
  if result.any():   # (the last iterate of a frame that did not converge: the stop rule says nothing about its pose -- printed; its
    #                    sse and errors are held to the same 1e-8 as a converged frame's)
    d_sse, d_err = np.abs(got.sse - want.sse)[result].max(), np.abs(got.error - want.error)[:, result].max()
    print(f"{label}: frames without convergence {np.nonzero(result)[0]}, parameter difference {np.abs(p - q)[result].max():.2e}, "
          f"sse {d_sse:.2e} px^2, err {d_err:.2e} px")
    assert d_sse <= 1e-8 and d_err <= 1e-8, label
  if not ok.any():
    return 0.0
  finite = ok & np.isfinite(want.cov).all(axis=(1, 2))
  H = np.linalg.inv(want.cov[finite])                    # sigma = 1: inv(cov) is J^T J
  dist = lh.whitened(H, (p - q)[finite]).max() if finite.any() else 0.0
  cov = (np.abs(got.cov[finite] - want.cov[finite]).max(axis=(1, 2)) / np.abs(want.cov[finite]).max(axis=(1, 2))).max() if finite.any() else 0.0
  sse, err = np.abs(got.sse - want.sse)[ok].max(), np.abs(got.error - want.error)[:, ok].max()
  print(f"{label}: {int(ok.sum())} of {ok.size} frames OK; whitened distance {dist:.2e} px, cov {cov:.2e} relative, sse {sse:.2e} px^2, "
        f"err {err:.2e} px, iterations {got.iters[ok].max()} / {want.iters[ok].max()}")
  assert dist <= 1e-8 and cov <= 1e-6 and sse <= 1e-8 and err <= 1e-8, label
  return dist


@pytest.mark.parametrize("n", N_EDGES)
def test_device_matches_host_build(n):
  """C in {1, 3, 8}, F in {1, 3}, static and rolling shutter, with and without init, the first n observations of every frame of the
  edge rig (localize_host_lib.dense_rig: well posed at every n, crossing from camera to camera past 576 / C observations).  Frames
  that converge -- and so stand under the 1e-8 px bound -- are required of the static AND of the rolling cases at every n; only
  rolling shutter at n = 3 and 4 has none, by definition (fewer than 6 observations: TOO_FEW)."""
  n_ok, worst = {False: 0, True: 0}, 0.0
  for Cn in (1, 3, 8):
    for F in (1, 3):
      for rolling in (False, True):
        rig = lh.keep_first(lh.dense_rig(Cn, F, rolling), n)
        cams_used = int(rig.valid.any(axis=(1, 2, 3)).sum())
        assert cams_used == min(Cn, -(-n // (576 // Cn))), (Cn, n, cams_used)      # the records do index more than camera 0
        for init in (False, True):
          kw = dict(sigma=1.0)
          if init:
            kw.update(init=rig.rig_poses, init_end=rig.rig_poses_end)
          got, want = lh.run(rig, backend="device", **kw), lh.run(rig, **kw)
          assert (got.n_obs == n).all()
          label = f"C={Cn} F={F} n={n}{' rolling' if rolling else ''}{' init' if init else ''}"
          worst = max(worst, compare(got, want, label, rig.valid))
          ok = got.status == localize.OK
          n_ok[rolling] += int(ok.sum())
          if n >= 63:      # (from one wave chunk on, every start reaches the optimum within the default 20 linearisations)
            assert ok.all(), (label, got.status, got.iters)
          ms, count = localize.last_call_ms()
          assert count == F and ms["kernel"] > 0.0 and ms["call"] >= ms["kernel"]
  note(f"device vs host build, first {n} observations a frame: {n_ok[False]} static and {n_ok[True]} rolling frames OK, largest whitened pose "
       f"distance {worst:.2e} px")
  assert n_ok[False] > 0 and (n_ok[True] > 0 or n < 6)


def test_sixteen_cameras_and_five_boards_in_one_frame():
  rig = lh.dense_rig(16, 1, False, boards=5, share=False)
  got, want = lh.run(rig, backend="device", sigma=1.0), lh.run(rig, sigma=1.0)
  assert (got.status == localize.OK).all() and got.n_obs[0] > 1500
  note(f"16 cameras x 5 boards in one frame ({got.n_obs[0]} observations): whitened pose distance {compare(got, want, 'C=16 B=5 F=1', rig.valid):.2e} px")
  # the automatic sigma and the cap are the host build's too
  auto, auto_want = lh.run(rig, backend="device"), lh.run(rig)
  assert (np.abs(auto.cov - auto_want.cov).max(axis=(1, 2)) / np.abs(auto_want.cov).max(axis=(1, 2))).max() <= 1e-6
  one, one_want = lh.run(rig, backend="device", max_iterations=1), lh.run(rig, max_iterations=1)
  assert (one.status == localize.NOT_CONVERGED).all() and np.abs(lh.result_params(one) - lh.result_params(one_want)).max() <= 1e-9
  lib = _lib.load()
  p, out, keep = lh.raw_problem(lh.dense_rig(3, 1, False), n_cameras=localize.MAX_CAMERAS + 1)
  assert lh.raw_call(lib.mcba_rig_poses, p, out) == 1 and b"at most 64" in lib.mcba_last_error()


def test_repeatable_and_scaffold():
  rig = lh.dense_rig(8, 3, True)
  a, b = lh.run(rig, backend="device"), lh.run(rig, backend="device")
  for k in KEYS:
    assert tobytes(a, k) == tobytes(b, k), k
  ms, count = localize.last_call_ms()
  assert count == 3 and ms["kernel"] > 0.0 and ms["start_kernel"] > 0.0
  # F == 0 launches nothing
  empty = localize.localize_rig(rig.cameras, rig.camera_poses, rig.board_poses, rig.board_points, rig.points[:, :0], rig.valid[:, :0],
                                rolling=True)
  assert empty.poses.shape == (0, 4, 4) and empty.cov.shape == (0, 12, 12)
  ms, count = localize.last_call_ms()
  assert count == 0 and ms["kernel"] == 0.0 and ms["start_kernel"] == 0.0
  # a refused call leaves its message and nothing else behind
  lib = _lib.load()
  small = lh.dense_rig(3, 1, False)
  for label, text in (("points", b"null argument"), ("heights", b"image_heights")):
    p, out, keep = lh.raw_problem(small)
    if label == "points":
      p.points = None
    else:
      p.rolling = 1
    assert lh.raw_call(lib.mcba_rig_poses, p, out) == 1 and text in lib.mcba_last_error(), label
    c = lh.run(rig, backend="device")
    for k in KEYS:
      assert tobytes(c, k) == tobytes(a, k), (label, k)
  # NULL outputs are neither allocated nor copied: poses and status alone are the full call's
  p, out, keep = lh.raw_problem(small)
  assert lh.raw_call(lib.mcba_rig_poses, p, out) == 0
  full = lh.run(small, backend="device")
  assert out.poses.tobytes() == full.poses.tobytes() and out.status.tobytes() == full.status.tobytes()


# ---- the Calibration built over localised frames ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "tiny_rolling", "tiny_handeye"])
def test_a_calibration_over_localised_frames_works_unchanged(name, caplog):
  """with_localized_frames(calib.point_table) at the fixture's truth parameters: the same masks, a reprojection RMS no higher than
  the calibration's own (localising can only lower each frame's cost), report() and a bundle adjustment run on it; a HandEye
  calibration yields StaticFrames"""
  import logging
  import pnp_host_lib
  from multical_amd import calibration
  calib = calibration.from_rig(pnp_host_lib.golden_rig(name), "truth")
  held = calib.with_localized_frames(calib.point_table)
  assert np.array_equal(held.valid, calib.valid) and held.reprojection_error.shape == calib.reprojection_error.shape
  assert type(held.motion).__name__ == ("RollingFrames" if name == "tiny_rolling" else "StaticFrames")
  own, rms = np.sqrt(np.mean(calib.reprojection_error ** 2)), np.sqrt(np.mean(held.reprojection_error ** 2))
  print(f"{name}: reprojection RMS {own:.9f} px at the fixture's poses, {rms:.9f} px over the localised frames")
  assert rms <= own * (1.0 + 1e-12)
  with caplog.at_level(logging.INFO, logger="calibration"):
    held.report("held-out:")
    calib.report_holdout(calib.point_table, "golden:")
  assert any("held-out: reprojection RMS=" in m for m in caplog.messages) and sum("frames localised" in m for m in caplog.messages) == 1
  again = held.enable(cameras=False, boards=False, camera_poses=False, board_poses=True, motion=True).bundle_adjust(solver="native")
  assert np.sqrt(np.mean(again.reprojection_error ** 2)) <= rms * (1.0 + 1e-9)


# ---- consistency with the bundle adjustment -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def adjusted(name):
  import pnp_host_lib
  from multical_amd import calibration, synthetic
  rig = pnp_host_lib.golden_rig(name) if name.startswith("tiny") else synthetic.make_rig(name)
  calib = calibration.from_rig(rig, "init")
  return calib.bundle_adjust(tolerance=1e-15, xtol=1e-15, gtol=1e-15, max_iterations=300, loss="linear", solver="native")


@pytest.mark.parametrize("name", ["tiny", "tiny_rolling", "cfg1"])
def test_localising_the_adjusted_table_reaches_the_bundle_adjustment(name):
  """the bundle adjustment at tight tolerance leaves every frame at the optimum of its own block: localising the same table from
  scratch (no init) ends there too -- per-frame sse no higher, the overall RMS the same to 1e-9 px"""
  calib = adjusted(name)
  err, mask = calib._errors()
  err = np.where(mask, err, 0.0)
  ba_sse = np.moveaxis(err ** 2, 1, 0).reshape(calib.size.rig_poses, -1).sum(axis=1)
  r = calib.localize(calib.point_table)
  seen = np.moveaxis(mask, 1, 0).reshape(calib.size.rig_poses, -1).sum(axis=1)
  assert np.array_equal(r.n_obs, seen) and (r.status[seen > 0] == localize.OK).all()
  start, end = calib._rig_poses()
  ba = lh.params(start) if end is None else np.concatenate([lh.params(start), lh.params(end)], axis=1)
  full = localize.localize_rig(calib.cameras, calib.camera_poses.poses, calib.board_poses.poses,
                               [np.asarray(b.adjusted_points) for b in calib.boards], calib.point_table.points, mask, rolling=end is not None,
                               sigma=1.0)
  live = seen > 0
  dist = lh.whitened(np.linalg.inv(full.cov[live]), (lh.result_params(full) - ba)[live])
  n = seen.sum()
  rms, ba_rms = np.sqrt(r.sse.sum() / n), np.sqrt(ba_sse.sum() / n)
  worst = (r.sse[live] / ba_sse[live]).max()
  note(f"{name}: {int(live.sum())} frames, RMS {rms:.12f} px localised, {ba_rms:.12f} px adjusted; largest sse ratio {worst:.3e}, largest whitened "
        f"pose distance {dist.max():.2e} px")
  assert (r.sse[live] <= ba_sse[live] * (1.0 + 1e-9)).all()
  assert abs(rms - ba_rms) <= 1e-9


def test_zz_write_profile():
  """(not a check) MCBA_WRITE_PROFILES=1: the figures the tests above measured go to profiles/rig_pose_device_parity.txt"""
  import os
  if os.environ.get("MCBA_WRITE_PROFILES") and _figures:
    root = os.path.dirname(lh.HERE)
    with open(os.path.join(root, "profiles", "rig_pose_device_parity.txt"), "w") as fh:
      fh.write("Rig localisation: k_rig_pose against the g++ build of csrc/mcba_localize.h and against the bundle adjustment "
               "(tests/test_gpu_localize.py, MI355X)\n")
      fh.write("\n".join(_figures) + "\n")
