"""The rig localisation mathematics (csrc/mcba_localize.h) in its g++ build, against an independent numpy / scipy restatement
(localize_reference.py), and the Python layer on top of it (multical_amd.localize, Calibration.localize / with_localized_frames /
report_holdout) driven through that build.  No GPU.

MCBA_WRITE_PROFILES=1 writes the measured figures to profiles/rig_pose_parity.txt."""
import functools
import logging
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest

from multical_amd import localize

import host_build
import localize_host_lib as lh
import localize_reference as lr

ROOT = os.path.dirname(lh.HERE)
SIGMA = lh.NOISE_PX
_figures = []


def note(line):
  print(line)
  _figures.append(line)


def truth_params(rig):
  t = lh.params(rig.rig_poses)
  return np.concatenate([t, lh.params(rig.rig_poses_end)], axis=1) if rig.rolling else t


@pytest.mark.parametrize("name", lh.RIG_IDS)
def test_noise_free_observations_give_the_truth(name):
  """started without init: every frame is OK and ends within 1e-9 px (whitened: sqrt(d^T J^T J d)) of the truth"""
  rig = lh.named_rig(name, noise=0.0)
  got = lh.run(rig, sigma=1.0)                   # sigma = 1: inv(cov) is J^T J
  assert (got.status == localize.OK).all() and (got.n_obs == np.moveaxis(rig.valid, 1, 0).reshape(len(got.status), -1).sum(axis=1)).all()
  d = lh.whitened(np.linalg.inv(got.cov), lh.result_params(got) - truth_params(rig))
  note(f"noise-free {name}: {rig.shape}, {got.n_obs.min()}..{got.n_obs.max()} observations a frame, whitened distance to the truth "
       f"<= {d.max():.2e} px, sse <= {got.sse.max():.2e} px^2, <= {got.iters.max()} linearisations")
  assert d.max() <= 1e-9


@functools.lru_cache(maxsize=None)
def solved(name):
  """rig `name` with 0.2 px noise once for every test: the host build's result from the truth as `init` and without init, and the
  restatement's optimum from the truth and from the truth perturbed by 1e-9"""
  rig = lh.named_rig(name)
  F = rig.shape[1]
  init = dict(init=rig.rig_poses, init_end=rig.rig_poses_end)
  got, scratch = lh.run(rig, sigma=SIGMA, **init), lh.run(rig, sigma=SIGMA)
  frames = [lr.Frame(rig, f) for f in range(F)]
  rng = np.random.default_rng(7)
  a, b = [], []
  for f, fr in enumerate(frames):
    x0 = lr.start_vector(rig, f)
    a.append(fr.solve(x0))
    b.append(fr.solve(x0 + rng.normal(0.0, 1e-9, x0.shape)))
  J = [fr.jacobian(r.x) for fr, r in zip(frames, a)]
  H = np.stack([j.T @ j for j in J])
  return SimpleNamespace(rig=rig, got=got, scratch=scratch, frames=frames, x=np.stack([r.x for r in a]), x2=np.stack([r.x for r in b]),
                         sse=np.array([2.0 * r.cost for r in a]), H=H, ok=[r.success for r in a])


@pytest.mark.parametrize("name", lh.RIG_IDS)
def test_distance_to_the_restatements_optimum(name):
  """no frame is skipped: the restatement converges on every one, and the host build ends within max(1e-9, 100 x the restatement's
  own spread between two starts) of it in whitened pixels -- from the truth as init and from its own views alike"""
  s = solved(name)
  assert all(s.ok) and all(fr.n >= 6 for fr in s.frames)
  assert (s.got.status == localize.OK).all() and (s.scratch.status == localize.OK).all()
  spread = lh.whitened(s.H, s.x - s.x2).max()
  dist = lh.whitened(s.H, lh.result_params(s.got) - s.x).max()
  scratch = lh.whitened(s.H, lh.result_params(s.scratch) - s.x).max()
  note(f"noisy {name}: whitened distance to the restatement's optimum {dist:.2e} px (init) {scratch:.2e} px (own views); its spread between "
       f"two starts {spread:.2e} px; <= {max(s.got.iters.max(), s.scratch.iters.max())} linearisations")
  assert dist <= max(1e-9, 100.0 * spread) and scratch <= max(1e-9, 100.0 * spread)


@pytest.mark.parametrize("name", lh.RIG_IDS)
def test_covariance_sse_and_errors(name):
  s = solved(name)
  inv = np.linalg.inv(s.H)
  scale = np.abs(inv).max(axis=(1, 2))
  assert np.array_equal(s.got.cov, np.swapaxes(s.got.cov, 1, 2))
  known = (np.abs(s.got.cov - SIGMA ** 2 * inv).max(axis=(1, 2)) / (SIGMA ** 2 * scale)).max()
  d_sse = np.abs(s.got.sse - s.sse).max()
  # the automatic sigma: the frame's own sse / (2 n - k), everything else unchanged
  auto = lh.run(s.rig, init=s.rig.rig_poses, init_end=s.rig.rig_poses_end)
  assert np.array_equal(auto.poses, s.got.poses) and np.array_equal(auto.sse, s.got.sse)
  K = s.H.shape[1]
  sigma2 = s.sse / (2 * s.got.n_obs - K)
  automatic = (np.abs(auto.cov - sigma2[:, None, None] * inv).max(axis=(1, 2)) / (sigma2 * scale)).max()
  # per-slot errors: the restatement's residual norms at the returned pose, 0 where nothing entered
  d_err, at = 0.0, lh.result_params(s.got)
  for f, fr in enumerate(s.frames):
    want = np.linalg.norm(fr.residuals(at[f]).reshape(-1, 2), axis=1)
    have = np.concatenate([s.got.error[c, f][s.rig.valid[c, f]] for c, _, _ in fr.cams])
    d_err = max(d_err, np.abs(have - want).max())
  assert (s.got.error[~s.rig.valid] == 0).all() and (s.got.error[s.rig.valid] > 0).all()
  note(f"noisy {name}: cov vs sigma^2 inv(J^T J) of the restatement {known:.2e} (known sigma) {automatic:.2e} (automatic) relative; "
       f"sse {d_sse:.2e} px^2, err {d_err:.2e} px")
  assert known <= 1e-6 and automatic <= 1e-6 and d_sse <= 1e-8 and d_err <= 1e-8


# ---- start selection -------------------------------------------------------------------------------------------------------------
def mirrored(rig, f, c, b):
  """the planar flip of view (c, b) of frame f as a rig pose: the board -> camera pose mirrored in the plane through the board's
  centre that faces the camera (the second minimum of planar PnP), taken back through camera_pose^-1 . T . board_pose^-1"""
  T = rig.camera_poses[c] @ rig.rig_poses[f] @ rig.board_poses[b]
  centre = np.asarray(rig.board_points[b]).mean(axis=0)
  o = T[:3, :3] @ centre + T[:3, 3]
  d = o / np.linalg.norm(o)
  S = np.eye(3) - 2.0 * np.outer(d, d)                       # reflection in the plane normal to the line of sight
  flipped = np.eye(4)
  R = S @ T[:3, :3]
  R[:, 2] = -R[:, 2]                                         # a proper rotation again: the board still shows its face
  flipped[:3, :3] = R
  flipped[:3, 3] = o - R @ centre
  assert np.linalg.det(R) > 0
  return np.linalg.inv(rig.camera_poses[c]) @ flipped @ np.linalg.inv(rig.board_poses[b])


def test_the_other_cameras_outvote_a_planar_flip():
  """a candidate list of the mirrored pose of the frame's largest view and the true pose (as a smaller view would give it): the
  scoring step picks the true one"""
  rig = lh.named_rig("8cam-2board-pin5")
  f = 0
  per_view = rig.valid[:, f].sum(axis=2)
  c, b = np.unravel_index(np.argmax(per_view), per_view.shape)
  flip = mirrored(rig, f, c, b)
  scores, picked = lh.score_candidates(rig, f, [flip, rig.rig_poses[f]])
  note(f"start selection: flipped largest view (camera {c}, board {b}, {per_view[c, b]} corners) scores {scores[0]:.3e} px^2, the true "
       f"pose {scores[1]:.3e} px^2 over {rig.valid[:, f].sum()} observations")
  assert picked == 1 and scores[1] < scores[0]
  assert scores[1] <= 1.5 * rig.valid[:, f].sum() * 2 * lh.NOISE_PX ** 2      # the true pose pays the noise alone


def test_a_distant_fronto_parallel_largest_view_still_ends_at_the_optimum():
  """two cameras; the largest view is a board far away and nearly fronto-parallel (the planar ambiguity at its weakest), the other
  camera sees a near board: the frame still ends at the restatement's optimum"""
  base = lh.make_rig(2, 2, "standard", False)
  rig = SimpleNamespace(**vars(base))
  f = 0
  # board 1 moves 6 m behind board 0, facing the rig; camera 0 keeps it whole, camera 1 keeps 15 corners of board 0
  cam0 = rig.camera_poses[0] @ rig.rig_poses[f]
  far = np.linalg.inv(cam0) @ lr.to_matrix(np.array([0.0, 0.01, 0.0, -0.18, -0.18, 6.0]))
  rig.board_poses = np.stack([rig.board_poses[0], far])
  pts = np.asarray(rig.board_points[1])
  valid = np.zeros_like(rig.valid[:, :1])
  points = np.zeros_like(rig.points[:, :1])
  rng = np.random.default_rng(3)
  for c, b, n in ((0, 1, len(pts)), (1, 0, 15)):
    T = rig.camera_poses[c] @ rig.rig_poses[f] @ rig.board_poses[b]
    X = np.asarray(rig.board_points[b])[:n] @ T[:3, :3].T + T[:3, 3]
    points[c, 0, b, :n] = lr.project(rig.cameras[c], X) + rng.normal(0.0, lh.NOISE_PX, (n, 2))
    valid[c, 0, b, :n] = True
  rig.points, rig.valid, rig.shape = points, valid, valid.shape
  rig.rig_poses = rig.rig_poses[f:f + 1]
  got = lh.run(rig, sigma=1.0)
  assert got.status[0] == localize.OK
  fr = lr.Frame(rig, 0)
  best = fr.solve(lr.start_vector(rig, 0))
  J = fr.jacobian(best.x)
  d = lh.whitened((J.T @ J)[None], lh.result_params(got) - best.x[None])[0]
  note(f"distant fronto-parallel largest view: whitened distance to the restatement's optimum {d:.2e} px")
  assert best.success and d <= 1e-8


# ---- statuses ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rolling", [(0, False), (1, False), (2, False), (5, True)])
def test_too_few_observations(n, rolling):
  rig = lh.keep_first(lh.make_rig(2, 1, "standard", rolling), n)
  for kw in (dict(), dict(init=rig.rig_poses, init_end=rig.rig_poses_end)):
    got = lh.run(rig, **kw)
    assert (got.status == localize.TOO_FEW).all() and (got.n_obs == n).all()
    assert np.array_equal(got.poses, np.broadcast_to(np.eye(4), got.poses.shape)) and np.isnan(got.cov).all()
    assert (got.sse == 0).all() and (got.error == 0).all()


def test_three_observations_are_enough_with_a_start():
  rig = lh.keep_first(lh.make_rig(2, 1, "standard", False, noise=0.0), 3, picks=(0, 4, 30))     # (three corners of three rows)
  got = lh.run(rig, init=rig.rig_poses, sigma=1.0)
  assert (got.status == localize.OK).all() and (got.n_obs == 3).all() and np.isfinite(got.cov).all()
  assert np.isnan(lh.run(rig, init=rig.rig_poses).cov).all()            # 2 n = k: no surplus for the automatic sigma
  assert (lh.run(rig).status == localize.DEGENERATE).all()              # no view of four corners: no start


def test_collinear_points_are_degenerate():
  base = lh.make_rig(2, 1, "standard", False)
  rig = SimpleNamespace(**vars(base))
  row = np.zeros(rig.shape[3], dtype=bool)
  row[:9] = True                                                         # the first row of the 9 x 9 corner grid: one line
  assert np.linalg.matrix_rank(np.asarray(rig.board_points[0])[:9] - np.asarray(rig.board_points[0])[0]) == 1
  rig.valid = base.valid & row
  assert (np.moveaxis(rig.valid, 1, 0).reshape(rig.shape[1], -1).sum(axis=1) >= 6).all()
  for kw in (dict(), dict(init=rig.rig_poses)):
    got = lh.run(rig, **kw)
    assert (got.status == localize.DEGENERATE).all() and np.isnan(got.cov).all() and (got.error == 0).all()
    assert np.array_equal(got.poses, np.broadcast_to(np.eye(4), got.poses.shape))


@pytest.mark.parametrize("name", ["2cam-2board-rational", "2cam-2board-mixed-rolling"])
def test_one_linearisation_is_one_levenberg_marquardt_step(name):
  rig = lh.named_rig(name)
  start = lh.run(rig, sigma=SIGMA)                                       # a start a few steps of 1e-3 away from the optimum
  rng = np.random.default_rng(11)
  init = start.poses @ lr.to_matrix(np.concatenate([rng.normal(0, 1e-3, 3), rng.normal(0, 1e-3, 3)]))
  init_end = None if not rig.rolling else start.poses_end @ lr.to_matrix(np.concatenate([rng.normal(0, 1e-3, 3), rng.normal(0, 1e-3, 3)]))
  got = lh.run(rig, init=init, init_end=init_end, max_iterations=1)
  assert (got.status == localize.NOT_CONVERGED).all() and (got.iters == 1).all()
  want = np.stack([lr.Frame(rig, f).lm_step(lr.start_vector(rig, f, init, init_end)) for f in range(rig.shape[1])])
  d = np.abs(lh.result_params(got) - want).max()
  print(f"{name}: one step against the restatement's hand-computed step {d:.2e}")
  assert d <= 1e-9
  # the cap is clamped to 100, 0 and below mean the default
  assert np.array_equal(lh.run(rig, max_iterations=10 ** 6).poses, lh.run(rig, max_iterations=0).poses)


def test_an_empty_frame_leaves_its_neighbours_alone():
  rig = lh.first_frames(lh.named_rig("2cam-2board-mixed-rolling"), 2)
  wide = SimpleNamespace(**vars(rig))
  shape = list(rig.valid.shape)
  shape[1] = 1
  wide.points = np.ascontiguousarray(np.concatenate([rig.points[:, :1], np.zeros(shape + [2]), rig.points[:, 1:]], axis=1))
  wide.valid = np.ascontiguousarray(np.concatenate([rig.valid[:, :1], np.zeros(shape, dtype=bool), rig.valid[:, 1:]], axis=1))
  wide.shape = wide.valid.shape
  a, b = lh.run(rig), lh.run(wide)
  assert b.status[1] == localize.TOO_FEW and b.n_obs[1] == 0
  for k in ("poses", "poses_end", "cov", "sse", "n_obs", "iters", "status"):
    assert np.asarray(a[k]).tobytes() == np.asarray(b[k])[[0, 2]].tobytes(), k
  assert a.error.tobytes() == np.ascontiguousarray(b.error[:, [0, 2]]).tobytes()


def test_refused_calls_and_empty_tables():
  rig = lh.make_rig(2, 1, "standard", False)
  fn = lh.lib().lh_rig_poses
  p, out, keep = lh.raw_problem(rig, n_cameras=localize.MAX_CAMERAS + 1)
  assert lh.raw_call(fn, p, out) == 1 and b"at most 64" in lh.lib().lh_last_error()
  p, out, keep = lh.raw_problem(rig)
  p.points = None
  assert lh.raw_call(fn, p, out) == 1 and b"null argument" in lh.lib().lh_last_error()
  p, out, keep = lh.raw_problem(rig)
  p.rolling = 1
  assert lh.raw_call(fn, p, out) == 1 and b"image_heights" in lh.lib().lh_last_error()
  # NULL outputs: poses and status alone are the full call's
  p, out, keep = lh.raw_problem(rig)
  assert lh.raw_call(fn, p, out) == 0
  full = lh.run(rig)
  assert out.poses.tobytes() == full.poses.tobytes() and out.status.tobytes() == full.status.tobytes()
  empty = lh.on_host(localize.localize_rig, rig.cameras, rig.camera_poses, rig.board_poses, rig.board_points, rig.points[:, :0], rig.valid[:, :0])
  assert empty.poses.shape == (0, 4, 4) and empty.cov.shape == (0, 6, 6) and empty.error.shape == (2, 0) + rig.shape[2:]


def test_a_masked_board_point_does_not_enter_the_plane_of_the_start():
  """board_valid with a hole before the last valid point: whatever stands in the masked slot, the start from the views (whose
  homography needs the board's plane) and so the whole result are the same bytes"""
  rig = lh.make_rig(2, 1, "standard", False)
  B, P = rig.shape[2:]
  pts = np.zeros((B, P, 3))
  pts[0, :len(rig.board_points[0])] = rig.board_points[0]
  board_valid = np.ones((B, P), dtype=bool)
  board_valid[0, 40] = False
  garbage = pts.copy()
  garbage[0, 40] = [3.0, -2.0, 5.0]
  a, b = [lh.on_host(localize.localize_rig, rig.cameras, rig.camera_poses, rig.board_poses, x, rig.points, rig.valid, board_valid=board_valid)
          for x in (pts, garbage)]
  assert (a.status == localize.OK).all() and (a.n_obs == (rig.valid & board_valid).sum(axis=(0, 2, 3))).all()
  for k in ("poses", "cov", "sse", "iters", "error", "status"):
    assert a[k].tobytes() == b[k].tobytes(), k


def test_sanitized_stand_alone_run(tmp_path):
  """the host build inside a small program of its own under AddressSanitizer + UBSan (CPU only): exact-size heap tables, pixels that
  are not finite, frames without observations, optional outputs left out -- no record is read and no error stored out of bounds"""
  r = host_build.sanitized_program("localize_host", "localize_sanitize_main.cpp", tmp_path)
  assert r.returncode == 0 and "localize sanitize run: ok" in r.stdout, r.stdout + r.stderr


# ---- Calibration.localize / with_localized_frames / report_holdout ---------------------------------------------------------------
def fixture_calibration(name):
  import pnp_host_lib
  from multical_amd import calibration
  return calibration.from_rig(pnp_host_lib.golden_rig(name), "truth")


def own_sse(calib):
  """[F] squared pixel error of the calibration's own poses over its valid points, by the restatement"""
  start, end = calib._rig_poses()
  rig = SimpleNamespace(cameras=list(calib.cameras), camera_poses=np.asarray(calib.camera_poses.poses),
                        board_poses=np.asarray(calib.board_poses.poses), board_points=[np.asarray(b.adjusted_points) for b in calib.boards],
                        points=np.asarray(calib.point_table.points), valid=np.asarray(calib.valid), rig_poses=start, rig_poses_end=end,
                        rolling=end is not None, shape=calib.valid.shape)
  return np.array([(lr.Frame(rig, f).residuals(lr.start_vector(rig, f)) ** 2).sum() for f in range(rig.shape[1])])


@pytest.mark.parametrize("name", ["tiny", "tiny_rolling", "tiny_fisheye"])
def test_localising_a_calibrations_own_table(name, caplog):
  """the fixture at its own parameters: with_localized_frames(calib.point_table) keeps the masks, every frame's cost can only go
  down (so the RMS does), the result pickles and report_holdout logs one line"""
  calib = fixture_calibration(name)
  before = own_sse(calib)
  with lh.host_backend(), caplog.at_level(logging.INFO, logger="calibration"):
    r = calib.localize(inliers_only=False)
    again = calib.localize(calib.point_table)
    held = calib.with_localized_frames(calib.point_table)
    calib.report_holdout(calib.point_table, "golden:")
  seen = np.moveaxis(calib.valid, 1, 0).reshape(calib.size.rig_poses, -1).sum(axis=1)
  assert (seen >= 12).sum() >= 5 and ((seen >= 12) | (seen == 0)).all()         # (a fixture frame may have no detection at all)
  want = np.where(seen > 0, localize.OK, localize.TOO_FEW)
  assert np.array_equal(r.status, want) and np.array_equal(again.status, want)
  assert np.array_equal(held.valid, calib.valid) and held.inlier_mask is None and held.size == calib.size
  assert type(held.motion).__name__ == ("RollingFrames" if name == "tiny_rolling" else "StaticFrames")
  assert np.array_equal(np.asarray(held.motion.valid), seen > 0)
  assert (r.sse <= before * (1.0 + 1e-12)).all() and (again.sse <= before * (1.0 + 1e-12)).all()
  n = calib.valid.sum()
  rms, own = np.sqrt(again.sse.sum() / n), np.sqrt(before.sum() / n)
  print(f"{name}: RMS {own:.6f} px at the fixture's poses, {rms:.6f} px localised (from its own views), {np.sqrt(r.sse.sum() / n):.6f} px (from its poses)")
  assert rms <= own and np.abs(np.sqrt((again.error[calib.valid] ** 2).mean()) - rms) <= 1e-9
  back = pickle.loads(pickle.dumps(held))
  assert np.array_equal(np.asarray(back.motion.frame_poses.poses), again.poses) and np.array_equal(back.valid, held.valid)
  lines = [m for m in caplog.messages if "held-out:" in m]
  assert len(lines) == 1 and f"{int((seen > 0).sum())} / {calib.size.rig_poses} frames localised" in lines[0] and "median translation std" in lines[0]


def test_zz_write_profile():
  """(not a check) MCBA_WRITE_PROFILES=1: the figures the tests above measured go to profiles/rig_pose_parity.txt"""
  if os.environ.get("MCBA_WRITE_PROFILES") and _figures:
    with open(os.path.join(ROOT, "profiles", "rig_pose_parity.txt"), "w") as fh:
      fh.write("Rig localisation: the host build of csrc/mcba_localize.h against tests/localize_reference.py (tests/test_localize_host.py)\n")
      fh.write("\n".join(_figures) + "\n")
