"""The stereo calibration mathematics (csrc/mcba_stereo.h) as g++ builds it, against an independent numpy / scipy restatement
(stereo_reference.py) -- no GPU.  The figures the tests print are recorded in profiles/stereo_parity.txt."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from multical_amd import camera, stereo, tables
from multical_amd.structs import Table

import pnp_host_lib
import stereo_host_lib as sh
import stereo_reference as sr


def note(line):
  print(line)


def case_of(name, **kw):
  return sh.make_case(name, frames=16, **kw)


@functools.lru_cache(maxsize=None)
def host_result(name, noise_free=False):
  return sh.run(case_of(name, noise_free=noise_free))


@functools.lru_cache(maxsize=None)
def reference_pair(name, i, j, noise_free=False):
  """(Pair, solution from the truth's relative pose, solution from a displaced start) of the restatement"""
  case = case_of(name, noise_free=noise_free)
  pair = sr.Pair(case, i, j)
  x0 = pair.start_vector(sh.truth_relative(case, i, j))
  a = pair.solve(x0)
  rng = np.random.default_rng(5)
  b = None if noise_free else pair.solve(x0 + np.concatenate([rng.normal(0, 2e-3, 6), rng.normal(0, 1e-3, len(x0) - 6)]))
  return pair, a, b


def index_of(res, i, j):
  return int(np.flatnonzero((res.pairs[:, 0] == i) & (res.pairs[:, 1] == j))[0])


# ---- noise-free: the truth comes back ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,i,j", [("tiny", 0, 1), ("tiny_mixed", 0, 1), ("tiny_mixed", 0, 2), ("tiny_mixed", 1, 3)])
def test_noise_free_tables_return_the_truth(name, i, j):
  """bound: max(1e-10, 100 x the restatement's own distance from the truth on the same data).  (tiny_mixed's camera 2 is `tilted`:
  the synthetic projection has no tilt, so on those pairs neither the header nor the restatement sits at the truth.)"""
  case, res = case_of(name, noise_free=True), host_result(name, True)
  k = index_of(res, i, j)
  truth = sh.truth_relative(case, i, j)
  pair, a, _ = reference_pair(name, i, j, True)
  ref_gap = sh.pose_gap(sr.to_matrix(a.x[:6]), truth)
  gap = sh.pose_gap(res.T[k], truth)
  note(f"noise-free {name} ({i}, {j}): header {gap:.3e} from the truth, restatement {ref_gap:.3e}, header - restatement "
       f"{sh.pose_gap(res.T[k], sr.to_matrix(a.x[:6])):.3e} (rad | m), status {res.status[k]}, {res.n_views[k]} views")
  assert res.status[k] == stereo.OK
  assert gap <= max(1e-10, 100.0 * ref_gap)
  # on the `tilted` pairs that bound is wide (neither sits at the truth); header and restatement share the data and their optimum:
  # the two agree as closely everywhere, which is what tests the tilt path of project_jac
  assert sh.pose_gap(res.T[k], sr.to_matrix(a.x[:6])) <= 1e-10


# ---- noisy: the optimum of the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,i,j", [("tiny", 0, 1), ("tiny_mixed", 0, 2), ("tiny_mixed", 1, 3), ("tiny_fishmix", 0, 1)])
def test_noisy_tables_end_at_the_optimum_of_the_restatement(name, i, j):
  """T, sse and cov within max(1e-9, 100 x scipy's own spread between two starts), the rule of profiles/pose_table_parity.txt
  (T: the six parameters, absolute; sse and cov: relative to their largest entry)"""
  case, res = case_of(name), host_result(name)
  k = index_of(res, i, j)
  pair, a, b = reference_pair(name, i, j)
  sa, sb = pair.summary(a.x), pair.summary(b.x)
  assert (pair.nv, pair.n_points) == (res.n_views[k], res.n_points[k]) == sh.common_counts(case, i, j)
  mine = sh.params(res.T[k])[0]
  figures = dict(
    T=(np.abs(mine - sa["params"]).max(), np.abs(sa["params"] - sb["params"]).max()),
    sse=(abs(res.sse[k] - sa["sse"]) / sa["sse"], abs(sa["sse"] - sb["sse"]) / sa["sse"]),
    cov=(np.abs(res.cov[k] - sa["cov"]).max() / np.abs(sa["cov"]).max(), np.abs(sa["cov"] - sb["cov"]).max() / np.abs(sa["cov"]).max()))
  note(f"noisy {name} ({i}, {j}): {pair.nv} views, {pair.n_points} points, rms {res.rms[k]:.4f} px, {res.iterations[k]} passes; "
       + "; ".join(f"{q}: header - restatement {d:.3e}, restatement's spread {s:.3e}" for q, (d, s) in figures.items()))
  assert res.status[k] == stereo.OK
  assert abs(res.rms[k] - sa["rms"]) <= 1e-9
  for q, (d, s) in figures.items():
    assert d <= max(1e-9, 100.0 * s), q
  # the per-view outputs: poses and costs of the views in table order
  slots = [(f, b) for f, b, _, _, _ in pair.views]
  vp = np.stack([res.view_poses[k, f, b] for f, b in slots])
  vs = np.stack([res.view_sse[k, f, b] for f, b in slots])
  assert sh.pose_gap(vp, sa["view_poses"]) <= max(1e-9, 100.0 * sh.pose_gap(sa["view_poses"], sb["view_poses"]))
  assert np.abs(vs - sa["view_sse"]).max() <= max(1e-9, 100.0 * np.abs(sa["view_sse"] - sb["view_sse"]).max()) * sa["sse"]
  assert abs(vs.sum() - res.sse[k]) <= 1e-12 * res.sse[k]


def test_both_summation_orders_agree():
  for name in ("tiny", "tiny_mixed", "tiny_bigboard"):
    case = sh.make_case(name, frames=8 if name == "tiny_bigboard" else 16)
    a, b = sh.run(case), sh.run(case, order=True)
    assert np.array_equal(a.status, b.status) and np.array_equal(a.n_points, b.n_points)
    assert np.abs(a.T - b.T).max() <= 1e-10 and np.abs(a.sse - b.sse).max() <= 1e-9 * a.sse.max()


# ---- a planted planar flip ----------------------------------------------------------------------------------------------------
def mirrored(T, centre):
  """the planar flip of a board -> camera pose: mirrored in the plane through the board's centre that faces the camera (the second
  minimum of planar PnP)"""
  o = T[:3, :3] @ centre + T[:3, 3]
  d = o / np.linalg.norm(o)
  R = (np.eye(3) - 2.0 * np.outer(d, d)) @ T[:3, :3]
  R[:, 2] = -R[:, 2]
  out = np.eye(4)
  out[:3, :3], out[:3, 3] = R, o - R @ centre
  assert np.linalg.det(R) > 0
  return out


def test_a_flipped_start_of_the_largest_view_still_ends_at_the_optimum():
  """the left camera's start pose of the pair's largest view is the mirrored one: its candidate for T_rel is outvoted by the other
  views', and the view itself is pulled back by the right camera's rows"""
  case, res = case_of("tiny"), host_result("tiny")
  n = np.where(case.view_valid[0] & case.view_valid[1], (case.valid[0] & case.valid[1]).sum(axis=-1), 0)
  f, b = np.unravel_index(np.argmax(n), n.shape)
  poses = case.view_poses.copy()
  poses[0, f, b] = mirrored(poses[0, f, b], np.asarray(case.board_points[b]).mean(axis=0))
  flipped = sh.run(sh.with_tables(case, view_poses=poses))
  note(f"flipped start of view ({f}, {b}), {n[f, b]} common corners: status {flipped.status[0]}, {flipped.iterations[0]} passes "
       f"(unflipped: {res.iterations[0]}), T differs by {sh.pose_gap(flipped.T[0], res.T[0]):.3e}, sse by "
       f"{abs(flipped.sse[0] - res.sse[0]) / res.sse[0]:.3e} relative")
  assert flipped.status[0] == stereo.OK
  assert sh.pose_gap(flipped.T[0], res.T[0]) <= 1e-9 and abs(flipped.sse[0] - res.sse[0]) <= 1e-9 * res.sse[0]
  assert sh.pose_gap(flipped.view_poses[0, f, b], res.view_poses[0, f, b]) <= 1e-9


# ---- statuses -------------------------------------------------------------------------------------------------------------------
def restricted(case, f, b, keep):
  """the case with the right camera's corners of slot (f, b) reduced to the ids `keep`"""
  valid = case.valid.copy()
  valid[1, f, b] = False
  valid[1, f, b, keep] = True
  return sh.with_tables(case, valid=valid, points=np.where(valid[..., None], case.points, 0.0))


def test_a_view_of_three_common_corners_is_dropped_and_one_of_four_enters():
  case, res = case_of("tiny"), host_result("tiny")
  n = np.where(case.view_valid[0] & case.view_valid[1], (case.valid[0] & case.valid[1]).sum(axis=-1), 0)
  f, b = np.argwhere(n >= 4)[0]
  ids = np.flatnonzero(case.valid[0, f, b] & case.valid[1, f, b])
  # four corners that are not on one line: two of the first grid row that is seen, two of the last
  rows = ids // 9
  four = np.concatenate([ids[rows == rows.min()][:2], ids[rows == rows.max()][:2]])
  assert len(four) == 4
  three, with_four = sh.run(restricted(case, f, b, four[:3])), sh.run(restricted(case, f, b, four))
  assert three.n_views[0] == res.n_views[0] - 1 and three.n_points[0] == res.n_points[0] - n[f, b]
  assert with_four.n_views[0] == res.n_views[0] and with_four.n_points[0] == res.n_points[0] - n[f, b] + 4
  assert three.status[0] == stereo.OK and with_four.status[0] == stereo.OK
  assert np.array_equal(three.view_poses[0, f, b], np.eye(4)) and not np.array_equal(with_four.view_poses[0, f, b], np.eye(4))
  # min_common is the caller's: at 3 the view enters
  assert sh.run(restricted(case, f, b, four[:3]), min_common=3).n_views[0] == res.n_views[0]


def test_a_pair_without_a_view_is_too_few():
  """tiny_fisheye's ring: no two cameras share a corner"""
  case = sh.make_case("tiny_fisheye")
  res = sh.run(case)
  assert len(res.pairs) == 3 and (res.status == stereo.TOO_FEW).all() and (res.n_views == 0).all() and (res.n_points == 0).all()
  assert np.array_equal(res.T, np.tile(np.eye(4), (3, 1, 1))) and np.isnan(res.cov).all() and (res.sse == 0).all()
  assert np.isnan(res.rms).all() and (res.iterations == 0).all()
  assert len(stereo.common_view_pairs(case.valid, case.view_valid)) == 0
  # beside a pair that has views, in one call
  tiny = case_of("tiny")
  none = sh.with_tables(tiny, view_valid=np.zeros_like(tiny.view_valid))
  assert (sh.run(none).status == stereo.TOO_FEW).all()


def test_collinear_common_corners_are_degenerate():
  """every view keeps one grid row of the board in the right camera: the rotation about that line is free"""
  case = case_of("tiny")
  valid = case.valid.copy()
  row = (np.arange(valid.shape[3]) // 9) == 4
  valid[1] &= row[None, None, :]
  line = sh.with_tables(case, valid=valid, points=np.where(valid[..., None], case.points, 0.0))
  res = sh.run(line)
  assert res.n_views[0] == 0 and sh.common_counts(line, 0, 1)[0] >= 1
  assert res.status[0] == stereo.DEGENERATE
  assert np.array_equal(res.T[0], np.eye(4)) and np.isnan(res.cov[0]).all() and res.sse[0] == 0
  # the list of pairs with a view follows the driver's rule where it is given the boards
  padded = stereo.pad_boards(line.board_points, line.valid.shape[3])[0]
  assert len(stereo.common_view_pairs(line.valid, line.view_valid, 4, padded)) == 0
  assert [tuple(p) for p in stereo.common_view_pairs(line.valid, line.view_valid, 4)] == [(0, 1)]
  assert [tuple(p) for p in stereo.common_view_pairs(case.valid, case.view_valid, 4, padded)] == [(0, 1)]
  # one such view among good ones is dropped, as one with too few corners is: the pair goes on without it
  full = host_result("tiny")
  f, b = np.argwhere(case.view_valid[0, :, :] & case.view_valid[1, :, :] & ((case.valid[0] & case.valid[1]).sum(axis=-1) >= 4))[0]
  one = case.valid.copy()
  one[1, f, b] &= row
  assert (one[0, f, b] & one[1, f, b]).sum() >= 4
  res = sh.run(sh.with_tables(case, valid=one, points=np.where(one[..., None], case.points, 0.0)))
  assert res.status[0] == stereo.OK and res.n_views[0] == full.n_views[0] - 1
  assert np.array_equal(res.view_poses[0, f, b], np.eye(4))


def test_refused_calls():
  case = case_of("tiny")
  for pairs in ([(0, 0)], [(0, 2)], [(-1, 1)]):
    with pytest.raises(RuntimeError, match="two different cameras"):
      sh.run(case, pairs=pairs)
  with pytest.raises(RuntimeError, match="min_common"):
    sh.run(case, min_common=2)
  assert len(sh.run(case, pairs=np.zeros((0, 2), dtype=np.int32)).status) == 0


def test_given_sigma_and_the_degree_of_freedom():
  case, res = case_of("tiny"), host_result("tiny")
  fixed = sh.run(case, sigma=0.5)
  dof = 4 * res.n_points[0] - 6 - 6 * res.n_views[0]
  assert np.allclose(fixed.cov[0] * (res.sse[0] / dof) / 0.25, res.cov[0], rtol=1e-12, atol=0)
  assert np.allclose(res.cov[0], res.cov[0].T, rtol=1e-9, atol=0) and (np.linalg.eigvalsh(res.cov[0]) > 0).all()


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def test_essential_and_fundamental_matrices():
  case, res = case_of("tiny", noise_free=True), host_result("tiny", True)
  T, (l, r) = res.T[0], res.pairs[0]
  rng = np.random.default_rng(0)
  Xl = rng.normal(0, 0.3, (20, 3)) + [0, 0, 2.0]
  Xr = Xl @ T[:3, :3].T + T[:3, 3]
  xl, xr = Xl / Xl[:, 2:], Xr / Xr[:, 2:]
  assert np.abs(np.einsum('ni,ij,nj->n', xr, res.essential[0], xl)).max() <= 1e-12
  Kl, Kr = case.cameras[l].intrinsic, case.cameras[r].intrinsic
  pl, pr = xl @ Kl.T, xr @ Kr.T
  assert np.abs(np.einsum('ni,ij,nj->n', pr, res.fundamental[0], pl)).max() <= 1e-12 * np.abs(res.fundamental[0]).max() * 1e7


def test_camera_stereo_calibrate_mirrors_stereo_pairs(monkeypatch):
  """camera.stereo_calibrate on tables.matching_points' output and stereo_pairs on the same pair end at the same optimum (the
  matched views are compacted: other chunks, other start poses, the same cost)"""
  case = case_of("tiny_mixed")
  case = sh.with_tables(case, cameras=[camera.Camera(c.image_size, c.intrinsic, c.dist, model=c.model) for c in case.cameras])
  i, j = 1, 3
  monkeypatch.setattr(camera, "_start_poses", pnp_host_lib.view_poses)
  table = Table.create(points=case.points, valid=case.valid)
  boards = [SimpleNamespace(points=p) for p in case.board_points]
  with sh.host_backend():
    matches = tables.matching_points(table, boards, i, j)
    left, right, pose, err = camera.stereo_calibrate((case.cameras[i], case.cameras[j]), matches)
    via_tables = tables.stereo_calibrate(table, boards, case.cameras, i, j)
    direct = stereo.stereo_pairs(case.cameras, boards, table, pairs=[(i, j)], pose_table=Table.create(poses=case.view_poses, valid=case.view_valid))
    with pytest.raises(NotImplementedError, match="Calibration.bundle_adjust"):
      camera.stereo_calibrate((case.cameras[i], case.cameras[j]), matches, fix_intrinsic=False)
    with pytest.raises(NotImplementedError, match="Calibration.bundle_adjust"):
      camera.stereo_calibrate_fisheye((case.cameras[i], case.cameras[j]), matches, fix_intrinsic=False)
  assert len(matches.points1) == case.valid.shape[1] * case.valid.shape[2]
  assert all(len(a) == len(b) == len(c) == len(d) for a, b, c, d in zip(matches.points1, matches.points2, matches.object_points, matches.ids))
  assert sum(len(x) for x in matches.ids if len(x) >= 4) >= direct.n_points[0]
  note(f"mirror tiny_mixed ({i}, {j}): pose differs by {sh.pose_gap(pose, direct.T[0]):.3e}, err by {abs(err - direct.rms[0]):.3e} px")
  assert sh.pose_gap(pose, direct.T[0]) <= 1e-9 and abs(err - direct.rms[0]) <= 1e-9
  assert np.array_equal(via_tables[2], pose) and via_tables[3] == err
  assert np.array_equal(left.intrinsic, case.cameras[i].intrinsic) and np.array_equal(right.dist, case.cameras[j].dist)


def test_sanitized_stand_alone_run(tmp_path):
  """the host build inside a small program of its own under AddressSanitizer + UBSan (CPU only; nothing is loaded into Python):
  exact-size heap tables, pixels that are not finite, a collinear slot, an invalid start pose, a camera that sees nothing in a frame,
  both summation orders, optional outputs left out -- no corner is read and no view block stored out of bounds"""
  import host_build
  r = host_build.sanitized_program("stereo_host", "stereo_sanitize_main.cpp", tmp_path)
  assert r.returncode == 0 and "stereo sanitize run: ok" in r.stdout, r.stdout + r.stderr


# ---- the scaled difference: cameras far apart ---------------------------------------------------------------------------------
def test_scaled_difference_against_a_sampled_covariance_at_120_degrees():
  """400 noisy copies of a pair whose cameras are 120 degrees apart (sigma = 0.2 px, given): the estimates' scatter about the truth
  in the covariance's own parameters -- global rotation vector, translation -- has the reported covariance, and
  stereo.scaled_difference squared averages 3, the mean of a chi-square of 3 degrees of freedom, for rotation and for translation.
  Bounds: the mean of N chi-square(3) draws has standard deviation sqrt(6 / N) = 0.12: 4 of them; an eigenvalue of C^-1 S of a
  sampled 3 x 3 covariance scatters by about sqrt(2 / N) + sqrt(3 / N) = 0.16 about 1: [0.6, 1.5].  The rotation vector of
  R R_truth^T, a left-tangent increment L(w) d_w, is printed beside it: at this angle it does not follow the covariance."""
  N = 400
  case, T_rel = sh.wide_case(120, N)
  res = sh.run(case, pairs=[(2 * k, 2 * k + 1) for k in range(N)], sigma=0.2)
  assert (res.status == stereo.OK).all()
  truth = np.tile(T_rel, (N, 1, 1))
  diff = stereo.scaled_difference(res.T, truth, res.cov)
  tol = 4.0 * np.sqrt(6.0 / N)
  naive = stereo.rotation_vectors(res.T[:, :3, :3] @ T_rel[:3, :3].T)
  C = res.cov.mean(axis=0)
  naive_mean = float(np.mean(np.einsum('ni,ij,nj->n', naive, np.linalg.inv(C[:3, :3]), naive)))
  eig = {}
  for part, d, sl in (("rotation", diff.d_rot, slice(0, 3)), ("translation", diff.d_t, slice(3, 6))):
    S = d.T @ d / N
    eig[part] = np.sort(np.linalg.eigvals(np.linalg.solve(C[sl, sl], S)).real)
  note(f"120 degrees apart, {N} draws: mean scaled^2 rotation {np.mean(diff.rotation ** 2):.3f}, translation "
       f"{np.mean(diff.translation ** 2):.3f} (3 expected, bound +- {tol:.2f}); the left-tangent increment against the same covariance "
       f"{naive_mean:.3f}; eigenvalues of C^-1 S rotation {np.round(eig['rotation'], 3)}, translation {np.round(eig['translation'], 3)}; "
       f"sd rotation {np.sqrt(np.diag(C)[:3])}")
  assert np.abs(res.cov - C).max() <= 0.2 * np.abs(C).max()        # (the linearisation point moves the covariance little)
  assert abs(np.mean(diff.rotation ** 2) - 3.0) <= tol and abs(np.mean(diff.translation ** 2) - 3.0) <= tol
  for part in eig:
    assert 0.6 <= eig[part][0] and eig[part][-1] <= 1.5, part
  # the 2 pi branch: the same pose given with the other representation of its rotation differs by nothing
  assert np.abs(stereo.scaled_difference(res.T[:1], res.T[:1], res.cov[:1]).d_rot).max() == 0.0


def test_scaled_difference_is_taken_in_the_parameters_of_the_covariance():
  """deterministic: poses whose global rotation vectors differ by a planted d (1e-6 rad, so terms of second order are 1e-6 of it)
  at rotations of 90, 150 and 179 degrees against an anisotropic covariance: the scaled difference is sqrt(d^T C^-1 d) to 1e-5
  relative, where the rotation vector of R R_other^T would give another figure"""
  from scipy.spatial.transform import Rotation
  C = np.zeros((6, 6))
  C[:3, :3] = np.array([[4.0, 1.0, 0.5], [1.0, 100.0, 2.0], [0.5, 2.0, 2500.0]]) * 1e-14
  C[3:, 3:] = np.diag([1.0, 4.0, 9.0]) * 1e-12
  d = 1e-6 * np.array([0.6, -0.5, 0.62])
  want = float(np.sqrt(d @ np.linalg.solve(C[:3, :3], d)))
  for deg in (90.0, 150.0, 179.0):
    w0 = np.deg2rad(deg) * np.array([0.48, 0.6, 0.64])
    a, b = np.eye(4), np.eye(4)
    a[:3, :3], b[:3, :3] = Rotation.from_rotvec(w0 + d).as_matrix(), Rotation.from_rotvec(w0).as_matrix()
    a[:3, 3], b[:3, 3] = [0.1 + 2e-6, 0.2, 0.3], [0.1, 0.2, 0.3]
    r = stereo.scaled_difference(a[None], b[None], C[None])
    naive = Rotation.from_matrix(a[:3, :3] @ b[:3, :3].T).as_rotvec()
    naive = float(np.sqrt(naive @ np.linalg.solve(C[:3, :3], naive)))
    note(f"{deg} degrees: scaled rotation {r.rotation[0]:.6f}, planted {want:.6f}, left-tangent increment {naive:.6f}")
    assert abs(r.rotation[0] - want) <= 1e-5 * want and abs(r.translation[0] - 2.0) <= 1e-9
    assert deg > 150.0 or abs(naive - want) > 0.05 * want       # (this planted d happens to suit the increment at 179 degrees)


def test_a_launched_pair_without_a_finite_cost_is_degenerate():
  """start poses that are not finite: the pair has views and is solved (one linearisation), its cost is not finite -- the loop's own
  DEGENERATE exit, with the outputs of a pair without a result"""
  case = case_of("tiny")
  poses = case.view_poses.copy()
  poses[0] = np.nan
  res = sh.run(sh.with_tables(case, view_poses=poses))
  assert res.status[0] == stereo.DEGENERATE and res.n_views[0] == host_result("tiny").n_views[0] and res.iterations[0] == 1
  assert np.array_equal(res.T[0], np.eye(4)) and np.isnan(res.cov[0]).all() and res.sse[0] == 0 and np.isnan(res.rms[0])
  assert (res.view_poses[0] == np.eye(4)).all() and (res.view_sse[0] == 0).all()


def test_corners_that_are_nearly_on_a_line_are_solved():
  """every view keeps one grid row of the board in the right camera, its corners moved 1e-5 of the row's length off the line to
  alternating sides: above the driver's 1e-6, so the views enter.  The rotation of every view about its line is all but free and the
  loop crawls, but the scaled pivots stay above the floor of 1e-12 -- that floor only guards what the driver's drop would let
  through -- and the pair has a result with a finite covariance"""
  case, full = case_of("tiny"), host_result("tiny")
  valid = case.valid.copy()
  row = (np.arange(valid.shape[3]) // 9) == 4
  valid[1] &= row[None, None, :]
  board = case.board_points[0].copy()
  ids = np.flatnonzero(row)
  length = np.linalg.norm(board[ids[-1]] - board[ids[0]])
  board[ids, 1] += 1e-5 * length * np.where(np.arange(len(ids)) % 2 == 0, 1.0, -1.0)
  res = sh.run(sh.with_tables(case, valid=valid, points=np.where(valid[..., None], case.points, 0.0), board_points=[board]))
  sd, sd_full = np.sqrt(np.diag(res.cov[0])[:3]).max(), np.sqrt(np.diag(full.cov[0])[:3]).max()
  note(f"nearly collinear: status {res.status[0]}, {res.n_views[0]} views, {res.iterations[0]} passes, largest rotation sd {sd:.3e} rad "
       f"(full views: {sd_full:.3e})")
  assert res.n_views[0] >= 1 and res.status[0] in (stereo.OK, stereo.NOT_CONVERGED)
  assert np.isfinite(res.cov[0]).all() and np.isfinite(res.T[0]).all() and res.sse[0] > 0


def test_pairwise_extrinsics_on_the_host_build():
  """Calibration.pairwise_extrinsics through the host build: the fields, the scaled differences as stereo.scaled_difference gives
  them, and the ranking"""
  from multical_amd import calibration
  case = case_of("tiny_mixed")
  calib = calibration.from_rig(case.rig, which="truth")
  with sh.host_backend():
    r = calib.pairwise_extrinsics()
  assert len(r.pairs) == 6 and r.enough.all() and ((r.status == stereo.OK) | (r.status == stereo.NOT_CONVERGED)).all()
  diff = stereo.scaled_difference(r.T, r.T_rig, r.cov)
  assert np.array_equal(r.rotation_scaled, diff.rotation) and np.array_equal(r.translation_scaled, diff.translation)
  assert np.array_equal(r.scaled, np.fmax(diff.rotation, diff.translation)) and (np.diff(r.scaled[r.ranking]) <= 0).all()
  assert np.allclose(r.T_rig, [sh.truth_relative(case, i, j) for i, j in r.pairs], atol=1e-14)
  # (the pairs' standard deviations are 0.4 .. 0.9 mrad and 0.5 .. 1.8 mm on these 16 frames: five of the largest)
  assert (r.rotation_mrad < 10.0).all() and (r.translation_mm < 10.0).all()
