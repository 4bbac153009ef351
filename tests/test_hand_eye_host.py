"""Host tests (no GPU) of the robot-world hand-eye start: the g++ build of multical_amd/csrc/mcba_handeye.h (tests/handeye_host)
against exact data, against the independent numpy restatement (tests/handeye_reference.py: SVD of K, lstsq) and under the status
rules; and the Python layer (multical_amd/hand_eye.py) driven through the host build instead of the device call.

Tolerances: exact data, well-separated singular values: 1e-12 (observed 3e-15).  cfg5_40's exact truth chain (3 .. 9 pairs a
problem, sigma2 / sigma1 of K up to 0.99997 because the ring rig turns almost about one axis): 1e-9 rad / 1e-9 m (observed 2.5e-12
/ 6.4e-12).  Host build against the restatement: max(1e-9, 100 x |restatement(pairs) - restatement(pairs reversed)|) per problem
-- the restatement's own sensitivity to the order of a sum is the scale of what two correct implementations may differ by.
Measured maxima: profiles/hand_eye_parity.txt."""
import numpy as np
import pytest
from scipy import stats
from scipy.spatial.transform import Rotation

import handeye_host_lib as hh
import handeye_reference as ref
from multical_amd import hand_eye, tables
from multical_amd.structs import Table

OK, TOO_FEW, DEGENERATE = tables.HANDEYE_OK, tables.HANDEYE_TOO_FEW, tables.HANDEYE_DEGENERATE


def _one(A, B, **kw):
  ok = np.ones((1, len(A)), dtype=bool)
  X, Z, n, st, err = hh.hand_eye_batch(A[None], ok, B[None], ok, [0], [0], **kw)
  return X[0], Z[0], int(n[0]), int(st[0]), err[0]


def _diff(a, b):
  return np.abs(np.asarray(a) - np.asarray(b)).reshape(len(a), -1).max(axis=1)


# ---- exact recovery ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 12, 200])
def test_exact_pairs_are_recovered(n):
  A, B, X, Z = hh.exact_pairs(100 + n, n)
  Xh, Zh, npairs, st, err = _one(A, B)
  print(f"n = {n}: |X - truth| {np.abs(Xh - X).max():.1e}, |Z - truth| {np.abs(Zh - Z).max():.1e}, err {err.max():.1e}")
  assert st == OK and npairs == n
  assert np.abs(Xh - X).max() <= 1e-12 and np.abs(Zh - Z).max() <= 1e-12
  assert err.max() <= 1e-12


def test_exact_chain_of_cfg5_40_gives_the_relative_camera_poses():
  poses, valid, rig, (C_, F, B) = hh.camera_board_chain("cfg5_40")
  ia, ib, combos = hh.camera_pair_problems(valid, C_, B)
  X, Z, n, st, err = hh.hand_eye_batch(poses, valid, poses, valid, ia, ib, invert=True)
  assert len(combos) == 216 and n.min() == 3 and n.max() == 9
  assert np.all(st == OK)
  cp = rig.truth.camera_poses
  truth = np.array([cp[m] @ np.linalg.inv(cp[s]) for m, s, _, _ in combos])
  ang, dist = hh.pose_distance(X, truth)
  print(f"cfg5_40 exact chain, {len(combos)} problems: {ang.max():.1e} rad, {dist.max():.1e} m, err {err.max():.1e}")
  assert ang.max() <= 1e-9 and dist.max() <= 1e-9


# ---- host build against the restatement ----------------------------------------------------------------------------------
def _cases():
  out = []
  for n in (3, 4, 12, 200):
    A, B, _, _ = hh.exact_pairs(100 + n, n)
    ok = np.ones((1, n), dtype=bool)
    out.append((f"exact{n}", (A[None], ok, B[None], ok, np.array([0]), np.array([0])), False))
  poses, valid, _, (C_, F, B_) = hh.camera_board_chain("cfg5_40", noise_seed=7)
  ia, ib, _ = hh.camera_pair_problems(valid, C_, B_)
  out.append(("cfg5_40_noisy", (poses, valid, poses, valid, ia, ib), True))
  return out


def test_host_build_agrees_with_the_restatement():
  compared, excluded = 0, 0
  for tag, args, invert in _cases():
    h = hh.hand_eye_batch(*args, invert=invert)
    r = ref.batch(*args, invert=invert)
    rr = ref.batch(*args, invert=invert, reversed_order=True)
    assert np.array_equal(h[2], r[2]) and np.array_equal(h[3], r[3]), tag          # n_pairs, status
    both_failed = (h[3] != OK) & (r[3] != OK)
    excluded += int(both_failed.sum())
    keep = ~both_failed
    compared += int(keep.sum())
    spread = np.maximum(_diff(r[0], rr[0]), _diff(r[1], rr[1]))
    tol = np.maximum(1e-9, 100.0 * spread)
    dX, dZ = _diff(h[0], r[0]), _diff(h[1], r[1])
    dE = np.abs(h[4] - r[4]).max(axis=1)
    print(f"{tag}: {int(keep.sum())} problems, |dX| {dX[keep].max():.1e}, |dZ| {dZ[keep].max():.1e}, |d err| {dE[keep].max():.1e}, "
          f"restatement order spread {spread[keep].max():.1e}")
    assert np.all(dX[keep] <= tol[keep]) and np.all(dZ[keep] <= tol[keep]) and np.all(dE[keep] <= tol[keep]), tag
  assert compared == 4 + 216 and excluded == 0


# ---- status rules ----------------------------------------------------------------------------------------------------------
def test_two_pairs_are_too_few():
  A, B, _, _ = hh.exact_pairs(5, 2)
  X, Z, n, st, err = _one(A, B)
  assert st == TOO_FEW and n == 2
  assert np.array_equal(X, np.eye(4)) and np.array_equal(Z, np.eye(4)) and not err.any()


def test_pure_translations_are_degenerate():
  rng = np.random.default_rng(11)
  X, Z = hh.random_poses(rng, 2)
  B = hh.random_poses(rng, 10)
  B[:, :3, :3] = B[0, :3, :3]                      # identical rotations, differing translations
  A = Z @ B @ np.linalg.inv(X)
  Xh, Zh, n, st, err = _one(A, B)
  assert st == DEGENERATE and n == 10
  assert np.array_equal(Xh, np.eye(4)) and np.array_equal(Zh, np.eye(4)) and not err.any()
  assert ref.solve(A, B)[2] == ref.DEGENERATE


def test_rotations_about_one_axis_are_degenerate():
  rng = np.random.default_rng(12)
  X, Z = hh.random_poses(rng, 2)
  axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
  A = hh.random_poses(rng, 10)
  A[:, :3, :3] = Rotation.from_rotvec(axis[None] * rng.uniform(-2.0, 2.0, (10, 1))).as_matrix()
  B = np.linalg.inv(Z) @ A @ X
  Xh, Zh, n, st, _ = _one(A, B)
  assert st == DEGENERATE and n == 10
  assert np.array_equal(Xh, np.eye(4)) and np.array_equal(Zh, np.eye(4))
  assert ref.solve(A, B)[2] == ref.DEGENERATE


def test_non_finite_input_is_degenerate():
  A, B, _, _ = hh.exact_pairs(6, 8)
  for bad in (np.nan, np.inf):
    A2 = A.copy()
    A2[3, 1, 2] = bad
    X, Z, n, st, err = _one(A2, B)
    assert st == DEGENERATE and np.array_equal(X, np.eye(4)) and np.array_equal(Z, np.eye(4)) and not err.any()


def test_masked_frames_do_not_enter():
  ta, va, tb, vb, Xs, Zs = hh.interleaved_problem(21, 12, n_rows=3)
  X, Z, n, st, err = hh.hand_eye_batch(ta, va, tb, vb, [0, 1, 2], [0, 1, 2])
  assert np.all(st == OK) and np.all(n == 12)
  assert np.abs(X - Xs).max() <= 1e-12 and np.abs(Z - Zs).max() <= 1e-12
  used = va & vb
  assert not err[~used].any() and err[used].max() <= 1e-12
  # mismatched rows: row 0 of A with row 1 of B share fewer usable frames and are no exact problem; the count is the intersection
  n01 = hh.hand_eye_batch(ta, va, tb, vb, [0], [1])[2][0]
  assert n01 == int((va[0] & vb[1]).sum())


def test_invert_inputs_equals_inverting_on_the_host():
  ta, va, tb, vb, _, _ = hh.interleaved_problem(22, 9, n_rows=2)
  a = hh.hand_eye_batch(ta, va, tb, vb, [0, 1], [0, 1], invert=True)
  b = hh.hand_eye_batch(ref.inverse(ta), va, ref.inverse(tb), vb, [0, 1], [0, 1])
  assert np.all(a[3] == OK) and np.array_equal(a[3], b[3]) and np.array_equal(a[2], b[2])
  for u, v in zip((a[0], a[1], a[4]), (b[0], b[1], b[4])):
    assert np.abs(u - v).max() <= 1e-12


def test_index_out_of_range_is_refused():
  A, B, _, _ = hh.exact_pairs(5, 4)
  ok = np.ones((1, 4), dtype=bool)
  with pytest.raises(RuntimeError, match="outside"):
    hh.hand_eye_batch(A[None], ok, B[None], ok, [1], [0])


# ---- the Python layer through the host build ----------------------------------------------------------------------------------
def _pose_table(poses, valid, C_, F, B):
  return Table.create(poses=np.moveaxis(poses.reshape(C_, B, F, 4, 4), 1, 2), valid=np.moveaxis(valid.reshape(C_, B, F), 1, 2))


def _expected_picks(poses, valid, C_, B):
  """the reference's loop (hand_eye/hand_eye.py:38-57) over the restatement with scipy's KDE (hand_eye/helper.py:5-18) and the
  documented fallback: {(master, slave): (candidate index, candidate count)}"""
  ia, ib, combos = hh.camera_pair_problems(valid, C_, B)
  X, _, n, st, _ = ref.batch(poses, valid, poses, valid, ia, ib, invert=True)
  out = {}
  for m in range(C_):
    for s in range(C_):
      if s == m:
        continue
      k = [i for i, c in enumerate(combos) if c[:2] == (m, s) and st[i] == ref.OK]
      if len(k) >= 5:
        xyz = X[k][:, :3, 3].T
        density = stats.gaussian_kde(xyz)(xyz)
        assert np.sort(density)[-2] < density.max() * (1.0 - 1e-6), (m, s, density)     # a clear winner: nothing to break
        pick = int(np.argmax(density))
      else:
        # 4 candidates or fewer: no vote exists.  scipy refuses fewer than 4; exactly 4 points in 3-D whiten to a regular simplex,
        # the density is the same at all four and a bare argmax would assert rounding noise (test_kde_of_four_candidates_is_flat).
        # The documented choice: the problem with the most pairs, the first on ties.
        pick = int(np.argmax(n[k]))
      out[(m, s)] = (pick, len(k))
  return out


def _check_hand_eye(poses, valid, C_, F, B):
  names = [f"cam{i}" for i in range(C_)]
  he = hand_eye.HandEye(_pose_table(poses, valid, C_, F, B), names, solver=hh.hand_eye_batch)
  cam_init = he.initialise_camera_poses()
  expected = _expected_picks(poses, valid, C_, B)
  for (m, s), (pick, count) in expected.items():
    assert he.picks[(names[m], names[s])] == pick, (m, s, count)
    assert len(he.camera_groups[names[m]][names[s]]) == count
  assert he.reference_camera in names and he.camera_poses['Reference_camera'] == he.reference_camera
  assert np.abs(cam_init[names[0]] - np.eye(4)).max() <= 1e-12
  return he, cam_init, expected


def test_hand_eye_class_picks_the_candidates_of_the_kde_vote():
  poses, valid, rig, (C_, F, B) = hh.camera_board_chain("cfg5_40", noise_seed=7)
  he, cam_init, expected = _check_hand_eye(poses, valid, C_, F, B)
  assert len(he.handeye_df) == 216
  assert he.viewed_boards == {f"cam{c}": [b for b in range(B) if valid.reshape(C_, B, F)[c, b].sum() > 6] for c in range(C_)}
  # the start is the truth's camera poses relative to the first camera, to the noise of the chain
  cp = rig.truth.camera_poses
  truth = cp @ np.linalg.inv(cp[0])
  ang, dist = hh.pose_distance(np.array([cam_init[f"cam{c}"] for c in range(C_)]), truth)
  print(f"cfg5_40 noisy chain: camera-pose start within {ang.max():.1e} rad, {dist.max():.1e} m of the truth")
  assert ang.max() < 5e-3 and dist.max() < 5e-3        # (pose noise 2e-4 rad / 1e-4 m through problems of 3 .. 9 pairs)
  # master_slave_pair is the single problem
  k = 17
  d = he.handeye_df[k]
  X, ids = he.master_slave_pair(int(d["master_cam"][3:]), int(d["slave_cam"][3:]), d["boardM"], d["boardS"])
  assert np.array_equal(ids, d["image_ids"]) and np.array_equal(X, d["slaveCam_wrt_masterCam"])


def test_kde_of_four_candidates_is_flat():
  """the fact behind the tie rule of multical_amd/hand_eye.py: any 4 points in general position get the same kernel density"""
  rng = np.random.default_rng(3)
  for _ in range(5):
    xyz = rng.normal(size=(3, 4)) * rng.uniform(0.1, 10.0, (3, 1))
    density = stats.gaussian_kde(xyz)(xyz)
    # equal up to the rounding of the whitening: eps x the covariance's condition (here <= 1e4, a few more for the sample) -- far
    # inside the 1e-9 within which hand_eye.vote counts densities as tied
    assert np.ptp(density) <= 1e-10 * density.max(), np.ptp(density) / density.max()
  # ... so the vote goes by the pair counts there, and by the density alone with a clear winner
  assert hand_eye.vote(xyz.T, [3, 9, 9, 4])[0] == 1
  five = np.array([[0, 0, 0], [0.01, 0, 0], [0, 0.01, 0], [0, 0, 0.01], [5.0, 4.0, 3.0]])
  assert hand_eye.vote(five, [3, 3, 3, 3, 99])[0] != 4


def test_fewer_than_four_candidates_fall_back_to_the_problem_with_most_pairs():
  poses, valid, rig, (C_, F, B) = hh.camera_board_chain("cfg5_40", noise_seed=7)
  ia, ib, combos = hh.camera_pair_problems(valid, C_, B)
  counts = {}
  for c in combos:
    counts[c[:2]] = counts.get(c[:2], 0) + 1
  pair = next(p for p in sorted(counts) if counts[p] == 4)
  m, s, bm, bs = next(c for c in combos if c[:2] == pair)
  valid = valid.copy()
  common = np.flatnonzero(valid[m * B + bm] & valid[s * B + bs])
  valid[m * B + bm, common[2:]] = False               # 2 common frames are left: the combination drops out
  he, _, expected = _check_hand_eye(poses, valid, C_, F, B)
  assert expected[pair][1] == 3
  assert he.camera_groups[f"cam{pair[0]}"][f"cam{pair[1]}"] is not None


def test_a_camera_pair_without_candidates_is_named():
  poses, valid, rig, (C_, F, B) = hh.camera_board_chain("cfg5_40", noise_seed=7)
  valid = valid.copy()
  valid[(C_ - 1) * B:] = False                         # the last camera sees nothing
  he = hand_eye.HandEye(_pose_table(poses, valid, C_, F, B), [f"cam{i}" for i in range(C_)], solver=hh.hand_eye_batch)
  with pytest.raises(ValueError, match=r"\(cam0, cam5\)"):
    he.initialise_camera_poses()


def test_hand_eye_robot_world_and_its_transposed_form():
  A, B, X, Z = hh.exact_pairs(31, 15)
  bw, gc, err = hand_eye.hand_eye_robot_world(A, B, solver=hh.hand_eye_batch)
  assert np.abs(bw - X).max() <= 1e-12 and np.abs(gc - Z).max() <= 1e-12 and err.shape == (15,) and err.max() <= 1e-12
  bw_t, gc_t, _ = hand_eye.hand_eye_robot_world_t(np.linalg.inv(A), np.linalg.inv(B), solver=hh.hand_eye_batch)
  assert np.abs(bw_t - np.linalg.inv(X)).max() <= 1e-11 and np.abs(gc_t - np.linalg.inv(Z)).max() <= 1e-11
  with pytest.raises(ValueError, match="fewer than 3"):
    hand_eye.hand_eye_robot_world(A[:2], B[:2], solver=hh.hand_eye_batch)


def test_library_reports_a_refusal_thrown_in_the_hand_eye_unit():
  """No device needed: the argument check of mcba_hand_eye throws in its own translation unit (csrc/mcba_handeye.hip) and
  mcba_last_error(), defined in another one, carries the message -- the host runtime's objects exist once per library."""
  from multical_amd import _lib
  ta, va, tb, vb, _, _ = hh.interleaved_problem(5, 6, n_rows=2)
  with pytest.raises(_lib.McbaError, match=r"mcba_hand_eye: problem 1: rows \(2, 1\) outside tables of 2 and 2 rows"):
    tables.hand_eye_batch(ta, va, tb, vb, [0, 2], [0, 1])
  assert "rows (2, 1)" in _lib.load().mcba_last_error().decode()
