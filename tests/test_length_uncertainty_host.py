"""The pair mathematics of csrc/mcba_recon.h (covariance of the difference of two triangulated points, of their length, and their cross
covariance) in its g++ build, and the marshalling of multical_amd.reconstruction / Calibration on top of it: against long double, its
own identities, the frame invariance of the length, Monte Carlo through the independent restatement, and the first-order law.  No GPU."""
import numpy as np
import pytest

from multical_amd import reconstruction, synthetic, uncertainty
from multical_amd.structs import struct

import host_build
import length_uncertainty_host_lib as ll
import reconstruction_uncertainty_host_lib as rl
import reconstruction_uncertainty_reference as rr
import uncertainty_host_lib as ul
from util import mirror

EPS = np.finfo(np.float64).eps
mats = reconstruction.covariance_matrices
cross = reconstruction.cross_matrices
LD = np.longdouble


def unit(v):
  return np.asarray(v, dtype=np.float64) / np.linalg.norm(v)


def held_sigma(m, seed=3):
  """a covariance of every stored parameter of the group with the pose of slot 0 held"""
  p = sum(M.shape[1] for M in rl.stored_maps(m))
  sigma = ul.random_spd(p, seed)
  lo = 5 + m.n_dist[0]
  sigma[lo:lo + 6, :] = 0.0
  sigma[:, lo:lo + 6] = 0.0
  return sigma


def exact(m, ref, sigma, F, Xa, Xb):
  """long double: (cov_diff, cross, C_a, C_b, J_a, J_b) from the header's own rows (pinned by the Richardson test of the point entry)"""
  Ja, sa = rl.stored_rows(m, ref, Xa)
  Jb, sb = rl.stored_rows(m, ref, Xb)
  assert sa == reconstruction.OK and sb == reconstruction.OK
  D = (Ja.astype(LD) - Jb.astype(LD)) @ F.astype(LD)
  S = sigma.astype(LD)
  return D @ D.T, Ja.astype(LD) @ S @ Jb.astype(LD).T, Ja.astype(LD) @ S @ Ja.astype(LD).T, Jb.astype(LD) @ S @ Jb.astype(LD).T, Ja, Jb


def diff_bound(Ja, Jb, F):
  """|dC| <= 2 e D + e^2: every z carries eps |J| |F|, and the sum of d d^T is D^2 = |(J_a - J_b) F|_F^2"""
  e = 1000.0 * EPS * (np.linalg.norm(Ja) + np.linalg.norm(Jb)) * np.linalg.norm(F, 2)
  D = np.linalg.norm((Ja.astype(LD) - Jb.astype(LD)).astype(np.float64) @ F)
  return 2.0 * e * D + e * e


# ---- 1. against long double ------------------------------------------------------------------------------------------------------
A0 = np.array([-0.2, 0.1, 1.5])
SEPARATIONS = [("1 m", 1.0, unit([0.3, -0.25, 0.95])), ("1 cm", 0.01, unit([1.0, 0.2, -0.1])), ("1 mm", 0.001, unit([0.1, 1.0, 0.3]))]


@pytest.mark.parametrize("ref", [None, 1], ids=["rig", "camera"])
def test_against_long_double(ref):
  """cov_diff_cal against ((J_a - J_b) F)((J_a - J_b) F)^T and cross_cal against J_a Sigma J_b^T in np.longdouble; beside them how far
  the naive C_a + C_b - C_ab - C_ab^T, formed from the entry's own outputs, is from the same value (printed, not asserted)"""
  m, _ = rl.group_rig(3, 3)
  p = sum(M.shape[1] for M in rl.stored_maps(m))
  A = np.random.default_rng(5).normal(size=(p, 5)) * 1e-3
  for label, sigma in (("held pose", held_sigma(m)), ("rank 5", A @ A.T)):
    F = uncertainty.factor(sigma)
    pts = np.array([A0] + [A0 + s * u for _, s, u in SEPARATIONS])
    assert (pts[:, 2] >= 1.5 - 1e-3).all() and (pts[:, 2] <= 2.5).all()
    n = len(SEPARATIONS)
    pairs = np.array([[0, 1 + k] for k in range(n)] + [[0, 0]] + [[1 + k, 1 + k] for k in range(n)])
    out = ll.run(m, [rl.job_of(m, ref, rl.factors_of(m, F), pts)], [pairs])
    assert (out.status == reconstruction.OK).all()
    got_diff, got_cross = mats(out.cov_diff_cal), cross(out.cross_cal)
    for k, (name, s, _) in enumerate(SEPARATIONS):
      want_diff, want_cross, Ca, Cb, Ja, Jb = exact(m, ref, sigma, F, pts[0], pts[1 + k])
      bound = diff_bound(Ja, Jb, F)
      err = float(np.abs(got_diff[k].astype(LD) - want_diff).max())
      naive = got_cross[n] + got_cross[n + 1 + k] - got_cross[k] - got_cross[k].T
      err_naive = float(np.abs(naive.astype(LD) - want_diff).max())
      size = float(np.abs(want_diff).max())
      cancellation = (np.linalg.norm(Ja) ** 2 + np.linalg.norm(Jb) ** 2) * np.linalg.norm(sigma, 2) / size
      print(f"{label} reference {ref} pair {name}: |cov_diff| {size:.3g}; difference form off by {err:.3g} ({err / size:.3g} relative), bound "
            f"{bound:.3g}; naive C_a + C_b - C_ab - C_ab^T off by {err_naive:.3g} ({err_naive / size:.3g} relative); cancellation {cancellation:.3g}")
      assert err <= bound, (label, name)
      if name == "1 mm":
        assert cancellation >= 1e4, (label, cancellation)          # (the input: the case does cancel)
      cbound = 1000.0 * EPS * np.linalg.norm(Ja) * np.linalg.norm(Jb) * np.linalg.norm(sigma, 2)
      cerr = float(np.abs(got_cross[k].astype(LD) - want_cross).max())
      print(f"    cross_cal off by {cerr:.3g}, bound {cbound:.3g}, |cross| {float(np.abs(want_cross).max()):.3g}")
      assert cerr <= cbound, (label, name)
      assert np.linalg.eigvalsh(got_diff[k]).min() >= -EPS * np.abs(got_diff[k]).max()
      assert abs(out.length[k] - s) <= 4 * EPS * np.abs(pts).max()


# ---- 2. identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", [None, 2], ids=["rig", "camera"])
def test_identities(ref):
  m, _ = rl.group_rig(3, 3)
  sigma = held_sigma(m)
  F = uncertainty.factor(sigma)
  pts = np.array([[0.0, 0.0, 1.0], [0.1, -0.15, 1.5], [-0.2, 0.1, 2.5], [0.101, -0.15, 1.5]])
  pairs = np.array([[0, 0], [1, 1], [2, 2], [3, 3], [0, 1], [1, 0], [1, 3], [3, 1], [2, 0], [0, 2]])
  job = rl.job_of(m, ref, rl.factors_of(m, F), pts)
  out = ll.run(m, [job], [pairs], sigma2=0.3)
  point = rl.run(m, [job], sigma2=0.3)
  assert (out.status == reconstruction.OK).all() and (point.status == reconstruction.OK).all()
  same = pairs[:, 0] == pairs[:, 1]
  # a == b: exactly 0, no length, and the cross covariance is the point's own covariance
  assert (out.cov_diff_cal[same] == 0).all() and (out.cov_diff_noise[same] == 0).all() and (out.length[same] == 0).all()
  assert np.isnan(out.length_var_cal[same]).all() and np.isnan(out.length_var_noise[same]).all()
  own = rl.whitened_difference(cross(out.cross_cal)[:4], mats(point.cov_cal))
  print(f"reference {ref}: cross(a, a) - cov_cal whitened {own.max():.3g}")
  assert own.max() <= 1e-13
  assert np.isfinite(out.length_var_cal[~same]).all() and (out.length_var_noise[~same] > 0).all()
  # cross(b, a) = cross(a, b)^T within the bound of the long-double test
  for k in (4, 6, 8):
    a, b = pairs[k]
    Ja, _ = rl.stored_rows(m, ref, pts[a])
    Jb, _ = rl.stored_rows(m, ref, pts[b])
    cbound = 1000.0 * EPS * np.linalg.norm(Ja) * np.linalg.norm(Jb) * np.linalg.norm(sigma, 2)
    assert np.abs(cross(out.cross_cal)[k + 1] - cross(out.cross_cal)[k].T).max() <= cbound
    assert np.abs(out.cov_diff_cal[k + 1] - out.cov_diff_cal[k]).max() <= diff_bound(Ja, Jb, F)
    # the noise of the difference is the sum of the two points' noise
    want = point.cov_noise[a] + point.cov_noise[b]
    assert (np.abs(out.cov_diff_noise[k] - want) <= 4 * EPS * np.abs(want)).all()
    assert out.views_a[k] == point.views[a] and out.views_b[k] == point.views[b]
  lam = np.linalg.eigvalsh(mats(out.cov_diff_cal))
  assert (lam[:, 0] >= -EPS * np.abs(out.cov_diff_cal).max(axis=1)).all()
  # r = 0 and a zero factor: exact zeros
  for width in (0, 3):
    zero = ll.run(m, [rl.job_of(m, ref, [(np.zeros((24, width)), False)] * 3, pts)], [pairs])
    assert (zero.status == reconstruction.OK).all() and (zero.cov_diff_cal == 0).all() and (zero.cross_cal == 0).all()
    assert (zero.length_var_cal[~same] == 0).all() and np.isnan(zero.length_var_cal[same]).all()
    assert (zero.cov_diff_noise[~same] != 0).any()


# ---- 3. the length does not know the frame -----------------------------------------------------------------------------------
MC_MEMBERS = (0, 2, 5)           # 5 Brown-Conrady coefficients, 8 (rational), Kannala-Brandt


def adjoint(T):
  R, t = T[:3, :3], T[:3, 3]
  A = np.zeros((6, 6))
  A[:3, :3] = R
  A[3:, :3] = uncertainty.skew(t) @ R
  A[3:, 3:] = R
  return A


def test_length_variance_is_the_same_in_every_frame():
  """Sigma = a small full covariance + a LARGE common motion of the rig frame (per camera Ad_{T_c} delta, taken to its stored rvec | tvec
  by the inverse of the stored map's pose block).  In the rig frame each end then moves by far more than their difference (checked on
  the CPU: cov_cal exceeds cov_diff_cal by >= 1e3), and length_var_cal must still agree with the value in the frame of every camera
  -- where the common motion cancels -- within 1000 eps (|J_a|^2 + |J_b|^2) |Sigma|_2 / length_var_cal relative, J of the rig frame"""
  m, _ = rl.group_rig(0, 3, members=MC_MEMBERS)
  maps = rl.stored_maps(m)
  sizes = [M.shape[1] for M in maps]
  p = sum(sizes)
  first = np.concatenate([[0], np.cumsum(sizes)])
  sigma = 1e-10 * ul.random_spd(p, 11)
  for k in range(6):
    delta = np.zeros(6)
    delta[k] = 1e-2
    v = np.zeros(p)
    for c, M in enumerate(maps):
      v[first[c + 1] - 6:first[c + 1]] = np.linalg.solve(M[18:, -6:], adjoint(m.poses[c]) @ delta)
    sigma += np.outer(v, v)
  skew_at = [int(first[c]) + 4 for c in range(3)]
  sigma[skew_at, :] = 0.0
  sigma[:, skew_at] = 0.0
  F = uncertainty.factor(sigma)
  pts = np.array([[0.05, -0.08, 1.5], [0.05, -0.08, 1.5] + 0.02 * unit([1.0, 0.5, 0.2])])
  factors = rl.factors_of(m, F)
  rig_frame = ll.run(m, [rl.job_of(m, None, factors, pts)], [[[0, 1]]])
  assert rig_frame.status[0] == reconstruction.OK
  want_diff, _, Ca, Cb, Ja, Jb = exact(m, None, sigma, F, pts[0], pts[1])
  ratio = min(float(np.trace(Ca)), float(np.trace(Cb))) / float(np.trace(want_diff))
  print(f"rig frame: trace cov_cal of an end / trace cov_diff_cal = {ratio:.3g}")
  assert ratio >= 1e3
  var = rig_frame.length_var_cal[0]
  tol = 1000.0 * EPS * (np.linalg.norm(Ja) ** 2 + np.linalg.norm(Jb) ** 2) * np.linalg.norm(sigma, 2) / var
  for ref in range(3):
    cam_frame = ll.run(m, [rl.job_of(m, ref, factors, pts)], [[[0, 1]]])
    assert cam_frame.status[0] == reconstruction.OK
    rel = abs(cam_frame.length_var_cal[0] - var) / var
    print(f"length_var_cal rig frame {var:.17g}, frame of camera {ref} {cam_frame.length_var_cal[0]:.17g}: relative difference {rel:.3g}, "
          f"tolerance {tol:.3g}; length_var_noise {rig_frame.length_var_noise[0]:.6g} / {cam_frame.length_var_noise[0]:.6g}")
    assert rel <= tol
    assert abs(cam_frame.length_var_noise[0] - rig_frame.length_var_noise[0]) <= 1e-12 * rig_frame.length_var_noise[0]
    assert cam_frame.length[0] == rig_frame.length[0]


# ---- 4. meaning ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", [None, 2], ids=["rig", "camera"])
def test_monte_carlo_meaning(ref):
  """N = 200 000 samples of the stored parameters from N(theta, Sigma), the SAME samples pushed through one restated chain per end
  (keep the end's noise-free pixels, re-triangulate, express in the reference): the sample variance of |X_a - X_b| over
  length_var_cal, and the sample covariance of X_a - X_b whitened by cov_diff_cal, are 1 and I within 5 sqrt(2 / (N - 1)).  Pairs 0.2 m
  apart across and along the line of sight; Sigma scaled as in the point entry's test (a standard deviation of 2e-4 of the distance)."""
  m, cams = rl.group_rig(0, 3, members=MC_MEMBERS)
  N = 200000
  centre = np.array([0.05, -0.08, 1.2])
  geometries = {"across": unit([1.0, 0.1, 0.0]), "along": unit(centre)}
  chain0 = rr.Chain(cams, m.rtvecs, m.fix_aspect, centre, range(3))
  p = len(chain0.theta)
  scales = chain0.steps / chain0.steps.max()
  sigma = ul.random_spd(p, 21, 1.0) * np.outer(scales, scales)
  skew_at = [int(chain0.first[s]) + 4 for s in range(3)]
  sigma[skew_at, :] = 0.0                           # (the skew enters no projection and is not a parameter of the device)
  sigma[:, skew_at] = 0.0
  job = lambda sg, pts: rl.job_of(m, ref, rl.factors_of(m, uncertainty.factor(sg)), pts)
  first = rl.run(m, [job(sigma, centre[None])])
  assert first.status[0] == reconstruction.OK
  sigma = sigma * (2e-4 * np.linalg.norm(centre)) ** 2 / np.linalg.eigvalsh(mats(first.cov_cal)[0]).max()
  F = uncertainty.factor(sigma)
  thetas = chain0.theta[None] + np.random.default_rng(100).normal(size=(N, F.shape[1])) @ F.T
  bound = 5.0 * np.sqrt(2.0 / (N - 1))
  for name, direction in geometries.items():
    pts = np.array([centre - 0.1 * direction, centre + 0.1 * direction])
    out = ll.run(m, [job(sigma, pts)], [[[0, 1]]])
    assert out.status[0] == reconstruction.OK
    ends = []
    for X in pts:
      chain = rr.Chain(cams, m.rtvecs, m.fix_aspect, X, range(3))
      samples_of = rr.SampleChain(chain)
      ends.append(samples_of.express(thetas, samples_of.triangulate(thetas), ref))
    d = ends[0] - ends[1]
    var_ratio = np.var(np.linalg.norm(d, axis=1), ddof=1) / out.length_var_cal[0]
    Li = np.linalg.inv(np.linalg.cholesky(mats(out.cov_diff_cal)[0]))
    dev = np.abs(Li @ np.cov(d.T) @ Li.T - np.eye(3)).max()
    print(f"monte carlo reference {ref} {name}: sample variance of the length / length_var_cal - 1 = {var_ratio - 1.0:+.4f}, whitened sample "
          f"covariance of the difference - I = {dev:.4f}, bound {bound:.4f}; length std {np.sqrt(out.length_var_cal[0]):.3g} m against "
          f"{np.sqrt(np.trace(np.cov(ends[0].T))):.3g} m of one end")
    assert abs(var_ratio - 1.0) <= bound and dev <= bound, (ref, name)


# ---- 5. the first-order law ----------------------------------------------------------------------------------------------------
LAW_DISTANCE = 12.0


def law_case():
  """rl.meaning_case() and a bar across the line of sight (along x of camera 0) centred on its axis at LAW_DISTANCE, 1 cm and 5 mm long;
  the pairs: the two bars, and each end of the first with itself (cross_cal of (p, p) is the end's cov_cal).
  The distance: across the line of sight a length L = dx Z errs by L dZ / Z, and dZ / Z grows with Z like each end's own lateral
  error, so length_std / naive hardly depends on the distance -- it is a property of the fixture's covariance and of L alone.  In
  long double (test_first_order_law, no code under test) a 1 cm bar of this fixture gives 0.128 at 0.75 m, 0.108 at 1.5 m, 0.102 at
  3 m, 0.0999 at 6 m, 0.0994 at 12 m, 0.0992 at 24 m: the 'less than a tenth' of the law holds from 6 m on, by 0.65 % at 12 m, which
  is 1e9 times the rounding of either build."""
  m, factors, _, ref = rl.meaning_case()
  pts = np.concatenate([ll.bar_points(m, 0, LAW_DISTANCE, 0.01, False), ll.bar_points(m, 0, LAW_DISTANCE, 0.005, False)])
  return m, factors, pts, ref, [[0, 1], [2, 3], [0, 0], [1, 1]]


def check_first_order_law(out, m, ref, pts):
  """halving the separation halves length_std_cal (d_j is linear in the separation; the second-order term is of relative size
  separation / d < 1 %), and at 1 cm the calibration's part of the length is less than a tenth of the naive sqrt(u^T (C_a + C_b) u)"""
  assert (out.status == reconstruction.OK).all()
  std = np.sqrt(out.length_var_cal[:2])
  u = m.poses[ref][:3, :3] @ unit(pts[0] - pts[1])
  naive = np.sqrt(u @ (cross(out.cross_cal)[2] + cross(out.cross_cal)[3]) @ u)
  print(f"length_std_cal at 1 cm {std[0]:.4g}, at 5 mm {std[1]:.4g}: ratio {std[0] / std[1]:.4f}; naive sqrt(u^T (C_a + C_b) u) {naive:.4g}")
  assert 1.8 <= std[0] / std[1] <= 2.2
  assert std[0] < 0.1 * naive


def test_first_order_law():
  m, factors, pts, ref, pairs = law_case()
  out = ll.run(m, [rl.job_of(m, ref, factors, pts)], [pairs])
  check_first_order_law(out, m, ref, pts)
  # the fixture itself, in long double: the same inequality without the code under test
  Ja, _ = rl.stored_rows(m, ref, pts[0])
  Jb, _ = rl.stored_rows(m, ref, pts[1])
  W = np.concatenate([w for w, _ in factors]).astype(LD)
  Ga, _ = rl.query_rows(m, ref, pts[0])
  Gb, _ = rl.query_rows(m, ref, pts[1])
  u = (m.poses[ref][:3, :3] @ unit(pts[0] - pts[1])).astype(LD)
  za, zb = Ga.astype(LD) @ W, Gb.astype(LD) @ W
  exact_std = np.sqrt(float((((za - zb).T @ u) ** 2).sum()))
  exact_naive = np.sqrt(float(((za.T @ u) ** 2).sum() + ((zb.T @ u) ** 2).sum()))
  print(f"long double: length std {exact_std:.4g}, naive {exact_naive:.4g}")
  assert exact_std < 0.1 * exact_naive


# ---- 6. statuses and refusals --------------------------------------------------------------------------------------------------
def test_statuses_with_ok_neighbours():
  m, _ = rl.group_rig(3, 3)
  factors = rl.random_factors(m, 4, 2)[0]
  good, near = np.array([0.0, 0.0, 1.5]), np.array([0.05, 0.02, 1.6])
  pts = np.array([good, near, [0.0, 0.0, -1.0], good])
  masks = np.array([7, 7, 7, 2], dtype=np.uint64)
  # the b end: behind the cameras; masked down to one view; then both orders, with OK pairs between them in one tile
  pairs = np.array([[0, 1], [0, 2], [1, 0], [0, 3], [0, 1], [2, 0], [3, 1], [1, 1]])
  out = ll.run(m, [rl.job_of(m, None, factors, pts, masks)], [pairs])
  TF, OK = reconstruction.TOO_FEW, reconstruction.OK
  assert list(out.status) == [OK, TF, OK, TF, OK, TF, TF, OK]
  bad = out.status != OK
  for k in ll.COVARIANCES:
    assert np.isnan(out[k][bad]).all(), k
    assert np.isfinite(out[k][~bad][:-1]).all(), k
  assert np.isfinite(out.length).all() and list(out.views_b[[1, 3]]) == [0, 2] and list(out.views_a[[5, 6]]) == [0, 2]
  assert out.cov_diff_cal[0].tobytes() == out.cov_diff_cal[4].tobytes()
  # two cameras with one centre: DEGENERATE; an unconstrained view: UNCONSTRAINED; the status of a comes first
  twin = uncertainty.RigModel(m.cameras[:2], np.stack([m.poses[0], m.poses[0]]))
  twin.poses[1, :3, :3] = m.poses[1, :3, :3]
  twin.poses[1, :3, 3] = m.poses[1, :3, :3] @ (m.poses[0, :3, :3].T @ m.poses[0, :3, 3])
  twin.rtvecs = ul.transform.from_matrix(twin.poses).reshape(-1, 6)
  out = ll.run(twin, [rl.job_of(twin, None, factors[:2], np.array([good, near]))], [[[0, 1]]])
  assert out.status[0] == reconstruction.DEGENERATE and np.isnan(out.cov_diff_cal).all() and np.isnan(out.cov_diff_noise).all()
  loose = [(factors[0][0], True)] + factors[1:]
  out = ll.run(m, [rl.job_of(m, None, loose, pts, np.array([6, 7, 7, 2], dtype=np.uint64))], [[[0, 1], [1, 0], [0, 0], [3, 1], [1, 3]]])
  U = reconstruction.UNCONSTRAINED
  assert list(out.status) == [U, U, OK, TF, U]
  assert np.isnan(out.cross_cal[[0, 1, 3, 4]]).all() and np.isfinite(out.cross_cal[2]).all()


def test_refused_calls_name_the_argument():
  m, _ = rl.group_rig(3, 3)
  factors = rl.random_factors(m, 4, 2)[0]
  pts = np.array([[0.0, 0.0, 1.5], [0.05, 0.02, 1.6]])
  job = rl.job_of(m, None, factors, pts)
  for bad in ([[0, 2]], [[0, 1], [-1, 0]], [[2, 2]]):
    with pytest.raises(RuntimeError, match=r"mcba_reconstruction_pairs: pairs: pair \d+ .*outside \[0, n = 2\)"):
      ll.run(m, [job], [bad])
  with pytest.raises(RuntimeError, match=r"job 1\): index 18 is outside"):     # the second job's pairs index ITS points
    ll.run(m, [rl.job_of(m, None, factors, np.tile(pts, (10, 1))), job], [[[0, 19]], [[0, 1], [1, 18]]])
  nine, _ = rl.group_rig(0, 9)
  with pytest.raises(RuntimeError, match="mcba_reconstruction_pairs: job 0: G = 9"):
    ll.run(nine, [rl.job_of(nine, None, rl.random_factors(nine, 2, 1)[0], pts)], [[[0, 1]]])
  with pytest.raises(RuntimeError, match="r = 129"):
    ll.run(m, [rl.job_of(m, None, [(np.zeros((24, 129)), False)] * 3, pts)], [[[0, 1]]])
  for bad in (np.nan, np.inf):
    with pytest.raises((RuntimeError, ValueError), match="points: point 1 is not finite"):
      ll.run(m, [rl.job_of(m, None, factors, np.array([pts[0], [0.0, bad, 1.0]]))], [[[0, 1]]])
  with pytest.raises(RuntimeError, match="sigma2"):
    ll.run(m, [job], [[[0, 1]]], sigma2=0.0)
  for out in (ll.run(m, [job], [np.zeros((0, 2))]), ll.run(m, [], [])):     # zero pairs: empty arrays, nothing is touched
    assert out.cov_diff_cal.shape == (0, 6) and out.cross_cal.shape == (0, 9) and out.status.shape == (0,)


# ---- 7. Calibration ------------------------------------------------------------------------------------------------------------
def stand_in_covariance(c, seed=4):
  """a covariance struct over the shared layout of the Calibration c (cameras and camera poses), camera 0's pose held"""
  camera_index, pose_index = c._shared_layout()
  index = np.concatenate([np.concatenate([a, b]) for a, b in zip(camera_index, pose_index)])
  shared = ul.random_spd(len(index), seed, 1e-8)
  n = len(np.asarray(c.param_vec))
  std, held = np.full(n, np.nan), np.zeros(n, dtype=bool)
  std[index] = np.sqrt(np.diag(shared))
  held[pose_index[0]] = True
  return struct(shared=shared, shared_index=index, std=std, held=held, sigma2=0.25, dof=100)


def test_calibration_length_uncertainty_is_the_functional_entry():
  c = mirror(synthetic.make_rig("tiny")).enable(cameras=True)
  cov = stand_in_covariance(c)
  c.covariance = lambda hold=None, sigma2=None: cov
  start, _ = c._rig_poses()
  f = int(np.flatnonzero(np.asarray(c.motion.valid))[0])
  world = c.world_points.points[0][c.world_points.valid[0]]
  X = world @ np.asarray(start)[f, :3, :3].T + np.asarray(start)[f, :3, 3]
  A, B = X, X[::-1]
  camera_index, pose_index = c._shared_layout()
  for reference in (None, 1):
    with ll.host_backend():
      got = c.length_uncertainty(A, B, reference=reference)
      want = reconstruction.pair_uncertainty(list(c.cameras), np.asarray(c.camera_poses.poses), cov, camera_index, pose_index,
                                             points_a=A, points_b=B, reference=reference,
                                             rtvecs=np.asarray(c.camera_poses.params, dtype=np.float64).reshape(-1, 6))
    assert (got.status == reconstruction.OK).sum() >= len(A) // 2, got.status
    for k in want.keys():
      assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k
    assert got.sigma2 == cov.sigma2 and got.cov_diff_cal.shape == (len(A), 3, 3) and got.cross_cal.shape == (len(A), 3, 3)
    ok = got.status == reconstruction.OK
    assert np.array_equal(got.cov_diff_total[ok], got.cov_diff_cal[ok] + got.cov_diff_noise[ok])
    far = ok & (got.length > 0)
    assert (got.length_std_cal[far] > 0).all() and (got.length_std[far] >= got.length_std_noise[far]).all()


def test_default_pairs_are_the_farthest_corners_and_boards_are_refused():
  c = mirror(synthetic.make_rig("tiny")).enable(cameras=True)
  pairs, defined = c.length_pairs()
  assert pairs.shape == (c.size.boards, c.size.points, 2) and defined.shape == pairs.shape[:2]
  for b, board in enumerate(c.boards):
    x = np.asarray(board.adjusted_points, dtype=np.float64).reshape(-1, 3)
    far = np.argmax(np.linalg.norm(x[:, None] - x[None], axis=-1), axis=1)       # (argmax: the first, so the lowest index)
    want = np.stack([np.arange(len(x)), far], axis=1)
    assert np.array_equal(pairs[b, :len(x)], want) and defined[b, :len(x)].all() and not defined[b, len(x):].any()
    assert (far != np.arange(len(x))).all()
  given, given_defined = c.length_pairs([[0, 1], [1, 10 ** 6]])
  assert given.shape == (c.size.boards, 2, 2) and given_defined[:, 0].all() and not given_defined[:, 1].any()
  locked = c.enable(boards=True)
  for call in (lambda: locked.length_errors(), lambda: locked.length_uncertainty(np.zeros((1, 3)), np.ones((1, 3))),
               lambda: locked.report_length_uncertainty()):
    with pytest.raises(ValueError, match="boards"):
      call()


# ---- 8. sanitizer ----------------------------------------------------------------------------------------------------------------
def test_sanitized_program(tmp_path):
  """the edge cases of the pair list in a stand-alone program under AddressSanitizer + UBSan (CPU only, nothing loaded into Python):
  the host header and the driver's planning code"""
  r = host_build.sanitized_program("length_host", "length_sanitize_main.cpp", tmp_path)
  assert r.returncode == 0 and "length sanitize run: ok" in r.stdout, r.stdout + r.stderr
