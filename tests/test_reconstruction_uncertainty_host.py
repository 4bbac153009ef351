"""The reconstruction-uncertainty mathematics (csrc/mcba_recon.h) in its g++ build and the marshalling of
multical_amd.reconstruction on top of it, against an independent numpy restatement without analytic derivatives
(reconstruction_uncertainty_reference.py).  No GPU."""
import numpy as np
import pytest

from multical_amd import reconstruction, uncertainty
from multical_amd.structs import struct

import host_build
import reconstruction_uncertainty_host_lib as rl
import reconstruction_uncertainty_reference as rr
import uncertainty_host_lib as ul

EPS = np.finfo(np.float64).eps
GROUP_SIZES = (2, 3, 5)
MARGIN = 60.0          # px: at a distance of one baseline the outer cameras see the point just outside their 200 px; they stay views


def mats(c6):
  return reconstruction.covariance_matrices(c6)


@pytest.mark.parametrize("b", range(9), ids=rl.CAMERA_IDS)
def test_jacobian_against_richardson_differences(b):
  """the header's rows G = -H^-1 [B_1 .. B_G] (+ the reference term), taken to the stored parameters of every camera of the group
  (fx fy cx cy skew dist, rvec, tvec) by the stored maps, against Richardson-extrapolated central differences of the restated chain
  (perturb one stored parameter, keep the noise-free pixels, re-triangulate to convergence): every entry within 10 x the
  restatement's own error estimate, floored at 1e-12 of the row's norm.  Camera b leads a group of 2, 3 or 5; both references;
  points on the axis and at the edge of the common field, at 1 and 10 baselines."""
  G = GROUP_SIZES[b % 3]
  m, cams = rl.group_rig(b, G)
  base = rl.SPACING * (G - 1)
  a = G - 1
  worst = 0.0
  for X in rl.field_points(m, (base, 10.0 * base)):
    chain = rr.Chain(cams, m.rtvecs, m.fix_aspect, X, range(G))
    restated = chain.jacobian([None, a])
    for ref in (None, a):
      J, status = rl.stored_rows(m, ref, X, margin=MARGIN)
      assert status == reconstruction.OK, (b, X, ref, status)
      Jr, err = restated[ref]
      tol = 10.0 * np.maximum(err, 1e-12 * np.linalg.norm(Jr, axis=1)[:, None])
      ratio = float((np.abs(J - Jr) / tol).max())
      worst = max(worst, ratio)
      print(f"camera {rl.CAMERA_IDS[b]} G {G} reference {ref} point {X}: |dJ| / tolerance {ratio:.3g}, |dJ| {np.abs(J - Jr).max():.3g}, "
            f"|J| {np.linalg.norm(Jr):.3g}")
      assert ratio <= 1.0, (b, X, ref)
  print(f"camera {rl.CAMERA_IDS[b]}: worst |dJ| / tolerance {worst:.3g}")


def test_views_are_all_cameras_under_the_margin():
  """(the Jacobian test's premise) with the margin every camera of every group is a view of every point"""
  for b in range(9):
    G = GROUP_SIZES[b % 3]
    m, _ = rl.group_rig(b, G)
    base = rl.SPACING * (G - 1)
    pts = rl.field_points(m, (base, 10.0 * base))
    out = rl.run(m, [rl.job_of(m, None, rl.random_factors(m, 3, 1)[0], pts)], margin=MARGIN)
    assert (out.status == reconstruction.OK).all() and (out.n_views == G).all() and (out.views == (1 << G) - 1).all(), (b, out)


# ---- covariance ------------------------------------------------------------------------------------------------------------------
def check_covariance(m, ref, sigma, pts, label, min_cancellation=None):
  """cov_cal of the host build against J Sigma J^T in np.longdouble, J the header's own rows (pinned by the test above):
  |dC| <= 1000 eps |J|_F^2 |Sigma|_2"""
  F = uncertainty.factor(sigma)
  out = rl.run(m, [rl.job_of(m, ref, rl.factors_of(m, F), pts)])
  assert (out.status == reconstruction.OK).all()
  got = mats(out.cov_cal)
  for i, X in enumerate(pts):
    J, _ = rl.stored_rows(m, ref, X)
    Jl, Sl = J.astype(np.longdouble), sigma.astype(np.longdouble)
    want = (Jl @ Sl @ Jl.T).astype(np.float64)
    scale = np.linalg.norm(J) ** 2 * np.linalg.norm(sigma, 2)
    diff = np.abs(got[i] - want).max()
    print(f"{label} point {X}: |dC| {diff:.3g}, bound {1000 * EPS * scale:.3g}, |C| {np.abs(want).max():.3g}, cancellation "
          f"{scale / np.abs(want).max():.3g}")
    assert diff <= 1000.0 * EPS * scale, (label, i)
    assert np.linalg.eigvalsh(got[i]).min() >= -EPS * np.abs(got[i]).max()
    if min_cancellation is not None:
      assert scale / np.abs(want).max() >= min_cancellation, (label, i)


COV_POINTS = np.array([[0.0, 0.0, 1.0], [0.1, -0.15, 1.5], [-0.2, 0.1, 2.5]])


@pytest.mark.parametrize("ref", [None, 1], ids=["rig", "camera"])
def test_covariance_with_held_block_and_rank_deficiency(ref):
  m, _ = rl.group_rig(3, 3)
  p = sum(M.shape[1] for M in rl.stored_maps(m))
  held = ul.random_spd(p, 3)
  lo = 5 + m.n_dist[0]
  held[lo:lo + 6, :] = 0.0                     # the pose of slot 0 is held
  held[:, lo:lo + 6] = 0.0
  check_covariance(m, ref, held, COV_POINTS, f"held pose, reference {ref}")
  A = np.random.default_rng(5).normal(size=(p, 5)) * 1e-3
  check_covariance(m, ref, A @ A.T, COV_POINTS, f"rank 5, reference {ref}")


def test_covariance_that_cancels():
  """four parameters (cx and the rotation about y of two cameras) correlated along the direction that leaves the point where it is:
  cov_cal is more than 1e4 below |J|^2 |Sigma|, and still within the bound"""
  m, _ = rl.group_rig(0, 2)
  X = COV_POINTS[:1]
  J, _ = rl.stored_rows(m, None, X[0])
  p = J.shape[1]
  n0 = 5 + m.n_dist[0] + 6
  K = [2, 5 + m.n_dist[0] + 1, n0 + 2, n0 + 5 + m.n_dist[1] + 1]
  null = np.linalg.svd(J[:, K])[2][-1]
  v = np.zeros(p)
  v[K] = null / np.abs(null).max()
  sigma = 1e-2 * np.outer(v, v) + 1e-6 * ul.random_spd(p, 9)
  check_covariance(m, None, sigma, X, "correlated centres and rotations", min_cancellation=1e4)


# ---- meaning ---------------------------------------------------------------------------------------------------------------------
MC_MEMBERS = (0, 2, 5)           # 5 Brown-Conrady coefficients, 8 (rational), Kannala-Brandt


@pytest.mark.parametrize("ref", [None, 2], ids=["rig", "camera"])
def test_monte_carlo_meaning(ref):
  """N = 200 000 samples of the stored parameters from N(theta, Sigma) pushed through the restated chain (keep the noise-free pixels,
  re-triangulate, express in the reference): the sample covariance whitened by cov_cal is I within 5 sqrt(2 / (N - 1)).  Sigma is
  scaled to a standard deviation of 2e-4 of the distance, which keeps the second-order term (relative size: a few times that) below
  a tenth of the bound.  A wrong sign of -H^-1 or of the reference term fails this by O(1)."""
  m, cams = rl.group_rig(0, 3, members=MC_MEMBERS)
  N = 200000
  X = np.array([0.05, -0.08, 1.2])
  chain = rr.Chain(cams, m.rtvecs, m.fix_aspect, X, range(3))
  samples_of = rr.SampleChain(chain)
  for s in range(3):                               # the vectorised projection is the restated one
    a = samples_of.pixel(chain.theta[None], s, X[None])[0]
    assert np.abs(a - chain.q[s]).max() < 1e-11
  p = len(chain.theta)
  scales = chain.steps / chain.steps.max()
  sigma = ul.random_spd(p, 21, 1.0) * np.outer(scales, scales)
  skew_at = [int(chain.first[s]) + 4 for s in range(3)]
  sigma[skew_at, :] = 0.0                           # (the skew enters no projection and is not a parameter of the device)
  sigma[:, skew_at] = 0.0
  job = lambda sg: rl.job_of(m, ref, rl.factors_of(m, uncertainty.factor(sg)), X[None])
  first = rl.run(m, [job(sigma)])
  assert first.status[0] == reconstruction.OK
  scale = (2e-4 * np.linalg.norm(X)) ** 2 / np.linalg.eigvalsh(mats(first.cov_cal)[0]).max()
  sigma = sigma * scale
  Cm = mats(rl.run(m, [job(sigma)]).cov_cal)[0]
  rng = np.random.default_rng(100)
  F = uncertainty.factor(sigma)
  thetas = chain.theta[None] + rng.normal(size=(N, F.shape[1])) @ F.T
  Xs = samples_of.express(thetas, samples_of.triangulate(thetas), ref)
  sample_cov = np.cov(Xs.T)
  Li = np.linalg.inv(np.linalg.cholesky(Cm))
  dev = np.abs(Li @ sample_cov @ Li.T - np.eye(3)).max()
  bound = 5.0 * np.sqrt(2.0 / (N - 1))
  print(f"monte carlo reference {ref}: Sigma scaled by {scale:.3g}; whitened sample covariance - I = {dev:.4f}, bound {bound:.4f}; std "
        f"{np.sqrt(np.diag(Cm))}")
  assert dev <= bound


def adjoint(T):
  R, t = T[:3, :3], T[:3, 3]
  A = np.zeros((6, 6))
  A[:3, :3] = R
  A[3:, :3] = uncertainty.skew(t) @ R
  A[3:, 3:] = R
  return A


def test_gauge_a_common_motion_of_the_rig_frame_cancels_in_the_camera_form():
  """the column of a common rigid motion delta of the rig frame (per camera Ad_{T_c} delta in its six pose rows): its z vanishes in the
  camera form, |z_cam| <= 1e4 eps cond(H) |z_rig|, and does not in the rig form"""
  m, _ = rl.group_rig(4, 5)
  pts = np.array([[0.05, -0.1, 1.0], [-0.3, 0.2, 3.0]])
  for k in range(6):
    delta = np.zeros(6)
    delta[k] = 1.0
    factors = []
    for c in range(5):
      W = np.zeros((24, 1))
      W[18:, 0] = adjoint(m.poses[c]) @ delta
      factors.append((W, False))
    rig_form = rl.run(m, [rl.job_of(m, None, factors, pts)])
    cam_form = rl.run(m, [rl.job_of(m, 2, factors, pts)])
    assert (rig_form.status == reconstruction.OK).all() and (cam_form.status == reconstruction.OK).all()
    for i in range(len(pts)):
      cond = np.linalg.cond(mats(rig_form.cov_noise)[i])
      z_rig = np.sqrt(np.trace(mats(rig_form.cov_cal)[i]))
      z_cam = np.sqrt(np.trace(mats(cam_form.cov_cal)[i]))
      print(f"delta {k} point {pts[i]}: |z_rig| {z_rig:.3g} |z_cam| {z_cam:.3g} cond(H) {cond:.3g} bound {1e4 * EPS * cond * z_rig:.3g}")
      assert z_rig > 1e-3
      assert z_cam <= 1e4 * EPS * cond * z_rig


def test_noise_covariance_is_that_of_the_triangulation():
  """at noise-free observations of the same point and views cov_noise (rig form) is the cov of the host build of mcba_triangulate.h
  within 1e3 eps cond(H) of its largest entry, on the points with cond(H) <= 1e4"""
  import triangulate_host_lib as tl
  rig = tl.make_rig(3, 1, 65)
  r = tl.run(rig, points=rig.clean, sigma=1.0)
  ok = r.status[0] == tl.triangulate.OK
  poses = np.tile(np.eye(4), (3, 1, 1))
  poses[:, :3, :] = rig.views[:, 0]
  m = uncertainty.RigModel(rig.cameras, poses)
  masks = (rig.valid[:, 0, :].astype(np.uint64) << np.arange(3, dtype=np.uint64)[:, None]).sum(axis=0).astype(np.uint64)
  pts = np.where(ok[:, None], r.points[0], [0.0, 0.0, 1.0])
  out = rl.run(m, [rl.job_of(m, None, rl.random_factors(m, 2, 1)[0], pts, masks)], sigma2=1.0)
  checked = 0
  for i in np.flatnonzero(ok):
    assert out.status[i] == reconstruction.OK and out.n_views[i] == r.n_views[0, i] and out.views[i] == masks[i]
    got, want = mats(out.cov_noise)[i], r.cov[0, i]
    cond = np.linalg.cond(want)
    if cond > 1e4:
      continue
    checked += 1
    assert np.abs(got - want).max() <= 1e3 * EPS * cond * np.abs(want).max(), (i, cond, np.abs(got - want).max() / np.abs(want).max())
  print(f"{checked} points with cond(H) <= 1e4 of {int(ok.sum())}")
  assert checked >= 20


# ---- statuses ----------------------------------------------------------------------------------------------------------------
def test_statuses_and_nan_outputs():
  m, _ = rl.group_rig(3, 3)
  factors = rl.random_factors(m, 4, 2)[0]
  good = np.array([0.0, 0.0, 1.5])
  pts = np.array([good, [1.2, 0.0, 1.5], [0.0, 0.0, -1.0], good, good])
  masks = np.array([7, 7, 7, 2, 5], dtype=np.uint64)
  out = rl.run(m, [rl.job_of(m, None, factors, pts, masks)])
  print(out.status, out.n_views, out.views)
  assert list(out.status) == [reconstruction.OK, reconstruction.TOO_FEW, reconstruction.TOO_FEW, reconstruction.TOO_FEW, reconstruction.OK]
  assert list(out.n_views) == [3, 1, 0, 1, 2] and list(out.views) == [7, out.views[1], 0, 2, 5]   # (one view inside the image; behind; masked)
  bad = out.status != reconstruction.OK
  assert np.isnan(out.cov_cal[bad]).all() and np.isnan(out.cov_noise[bad]).all()
  assert np.isfinite(out.cov_cal[~bad]).all() and np.isfinite(out.cov_noise[~bad]).all()
  # a camera that looks the other way drops out: the other two still triangulate
  back = uncertainty.RigModel(m.cameras, m.poses.copy())
  back.poses[0] = np.diag([-1.0, 1.0, -1.0, 1.0]) @ m.poses[0]
  back.rtvecs = ul.transform.from_matrix(back.poses).reshape(-1, 6)
  out = rl.run(back, [rl.job_of(back, None, factors, good[None])])
  assert out.status[0] == reconstruction.OK and out.views[0] == 6
  # two cameras with one centre: the rays are one and the same
  twin = uncertainty.RigModel(m.cameras[:2], np.stack([m.poses[0], m.poses[0]]))
  twin.poses[1, :3, :3] = m.poses[1, :3, :3]
  twin.poses[1, :3, 3] = m.poses[1, :3, :3] @ (m.poses[0, :3, :3].T @ m.poses[0, :3, 3])       # the centre of camera 0
  twin.rtvecs = ul.transform.from_matrix(twin.poses).reshape(-1, 6)
  out = rl.run(twin, [rl.job_of(twin, None, factors[:2], good[None])])
  assert out.status[0] == reconstruction.DEGENERATE and out.n_views[0] == 2 and np.isnan(out.cov_cal).all() and np.isnan(out.cov_noise).all()
  # an unconstrained view; an unconstrained reference camera that is no view; an unconstrained camera that is neither
  loose = [(factors[0][0], True)] + factors[1:]
  out = rl.run(m, [rl.job_of(m, None, loose, np.array([good, good]), np.array([7, 6], dtype=np.uint64))])
  assert list(out.status) == [reconstruction.UNCONSTRAINED, reconstruction.OK] and np.isnan(out.cov_cal[0]).all()
  out = rl.run(m, [rl.job_of(m, 0, loose, good[None], np.array([6], dtype=np.uint64))])
  assert out.status[0] == reconstruction.UNCONSTRAINED and np.isnan(out.cov_noise[0]).all()


def test_everything_held_is_exactly_zero():
  m, _ = rl.group_rig(3, 3)
  for ref in (None, 1):
    out = rl.run(m, [rl.job_of(m, ref, [(np.zeros((24, 0)), False)] * 3, COV_POINTS)])
    assert (out.status == reconstruction.OK).all() and (out.cov_cal == 0).all() and np.isfinite(out.cov_noise).all()
    out = rl.run(m, [rl.job_of(m, ref, [(np.zeros((24, 3)), False)] * 3, COV_POINTS)])
    assert (out.status == reconstruction.OK).all() and (out.cov_cal == 0).all()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refused_calls_name_the_argument():
  m, cams = rl.group_rig(3, 3)
  factors = rl.random_factors(m, 4, 2)[0]
  good = COV_POINTS[:1]
  with pytest.raises(RuntimeError, match="G = 1"):
    rl.run(m, [reconstruction.Job([0], None, factors[:1], good)])
  nine, _ = rl.group_rig(0, 9)
  with pytest.raises(RuntimeError, match="G = 9"):
    rl.run(nine, [rl.job_of(nine, None, rl.random_factors(nine, 2, 1)[0], good)])
  with pytest.raises(RuntimeError, match="r = 129"):
    rl.run(m, [rl.job_of(m, None, [(np.zeros((24, 129)), False)] * 3, good)])
  with pytest.raises(RuntimeError, match="reference 2 is not a camera of the group"):
    rl.run(m, [reconstruction.Job([0, 1], 2, factors[:2], good)])
  with pytest.raises(RuntimeError, match=r"cameras\[2\] = 0 is repeated"):
    rl.run(m, [reconstruction.Job([0, 1, 0], None, factors, good)])
  for bad in (np.nan, np.inf):
    with pytest.raises((RuntimeError, ValueError), match="points: point 1 is not finite"):
      rl.run(m, [rl.job_of(m, None, factors, np.array([good[0], [0.0, bad, 1.0]]))])
  odd = uncertainty.RigModel(m.cameras, m.poses)
  odd.cameras = list(m.cameras)
  odd.cameras[1] = struct(intrinsic=m.cameras[1].intrinsic, dist=np.zeros(6), model="pinhole", image_size=m.cameras[1].image_size)
  with pytest.raises(RuntimeError, match="unsupported camera family"):
    rl.run(odd, [rl.job_of(odd, None, factors, good)])
  with pytest.raises(RuntimeError, match="sigma2"):
    rl.run(m, [rl.job_of(m, None, factors, good)], sigma2=0.0)
  assert rl.run(m, []).cov_cal.shape == (0, 6)                          # nothing to do: no array is touched


def fake_covariance(m, seed=4):
  """(cov struct, camera_index, pose_index) over the stored blocks of the rig, camera 0's pose held"""
  sizes = [5 + n for n in m.n_dist]
  p = sum(sizes) + 6 * len(sizes)
  camera_index, pose_index, at = [], [], 0
  for n in sizes:
    camera_index.append(np.arange(at, at + n))
    pose_index.append(np.arange(at + n, at + n + 6))
    at += n + 6
  shared = ul.random_spd(p, seed, 1e-8)
  held = np.zeros(p, dtype=bool)
  held[pose_index[0]] = True
  return struct(shared=shared, shared_index=np.arange(p), std=np.sqrt(np.diag(shared)), held=held, sigma2=0.25, dof=100), camera_index, pose_index


def test_grid_form_and_list_form_return_the_same_bytes():
  m, cams = rl.group_rig(3, 3)
  cov, camera_index, pose_index = fake_covariance(m)
  for ref in (None, 1):
    with ul.uh.host_backend(), rl.host_backend():
      grid = reconstruction.reconstruction_uncertainty(cams, m.poses, cov, camera_index, pose_index, reference=ref, grid=(5, 4),
                                                       distances=[0.8, 2.0], rtvecs=m.rtvecs)
      flat = reconstruction.reconstruction_uncertainty(cams, m.poses, cov, camera_index, pose_index, reference=ref,
                                                       points=grid.points.reshape(-1, 3), rtvecs=m.rtvecs)
    assert grid.cov_cal.shape == (2, 4, 5, 3, 3) and grid.range_std_cal.shape == (2, 4, 5)
    assert (grid.status == reconstruction.OK).any()
    for k in ("cov_cal", "cov_noise", "cov_total", "n_views", "views", "status", "range_std_cal", "lateral_std_noise"):
      assert np.asarray(grid[k]).tobytes() == np.asarray(flat[k]).tobytes(), k
    ok = grid.status == reconstruction.OK
    assert (grid.range_std_cal[ok] > 0).all() and (grid.lateral_std_cal[ok] > 0).all()
    with pytest.raises(ValueError, match="reference 7 is not a camera of the group"):
      reconstruction.reconstruction_uncertainty(cams, m.poses, cov, camera_index, pose_index, reference=7, points=COV_POINTS)


def test_sanitized_program(tmp_path):
  """the edge cases once more in a stand-alone program under AddressSanitizer + UBSan (CPU only, nothing loaded into Python): the
  host header and the driver's planning code"""
  r = host_build.sanitized_program("recon_host", "recon_sanitize_main.cpp", tmp_path)
  assert r.returncode == 0 and "reconstruction sanitize run: ok" in r.stdout, r.stdout + r.stderr


def test_range_grows_with_the_square_of_the_distance_and_lateral_with_the_distance():
  """the fixture of the device test of the same name: on the optical axis of camera 0 at d and 2 d the calibration's range_std grows by
  more than 3 x (the d^2 law) and its lateral_std by less than 3 x (the d law, with the first-order terms of the intrinsics)"""
  m, factors, pts, ref = rl.meaning_case()
  out = rl.run(m, [rl.job_of(m, ref, factors, pts)])
  assert (out.status == reconstruction.OK).all()
  rng, lat = rl.range_lateral(m, ref, out, pts)
  print(f"range_std {rng}, ratio {rng[1] / rng[0]:.3f}; lateral_std {lat}, ratio {lat[1] / lat[0]:.3f}")
  assert rng[1] > 3.0 * rng[0] and lat[1] < 3.0 * lat[0]
