"""The projection-uncertainty mathematics (csrc/mcba_uncertainty.h) in its g++ build and the marshalling of
multical_amd.uncertainty on top of it, against an independent numpy restatement without analytic derivatives
(uncertainty_reference.py).  No GPU.  Measured values: profiles/projection_uncertainty_parity.txt."""
import functools

import numpy as np
import pytest

from multical_amd import uncertainty

import host_build
import uncertainty_host_lib as ul
import uncertainty_reference as ur

RHOS = [0.0, 0.5, 2.0]
# centre, edges and corners (ul.edge_pixels) dealt over the three distances: every (camera, mode) meets all nine
PIXELS_OF_RHO = {0.0: [0, 1, 5, 8], 0.5: [0, 2, 3, 6], 2.0: [0, 4, 7, 5]}
CAMERA_IDS = list(ul.uh.CAMERA_IDS) + ["tiny-0-fix_aspect"]
EPS = np.finfo(np.float64).eps


def neighbour(b):
  """the reference camera of the transfer jobs: the next one on the arc (10 cm away), so that the views overlap at 0.5 m"""
  return b - 1 if b > 0 else 1


def chain_of(b, a, rho):
  m, cams = ul.rig(), ul.source_cameras()
  return ur.Chain(cams[b], m.rtvecs[b], None if a is None else cams[a], None if a is None else m.rtvecs[a], rho, m.fix_aspect[b],
                  False if a is None else m.fix_aspect[a])


@pytest.mark.parametrize("b", range(9), ids=CAMERA_IDS)
def test_jacobian_against_richardson_differences(b):
  """the header's row pair, taken to the stored parameters (fx fy cx cy skew dist, rvec, tvec of b and of a) by
  RigModel.stored_map, against Richardson-extrapolated central differences of the restated chain: every entry within 10 x the
  restatement's own error estimate (the difference of its two finest levels), floored at 1e-12 of the row's norm"""
  m, px = ul.rig(), ul.edge_pixels()
  worst = 0.0
  for a in (None, neighbour(b)):
    for rho in RHOS:
      uv = px[PIXELS_OF_RHO[rho]]
      J, status = ul.query_rows(m, b, a, rho, uv)
      assert (status == uncertainty.OK).all(), (b, a, rho, status)
      chain = chain_of(b, a, rho)
      for i, q in enumerate(uv):
        Jr, err = chain.jacobian(q)
        tol = 10.0 * np.maximum(err, 1e-12 * np.linalg.norm(Jr, axis=1)[:, None])
        ratio = float((np.abs(J[i] - Jr) / tol).max())
        worst = max(worst, ratio)
        print(f"camera {CAMERA_IDS[b]} reference {a} rho {rho} pixel {q}: |dJ| / tolerance {ratio:.3g}, |dJ| {np.abs(J[i] - Jr).max():.3g}, "
              f"|J| {np.linalg.norm(Jr):.3g}")
        assert ratio <= 1.0, (b, a, rho, q)
  print(f"camera {CAMERA_IDS[b]}: worst |dJ| / tolerance {worst:.3g}")


def exact_covariance(J, sigma):
  Jl, Sl = J.astype(np.longdouble), sigma.astype(np.longdouble)
  return (Jl @ Sl @ Jl.T).astype(np.float64)


def blocks(cov3):
  return uncertainty.covariance_matrices(cov3)


def check_covariance(b, a, rho, sigma, uv, label, min_cancellation=None):
  """C of the host build against J Sigma J^T in np.longdouble, J the header's own row pair (pinned by the test above):
  |dC| <= 1000 eps |J|_F^2 |Sigma|_2, the backward error of a factor-and-product chain of K <= 48 with a margin of about 20 K"""
  m = ul.rig()
  J, status = ul.query_rows(m, b, a, rho, uv)
  assert (status == uncertainty.OK).all()
  cov, std, st = ul.run(m, [uncertainty.Job(b, a, np.inf if rho == 0 else 1.0 / rho, sigma, pixels=uv)])
  assert (st == uncertainty.OK).all()
  got = blocks(cov)
  for i in range(len(uv)):
    want = exact_covariance(J[i], sigma)
    scale = np.linalg.norm(J[i]) ** 2 * np.linalg.norm(sigma, 2)
    diff = np.abs(got[i] - want).max()
    print(f"{label} pixel {uv[i]}: |dC| {diff:.3g}, bound {1000 * EPS * scale:.3g}, |C| {np.abs(want).max():.3g}, cancellation "
          f"{scale / np.abs(want).max():.3g}")
    assert diff <= 1000.0 * EPS * scale, (label, i)
    assert np.linalg.eigvalsh(got[i]).min() >= -EPS * np.abs(got[i]).max()
    if min_cancellation is not None:
      assert scale / np.abs(want).max() >= min_cancellation, (label, i)


@pytest.mark.parametrize("a", [None, 4], ids=["rig", "transfer"])
def test_covariance_with_held_block_and_rank_deficiency(a):
  m, b, rho = ul.rig(), 3, 0.5
  p = m.stored_count(b, a)
  uv = ul.edge_pixels()[[0, 2, 5]]
  full = ul.random_spd(p, 3)
  held = full.copy()
  lo = 5 + m.n_dist[b]
  held[lo:lo + 6, :] = 0.0                     # the pose of b is held
  held[:, lo:lo + 6] = 0.0
  check_covariance(b, a, rho, held, uv, f"held pose, reference {a}")
  A = np.random.default_rng(5).normal(size=(p, 5)) * 1e-3
  check_covariance(b, a, rho, A @ A.T, uv, f"rank 5, reference {a}")


def test_covariance_that_cancels():
  """cx and the rotation about y of camera b anti-correlated along the direction that leaves the centre pixel where it is: C is
  more than 1e4 below |J|^2 |Sigma|, and still within the bound"""
  m, b, rho = ul.rig(), 1, 0.5
  p = m.stored_count(b, None)
  centre = ul.edge_pixels()[[0]]
  J, _ = ul.query_rows(m, b, None, rho, centre)
  icx, iry = 2, 5 + m.n_dist[b] + 1
  v = np.zeros(p)
  v[icx], v[iry] = 1.0, -J[0, 0, icx] / J[0, 0, iry]
  sigma = 1e-2 * np.outer(v, v) + 1e-6 * ul.random_spd(p, 9)
  check_covariance(b, None, rho, sigma, centre, "anti-correlated cx and rotation", min_cancellation=1e4)


MONTE_CARLO = [(1, None, 0.5), (5, 0, 0.5), (3, 2, 0.0)]   # rig reference; pinhole -> fisheye; transfer at infinity


@pytest.mark.parametrize("case", range(3), ids=["rig", "pinhole-to-fisheye", "transfer-at-infinity"])
def test_monte_carlo_meaning(case):
  """N = 40 000 parameter samples from N(theta, Sigma), Sigma scaled to a pixel std of about 0.1 px, pushed through the exact chain
  of the restatement (inverse through a, transform, project through b): the sample covariance whitened by the returned one is I
  within 5 sqrt(2 / (N - 1)).  A wrong sign of the implicit term doubles the contribution of camera a instead of cancelling it."""
  b, a, rho = MONTE_CARLO[case]
  m, N = ul.rig(), 40000
  p = m.stored_count(b, a)
  q = ul.edge_pixels()[[0]] + np.array([[31.0, -17.0]])
  chain = chain_of(b, a, rho)
  scales = chain.steps / chain.steps.max()
  sigma = ul.random_spd(p, 20 + case, 1.0) * np.outer(scales, scales)
  skew_at = [4] + ([p - (m.n_dist[a] + 1)] if a is not None else [])
  sigma[skew_at, :] = 0.0                           # (the skew enters neither projection and is not a parameter of the device)
  sigma[:, skew_at] = 0.0
  job = lambda s: uncertainty.Job(b, a, np.inf if rho == 0 else 1.0 / rho, s, pixels=q)
  cov0, _, st = ul.run(m, [job(sigma)])
  assert st[0] == uncertainty.OK
  sigma *= 0.01 / np.linalg.eigvalsh(blocks(cov0)[0]).max()
  cov, std, st = ul.run(m, [job(sigma)])
  Cm = blocks(cov)[0]
  assert abs(std[0] - 0.1) < 1e-6
  rng = np.random.default_rng(100 + case)
  F = uncertainty.factor(sigma)
  samples = chain.theta[None] + rng.normal(size=(N, F.shape[1])) @ F.T
  src = chain.source(q[0])
  uv = np.array([chain.predict(t, q[0], src)[0] for t in samples])
  sample_cov = np.cov(uv.T)
  L = np.linalg.cholesky(Cm)
  Li = np.linalg.inv(L)
  white = Li @ sample_cov @ Li.T
  dev = np.abs(white - np.eye(2)).max()
  print(f"monte carlo {MONTE_CARLO[case]}: whitened sample covariance - I = {dev:.4f}, bound {5 * np.sqrt(2 / (N - 1)):.4f}; mean shift "
        f"{np.abs(uv.mean(axis=0) - chain.predict(chain.theta, q[0], src)[0]).max():.2e} px")
  assert dev <= 5.0 * np.sqrt(2.0 / (N - 1))


# ---- edges ----------------------------------------------------------------------------------------------------------------
def test_same_camera_and_held_everything_are_exactly_zero():
  m, uv = ul.rig(), ul.edge_pixels()
  p = m.stored_count(2, 2)
  cov, std, st = ul.run(m, [uncertainty.Job(2, 2, 2.0, ul.random_spd(p, 1), pixels=uv)])
  assert (st == uncertainty.OK).all() and (cov == 0).all() and (std == 0).all()
  for a in (None, 3):
    p = m.stored_count(2, a)
    cov, std, st = ul.run(m, [uncertainty.Job(2, a, 2.0, np.zeros((p, p)), pixels=uv)])
    assert (st == uncertainty.OK).all() and (cov == 0).all() and (std == 0).all()


def test_outside_the_model_and_behind():
  m = ul.rig()
  far = np.array([[5000.0, 4000.0], [np.nan, 10.0], [99.5, 74.5]])      # (no fisheye camera has produced the first)
  for a in (None, 4):
    p = m.stored_count(5, a) if a is None else m.stored_count(4, 5)
    job = uncertainty.Job(5, None, 2.0, ul.random_spd(p, 2), pixels=far) if a is None else uncertainty.Job(4, 5, 2.0, ul.random_spd(p, 2), pixels=far)
    cov, std, st = ul.run(m, [job])
    assert list(st) == [uncertainty.NOT_CONVERGED, uncertainty.NOT_CONVERGED, uncertainty.OK]
    assert np.isnan(cov[:2]).all() and np.isnan(std[:2]).all() and np.isfinite(cov[2]).all()
  # a camera that looks the other way: the point camera 1 sees lies behind it
  back = uncertainty.RigModel(ul.source_cameras(), m.poses.copy())
  back.poses[0] = np.diag([-1.0, 1.0, -1.0, 1.0]) @ m.poses[0]
  back.rtvecs = ul.transform.from_matrix(back.poses).reshape(-1, 6)
  cov, std, st = ul.run(back, [uncertainty.Job(0, 1, 1.0, ul.random_spd(back.stored_count(0, 1), 3), pixels=far[2:])])
  assert list(st) == [uncertainty.BEHIND] and np.isnan(cov).all() and np.isnan(std).all()


def test_unconstrained_columns():
  """a non-zero column of J on an unobserved parameter: UNCONSTRAINED and NaN; a coefficient the camera does not have (a padded
  column), the skew and the ignored second focal length of fix_aspect have J = 0 exactly and stay harmless; so does a translation
  at infinity"""
  m, uv = ul.rig(), ul.edge_pixels()[:3]
  b = 1
  p = m.stored_count(b, None)
  sigma = ul.random_spd(p, 4)
  loose = np.zeros(p, dtype=bool)
  loose[2] = True                                   # cx of b
  cov, std, st = ul.run(m, [uncertainty.Job(b, None, 2.0, sigma, loose, pixels=uv)])
  assert (st == uncertainty.UNCONSTRAINED).all() and np.isnan(cov).all() and np.isnan(std).all()
  loose[:] = False
  loose[4] = True                                   # the skew
  cov, std, st = ul.run(m, [uncertainty.Job(b, None, 2.0, sigma, loose, pixels=uv)])
  assert (st == uncertainty.OK).all() and np.isfinite(cov).all()
  f = ul.FIX_ASPECT
  p = m.stored_count(f, None)
  loose = np.zeros(p, dtype=bool)
  loose[1] = True                                   # the second focal length of a fix_aspect camera
  cov, std, st = ul.run(m, [uncertainty.Job(f, None, 2.0, ul.random_spd(p, 5), loose, pixels=uv)])
  assert (st == uncertainty.OK).all() and np.isfinite(cov).all()
  loose[:] = False
  loose[-3:] = True                                 # the translation of the pose: no part at infinity
  cov, std, st = ul.run(m, [uncertainty.Job(f, None, np.inf, ul.random_spd(p, 5), loose, pixels=uv)])
  assert (st == uncertainty.OK).all()
  cov, std, st = ul.run(m, [uncertainty.Job(f, None, 2.0, ul.random_spd(p, 5), loose, pixels=uv)])
  assert (st == uncertainty.UNCONSTRAINED).all()
  # the raw call: a padded distortion column does not exist in W at all -- K is the cameras' own
  with pytest.raises(RuntimeError, match="K = "):
    from multical_amd import _lib
    import ctypes as C
    from multical_amd.undistort import CameraSetInputs
    inp = CameraSetInputs(m.cameras)
    job = _lib.UncertaintyJob()
    job.camera, job.reference, job.K, job.r = 1, -1, 24, 0
    ul._host.check(ul.lib().unh_projection_uncertainty(C.byref(inp.struct()), _lib.dp(m.poses), 1, C.byref(job), None, None, None))


def test_std_is_the_eigenvalue_formula_bit_for_bit():
  m = ul.rig()
  jobs = [uncertainty.Job(b, a, 1.5, ul.random_spd(m.stored_count(b, a), 6 + b), grid=uncertainty.grid_of(ul.uh.IMAGE_SIZE, (7, 5)))
          for b, a in ((0, None), (4, 3), (6, 7))]
  cov, std, st = ul.run(m, jobs)
  assert (st == uncertainty.OK).all()
  uu, uv, vv = cov[:, 0], cov[:, 1], cov[:, 2]
  hs, hd = 0.5 * (uu + vv), 0.5 * (uu - vv)
  again = np.sqrt(np.maximum(hs + np.sqrt(hd * hd + uv * uv), 0.0))
  assert again.tobytes() == std.tobytes()
  assert std.max() == again.max()


def test_grid_and_list_return_the_same_bytes():
  m = ul.rig()
  for b, a in ((2, None), (5, 6)):
    sigma = ul.random_spd(m.stored_count(b, a), 8)
    grid = uncertainty.Job(b, a, 3.0, sigma, grid=uncertainty.grid_of(ul.uh.IMAGE_SIZE, (17, 5)))
    as_list = uncertainty.Job(b, a, 3.0, sigma, pixels=grid.pixel_array())
    one, two = ul.run(m, [grid]), ul.run(m, [as_list])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(one, two))
    assert (one[2] == uncertainty.OK).all()


def test_refused_calls_name_the_argument():
  m = ul.rig()
  uv = ul.edge_pixels()[:1]
  with pytest.raises(RuntimeError, match="inv_distance"):
    ul.run(m, [uncertainty.Job(0, None, -2.0, ul.random_spd(m.stored_count(0, None), 1), pixels=uv)])
  job = uncertainty.Job(0, None, 2.0, ul.random_spd(m.stored_count(0, None), 1), pixels=uv)
  job.camera = 9
  with pytest.raises((RuntimeError, IndexError), match="camera 9|index"):
    ul.run(m, [job])
  assert ul.run(m, []) [0].shape == (0, 3)                            # nothing to do: no array is touched


def test_sanitized_program(tmp_path):
  """the edge cases above once more in a stand-alone program under AddressSanitizer + UBSan (CPU only, nothing loaded into Python)"""
  r = host_build.sanitized_program("uncertainty_host", "uncertainty_sanitize_main.cpp", tmp_path)
  assert r.returncode == 0 and "uncertainty sanitize run: ok" in r.stdout, r.stdout + r.stderr
