"""mcba_view_information, host side (no GPU): the g++ build of csrc/mcba_guidance.h (guidance_host_lib) against the numpy restatement
(guidance_reference: own projection, Richardson differences, QR instead of the Schur step), the exactness of the update against the
dense Gauss-Newton covariance of a problem extended by the candidate frame (oracle.restate), the properties of the scores, the
statuses, and a stand-alone sanitizer program.  Measured worst cases: profiles/guidance_parity.txt."""
import numpy as np
import pytest

import host_build
from multical_amd import guidance, synthetic, uncertainty

import guidance_host_lib as gl
import guidance_reference as gr
import uncertainty_host_lib as ul
import uncertainty_reference as ur
import undistort_reference as ref

N_CAMERAS = 9
FOCUS_GRID = (5, 4, 20.0, 15.0, 40.0, 40.0)


def focus_pixels(grid=FOCUS_GRID):
  gw, gh, u0, v0, du, dv = grid
  return np.stack(np.broadcast_arrays((u0 + np.arange(gw) * du)[None, :], (v0 + np.arange(gh) * dv)[:, None]), axis=-1).reshape(-1, 2)


def theta_of(c):
  cam = ul.source_cameras()[c]
  return gr.stored_block(cam, gl.fix_aspect(c)), ref.is_fisheye(cam), gl.fix_aspect(c)


def factors_with(c, F):
  fac = gl.empty_factors()
  fac[c] = gl.device_factor(c, F)
  return fac


@pytest.mark.parametrize("c", range(N_CAMERAS))
def test_restated_projection_is_the_projection(c):
  """the restatement's own forward function against undistort_reference.project (the restated cv2 projections)"""
  theta, fish, fa = theta_of(c)
  rng = np.random.default_rng(c)
  X = np.concatenate([rng.uniform(-0.3, 0.3, (40, 2)), rng.uniform(0.8, 1.5, (40, 1))], axis=1)
  want = ref.project(ur.camera_of(theta, fish, fa), X)
  assert np.abs(gr.project(theta, fish, fa, X) - want).max() <= 1e-10


# ---- 1. S against the restatement --------------------------------------------------------------------------------------------
def stored_factors(c):
  """full rank (every parameter the device has a column for), rank 5, all but one held"""
  p = 5 + gl.n_dist(c)
  full = p - 1 - (1 if gl.fix_aspect(c) else 0)
  held = [i for i in range(p) if i != 2]
  out = dict(full=gl.stored_factor(c, full, 100 + c, held=[1] if gl.fix_aspect(c) else []), rank5=gl.stored_factor(c, 5, 200 + c),
             one=gl.stored_factor(c, 1, 300 + c, held=held))
  return out


@pytest.mark.parametrize("c", range(N_CAMERAS))
def test_schur_complement_against_the_restatement(c):
  theta, fish, fa = theta_of(c)
  pts, T = gl.board(25), gl.pose(40 + c)
  px = focus_pixels()
  worst = 0.0
  for name, F in stored_factors(c).items():
    views, want = [], []
    for nn in (0, 3, 6):
      views.append(guidance.View(c, 0, T, nn, 1))
      want.append(gr.board_view(theta, fish, fa, pts, T, nn, F, (gl.W_IMG, gl.H_IMG)))
    for rho in (0.0, 0.5, 2.0):
      for nn in (0, 3) if rho == 0.0 else (0, 3, 6):
        views.append(guidance.Focus(c, np.inf if rho == 0.0 else 1.0 / rho, grid=FOCUS_GRID, n_nuisance=nn, min_points=1))
        want.append(gr.focus_view(theta, fish, fa, px, rho, nn, F))
    got = gl.run(factors_with(c, F), [pts], views, n=0)
    r = F.shape[1]
    for v, (S_qr, S_ne, ok, scale) in enumerate(want):
      assert got.status[v] == guidance.OK and got.n_visible[v] == ok.sum() and ok.sum() >= 12, (name, v)
      spread = np.abs(S_qr - S_ne).max() / scale
      err = np.abs(got.S[v, :r, :r] - S_qr).max() / scale
      tol = max(1e-9, 100.0 * spread)
      worst = max(worst, err / tol)
      assert err <= tol, (name, v, err, spread)
      assert (got.S[v, r:] == 0).all() and (got.S[v, :, r:] == 0).all()
  print(f"camera {c}: worst |S - S_restated| / |KW|^2 = {worst:.3g} of its tolerance")


# ---- 2. exactness end to end -------------------------------------------------------------------------------------------------
TWO_BOARDS = dict(cameras=2, frames=6, boards=["charuco_10x10", "aprilgrid_9x9"], motion="static", model="standard",
                  optimize_cameras=True, layout="stereo", seed=21)
_problems = {}


def dense_problem(name):
  """(oracle calibration with the cameras enabled, x, block offsets) of a static rig"""
  if name not in _problems:
    from oracle import restate
    rig = synthetic.make_rig("tiny" if name == "tiny" else TWO_BOARDS)
    oc = restate.from_rig(rig, "truth").enable(cameras=True)
    _problems[name] = oc
  return _problems[name]


def layout(oc):
  """offsets of the blocks of param_vec: camera_poses, board_poses, motion, cameras (list per camera)"""
  C, F, B, _ = oc.point_valid.shape
  cams, at = [], 6 * C + 6 * B + 6 * F
  for cam in oc.cameras:
    n = cam.param_vec.size
    cams.append(np.arange(at, at + n))
    at += n
  return dict(camera_poses=0, board_poses=6 * C, motion=6 * C + 6 * B, cameras=cams, n=at)


def extended(oc, c, b, T, mask):
  """the problem with one more frame in which only camera c sees board b at the board-in-camera pose T, the points in `mask`"""
  from types import SimpleNamespace
  C, F, B, P = oc.point_valid.shape
  R = np.linalg.inv(oc.camera_poses[c]) @ T @ np.linalg.inv(oc.board_poses[b])
  motion = SimpleNamespace(kind="static", valid=np.concatenate([oc.motion.valid, [True]]), poses=np.concatenate([oc.motion.poses, R[None]]))
  valid = np.concatenate([oc.point_valid, np.zeros((C, 1, B, P), dtype=bool)], axis=1)
  valid[c, F, b, :len(mask)] = mask
  ext = oc.copy(points=np.concatenate([oc.points, np.zeros((C, 1, B, P, 2))], axis=1), valid=valid, motion=motion)
  proj, _ = ext.reprojected()
  ext.points[:, F] = proj[:, F]                                   # the noise-free projections
  return ext


def dense_jacobian(oc):
  x = oc.param_vec
  lay = layout(oc)
  steps = np.full(x.size, 2e-3)
  for idx in lay["cameras"]:
    steps[idx[:5]] = 0.5
  return gr.richardson(oc.evaluate, x, steps)


def covariance_routes(J, free, sigma2):
  """sigma2 (J_free^T J_free)^-1 by numpy's inverse and by a QR of J_free, scattered to all parameters"""
  free = free[np.abs(J[:, free]).max(axis=0) > 0]                  # (a parameter that no residual depends on has no covariance)
  Jf = J[:, free]
  out = []
  R = np.linalg.qr(Jf, mode="r")
  Ri = np.linalg.inv(R)
  for cov in (np.linalg.inv(Jf.T @ Jf), Ri @ Ri.T):
    full = np.zeros((J.shape[1], J.shape[1]))
    full[np.ix_(free, free)] = sigma2 * cov
    out.append(full)
  return out


@pytest.mark.parametrize("name,c,b", [("tiny", 0, 0), ("tiny", 1, 0), ("two_boards", 0, 1), ("two_boards", 1, 1)],
                         ids=["tiny-held", "tiny-free", "two-boards-held", "two-boards-free"])
def test_update_is_exact_against_the_extended_problem(name, c, b):
  sigma2 = 0.04
  oc = dense_problem(name)
  C, F, B, P = oc.point_valid.shape
  lay = layout(oc)
  cam, pts = oc.cameras[c], np.asarray(oc.board_points[b], dtype=np.float64)
  theta, fish, fa = cam.param_vec, cam.model == "fisheye", cam.fix_aspect
  poses = guidance.candidate_poses(cam, pts)
  counts = np.array([gr.visible(theta, fish, fa, pts @ T[:3, :3].T + T[:3, 3], cam.image_size).sum() for T in poses])
  tilted = np.array([abs(T[2, 2]) < 0.99 for T in poses])
  picks = [int(np.flatnonzero((counts == len(pts)) & tilted)[0]), int(np.flatnonzero((counts > 0.3 * len(pts)) & (counts < 0.7 * len(pts)))[0])]
  # the original problem: hold the gauge (first camera pose, first board pose) and the skews
  def free_of(layout_, n_frames):
    hold = np.zeros(layout_["n"], dtype=bool)
    hold[0:6] = True
    hold[layout_["board_poses"]:layout_["board_poses"] + 6] = True
    for idx in layout_["cameras"]:
      hold[idx[4]] = True
    return np.flatnonzero(~hold)
  worst = 0.0
  for v in picks:
    T = poses[v]
    mask = gr.visible(theta, fish, fa, pts @ T[:3, :3].T + T[:3, 3], cam.image_size)
    ext = extended(oc, c, b, T, mask)
    lay_x = layout(ext)
    Jx = dense_jacobian(ext)
    frame_of = np.broadcast_to(np.arange(F + 1)[None, :, None, None], ext.inliers.shape)[ext.inliers]
    old_rows = np.flatnonzero(np.repeat(frame_of < F, 2))
    assert Jx.shape[0] - old_rows.size == 2 * int(mask.sum())
    old_cols = np.concatenate([np.arange(lay["motion"] + 6 * F), np.arange(lay_x["motion"] + 6 * (F + 1), lay_x["n"])])
    J0 = Jx[np.ix_(old_rows, old_cols)]
    assert np.abs(Jx[old_rows][:, lay_x["motion"] + 6 * F:lay_x["motion"] + 6 * F + 6]).max() == 0.0
    sig0 = covariance_routes(J0, free_of(lay, F), sigma2)[0]
    sig_inv, sig_qr = covariance_routes(Jx, free_of(lay_x, F + 1), sigma2)
    block0, block_x = sig0[np.ix_(lay["cameras"][c], lay["cameras"][c])], lay_x["cameras"][c]
    Fc = uncertainty.factor(block0)
    cams = [type("Cam", (), dict(intrinsic=k.intrinsic, dist=k.dist, image_size=k.image_size, fix_aspect=k.fix_aspect,
                                 model=k.model))() for k in oc.cameras]
    model = uncertainty.RigModel(cams, np.tile(np.eye(4), (C, 1, 1)), np.zeros((C, 6)))
    factors = [(np.zeros((4 + model.n_dist[k], 0)), False) for k in range(C)]
    factors[c] = (uncertainty.camera_map(model.n_dist[c], fa) @ Fc, False)
    with gl.host_backend():
      got = guidance.view_information(model.cameras, factors, [np.asarray(p, dtype=np.float64) for p in oc.board_points],
                                      [guidance.View(c, b, T, 6, 4)], n=1, criterion="gain", sigma2=sigma2)
    assert got.status[0] == guidance.OK and got.n_visible[0] == mask.sum()
    r = Fc.shape[1]
    post = Fc @ np.linalg.inv(np.eye(r) + got.S[0, :r, :r] / sigma2) @ Fc.T
    assert np.abs(post - Fc @ got.posterior[c, :r, :r] @ Fc.T).max() <= 1e-9 * np.abs(post).max()    # (the device's own posterior)
    want = sig_inv[np.ix_(block_x, block_x)]
    std = np.sqrt(np.diag(want))
    live = std > 0
    scale = np.outer(std, std)[np.ix_(live, live)]
    err = (np.abs(post - want)[np.ix_(live, live)] / scale).max()
    spread = (np.abs(sig_qr[np.ix_(block_x, block_x)] - want)[np.ix_(live, live)] / scale).max()
    shrink = (np.abs(block0 - want)[np.ix_(live, live)] / scale).max()
    tol = max(1e-9, 100.0 * spread)
    worst = max(worst, err / tol)
    print(f"{name} camera {c} board {b} view {v}: {int(mask.sum())} of {len(pts)} visible, |posterior - dense| = {err:.3g} "
          f"(correlation-normalised), spread of the dense routes {spread:.3g}, the update itself {shrink:.3g}")
    assert shrink > 1e-3                    # (the view does change the covariance: the comparison is not vacuous)
    assert err <= tol, (err, spread)


# ---- 3. properties -----------------------------------------------------------------------------------------------------------
def candidate_set(c, n=12, P=36):
  return [guidance.View(c, 0, gl.pose(500 + 7 * c + i, tilt=0.5, shift=0.08), 6, 4) for i in range(n)], gl.board(P)


def default_focus(c, distance=np.inf):
  return [guidance.Focus(k, distance, grid=uncertainty.grid_of((gl.W_IMG, gl.H_IMG), (8, 6))) if k == c else None for k in range(N_CAMERAS)]


@pytest.mark.parametrize("c", [0, 4, 5, 8])
def test_scores_do_not_depend_on_the_factor(c):
  F = stored_factors(c)["full"]
  r = F.shape[1]
  O = np.linalg.qr(np.random.default_rng(c).normal(size=(r, r)))[0]
  views, pts = candidate_set(c)
  a = gl.run(factors_with(c, F), [pts], views, default_focus(c), n=2)
  b = gl.run(factors_with(c, F @ O), [pts], views, default_focus(c), n=2)
  assert np.array_equal(a.status, b.status) and (a.status == guidance.OK).all()
  assert np.allclose(a.gain, b.gain, rtol=1e-9, atol=1e-12) and np.allclose(a.focus_rms, b.focus_rms, rtol=1e-9)
  assert np.allclose(a.focus_before, b.focus_before, rtol=1e-9, equal_nan=True) and np.array_equal(a.picks, b.picks)
  assert np.allclose(a.pick_focus_rms[c], b.pick_focus_rms[c], rtol=1e-9)


@pytest.mark.parametrize("criterion", ["focus", "gain"])
@pytest.mark.parametrize("c", [1, 2, 6])
def test_greedy_selection_and_its_inequalities(c, criterion):
  sigma2 = 0.25
  F = stored_factors(c)["full"]
  r = F.shape[1]
  views, pts = candidate_set(c)
  got = gl.run(factors_with(c, F), [pts], views, default_focus(c, 1.5), n=3, criterion=criterion, sigma2=sigma2, with_rounds=True)
  S, Q, G = got.S[:, :r, :r], got.Q[c, :r, :r], int(got.focus_n_visible[c])
  assert got.focus_status[c] == guidance.OK and G == 48
  # the scores against the base I
  for v in range(len(views)):
    assert np.isclose(got.gain[v], gr.gain(np.eye(r), S[v] / sigma2), rtol=1e-9)
    assert np.isclose(got.focus_rms[v], gr.focus_rms(np.eye(r), S[v] / sigma2, Q, G), rtol=1e-8)
  assert np.isclose(got.focus_before[c], np.sqrt(np.trace(Q) / G), rtol=1e-12)
  # greedy picks equal a numpy greedy over the returned S
  want = gr.greedy(S, got.status, Q, G, sigma2, 3, criterion)
  assert [w[0] for w in want] == list(got.picks[c])
  assert np.allclose([w[1] for w in want], got.pick_gain[c], rtol=1e-9) and np.allclose([w[2] for w in want], got.pick_focus_rms[c], rtol=1e-8)
  # focus_rms_after <= focus_rms_before, pick after pick
  chain = np.concatenate([[got.focus_before[c]], got.pick_focus_rms[c]])
  assert (np.diff(chain) <= 0).all() and (got.focus_rms <= got.focus_before[c]).all()
  # the chain rule
  v1, v2, v3 = got.picks[c]
  assert np.isclose(got.pick_gain[c, 0] + got.pick_gain[c, 1], 0.5 * np.linalg.slogdet(np.eye(r) + (S[v1] + S[v2]) / sigma2)[1], rtol=1e-10)
  assert np.isclose(got.pick_gain[c].sum(), 0.5 * np.linalg.slogdet(np.eye(r) + (S[v1] + S[v2] + S[v3]) / sigma2)[1], rtol=1e-10)
  # information is submodular: gain(v | base) <= gain(v | I)
  assert np.array_equal(got.round_gain[0], got.gain)
  for k in (1, 2):
    assert (got.round_gain[k] <= got.round_gain[k - 1] * (1 + 1e-12)).all()
  # the posterior
  B = np.eye(r) + (S[v1] + S[v2] + S[v3]) / sigma2
  assert np.allclose(got.posterior[c, :r, :r] @ B, np.eye(r), atol=1e-9)


@pytest.mark.parametrize("c", [0, 3, 5, 8])
def test_plain_focus_is_the_intrinsics_only_uncertainty_map(c):
  """n_nuisance = 0 at rho = 0: trace Q_c is the summed trace of mcba_projection_uncertainty's map of a camera whose pose is held"""
  F = stored_factors(c)["full"]
  p = F.shape[0]
  grid = uncertainty.grid_of((gl.W_IMG, gl.H_IMG), (8, 6))
  foci = [guidance.Focus(k, np.inf, grid=grid, n_nuisance=0) if k == c else None for k in range(N_CAMERAS)]
  views, pts = candidate_set(c, 1)
  got = gl.run(factors_with(c, F), [pts], views, foci, n=0)
  sigma = np.zeros((p + 6, p + 6))
  sigma[:p, :p] = F @ F.T
  cov, _, status = ul.run(ul.rig(), [uncertainty.Job(c, None, np.inf, sigma, grid=grid)])
  assert (status == uncertainty.OK).all() and got.focus_n_visible[c] == 48
  assert np.isclose(got.focus_before[c] ** 2 * 48, (cov[:, 0] + cov[:, 2]).sum(), rtol=1e-10)
  assert np.isclose(np.trace(got.Q[c]), (cov[:, 0] + cov[:, 2]).sum(), rtol=1e-10)


# ---- 4. statuses -------------------------------------------------------------------------------------------------------------
def test_statuses():
  c = 0
  F = stored_factors(c)["rank5"]
  pts = gl.board(16)
  far = gl.pose(1)
  far[:3, 3] = [5.0, 0.0, 0.5]                                        # every corner outside the image
  behind = gl.pose(2)
  behind[2, 3] = -0.5
  line = np.stack([np.linspace(-0.05, 0.05, 16), np.zeros(16), np.zeros(16)], axis=1)
  views = [guidance.View(c, 0, gl.pose(3), 6, 16), guidance.View(c, 0, gl.pose(3), 6, 17), guidance.View(c, 0, far, 6, 1),
           guidance.View(c, 0, behind, 6, 1), guidance.View(c, 1, gl.pose(3), 6, 4), guidance.View(c, 1, gl.pose(3), 3, 4),
           guidance.View(1, 0, gl.pose(3), 6, 4), guidance.View(2, 0, gl.pose(3), 6, 4)]
  fac = factors_with(c, F)
  fac[1] = (gl.device_factor(1, gl.stored_factor(1, 3, 9))[0], True)   # a loose intrinsic
  foci = [guidance.Focus(k, np.inf, grid=FOCUS_GRID) for k in range(N_CAMERAS)]
  got = gl.run(fac, [pts, line], views, foci, n=2, criterion="gain")
  OK, FEW, DEG, UNC = guidance.OK, guidance.TOO_FEW, guidance.DEGENERATE, guidance.UNCONSTRAINED
  assert list(got.status) == [OK, FEW, FEW, FEW, DEG, OK, UNC, OK]
  assert list(got.n_visible[:6]) == [16, 16, 0, 0, 16, 16]
  bad = got.status != OK
  assert np.isnan(got.gain[bad]).all() and np.isnan(got.focus_rms[bad]).all() and (got.S[bad] == 0).all()
  assert got.gain[7] == 0.0 and got.focus_rms[7] == 0.0               # camera 2: r = 0, nothing to learn
  assert sorted(got.picks[c]) == [0, 5] and (got.picks[1:] == -1).all() and np.isnan(got.pick_gain[1:]).all()
  assert got.focus_status[1] == UNC and got.focus_status[0] == OK and np.isnan(got.focus_before[1]) and got.focus_before[2] == 0.0
  # a view that is not OK is never chosen, however many picks are asked for
  more = gl.run(fac, [pts, line], views, foci, n=4, criterion="focus")
  assert sorted(more.picks[c][:2]) == [0, 5] and list(more.picks[c][2:]) == [-1, -1] and np.isnan(more.pick_gain[c, 2:]).all()


def test_empty_and_refused_calls():
  c = 0
  fac = factors_with(c, stored_factors(c)["rank5"])
  pts = gl.board(9)
  got = gl.run(fac, [pts], [], None, n=2)                               # zero views
  assert got.gain.shape == (0,) and (got.picks == -1).all() and np.isnan(got.pick_gain).all()
  got = gl.run(gl.empty_factors(), [pts], [guidance.View(3, 0, gl.pose(1))], None, n=1)      # r = 0 everywhere
  assert got.status[0] == guidance.OK and got.gain[0] == 0.0 and (got.picks == -1).all()
  for bad, match in ((guidance.View(9, 0, gl.pose(1)), "camera 9"), (guidance.View(0, 1, gl.pose(1)), "board 1"),
                     (guidance.View(0, 0, gl.pose(1), 4), "n_nuisance"), (guidance.View(0, 0, np.full((4, 4), np.nan)), "not finite"),
                     (guidance.Focus(0, np.inf, grid=FOCUS_GRID, n_nuisance=6), "inv_distance")):
    with pytest.raises((RuntimeError, ValueError), match=match):
      gl.run(fac, [pts], [bad], None)
  with pytest.raises((RuntimeError, ValueError), match="sigma2"):
    gl.run(fac, [pts], [guidance.View(0, 0, gl.pose(1))], None, sigma2=0.0)


def test_candidate_poses_face_the_camera():
  cam, pts = gl.cameras()[0], gl.board(81)
  T = guidance.candidate_poses(cam, pts)
  assert T.shape == (7 * 5 * 2 * 5, 4, 4)
  centre = (T[:, :3, :3] @ (0.5 * (pts.min(axis=0) + pts.max(axis=0)))) + T[:, :3, 3]
  assert (centre[:, 2] > 0).all() and np.allclose(np.linalg.det(T[:, :3, :3]), 1.0)
  uv = gr.project(*theta_of(0), centre)
  assert (uv >= -1e-6).all() and (uv[:, 0] <= gl.W_IMG).all() and (uv[:, 1] <= gl.H_IMG).all()


# ---- 5. sanitizer ------------------------------------------------------------------------------------------------------------
def test_sanitized_program(tmp_path):
  """the edge cases once more in a stand-alone program under AddressSanitizer + UBSan (CPU only, nothing loaded into Python)"""
  r = host_build.sanitized_program("guidance", "guidance_sanitize_main.cpp", tmp_path)
  assert r.returncode == 0 and "guidance sanitize run: ok" in r.stdout, r.stdout + r.stderr
