"""mcba_hand_eye / k_hand_eye on the MI355X: against the host build of the same header (tests/handeye_host) at the pair counts where
staging, the MFMA tail and chunking can go wrong, repeatability, empty launches, the scatter of statuses, HandEyeCalibration.initialise
on the hand-eye rigs, and detections -> Workspace.initialise_poses(is_non_overlapping=True) -> bundle adjustment end to end.

Tolerance of device against host: max(1e-10, 100 x the host build's own difference between its two summation orders) per problem --
pairs added in frame order against reversed frame order.  The device adds them in a third order (four pairs per MFMA step in frame
order for K; 64 lane partials folded by the xor butterfly for the other sums) and contracts to FMAs; the rule and the reason are
those of tests/test_gpu_pose_table.py.  Measured figures: profiles/hand_eye_parity.txt."""
import ctypes as C

import numpy as np
import pytest

import handeye_host_lib as hh
import pnp_host_lib as L
from multical_amd import _lib, calibration, hand_eye, synthetic, tables
from multical_amd.workspace import Workspace

pytestmark = pytest.mark.gpu

OK, TOO_FEW, DEGENERATE = tables.HANDEYE_OK, tables.HANDEYE_TOO_FEW, tables.HANDEYE_DEGENERATE


def _diff(a, b):
  return np.abs(np.asarray(a) - np.asarray(b)).reshape(len(a), -1).max(axis=1)


def _compare(args, invert, tag):
  """device against host on one problem list; returns the device result"""
  dev = tables.hand_eye_batch(*args, invert=invert)
  host = hh.hand_eye_batch(*args, invert=invert)
  rev = hh.hand_eye_batch(*args, invert=invert, reversed_order=True)
  assert np.array_equal(host[3], rev[3])
  assert np.array_equal(dev[3], host[3]), (tag, dev[3], host[3])
  assert np.array_equal(dev[2], host[2]), tag
  worst = 0.0
  for i, name in ((0, "X"), (1, "Z"), (4, "err")):
    tol = np.maximum(1e-10, 100.0 * _diff(host[i], rev[i]))
    d = _diff(dev[i], host[i])
    worst = max(worst, float((d / tol).max()))
    assert np.all(d <= tol), (tag, name, float(d.max()), float(tol[np.argmax(d / tol)]))
  print(f"{tag}: {len(dev[0])} problems, |dX| {_diff(dev[0], host[0]).max():.1e}, |dZ| {_diff(dev[1], host[1]).max():.1e}, "
        f"|d err| {_diff(dev[4], host[4]).max():.1e}, host order spread {max(_diff(host[0], rev[0]).max(), _diff(host[1], rev[1]).max()):.1e}, "
        f"worst / tolerance {worst:.2g}")
  return dev


# usable pairs: 3 = the minimum, 4 / 5 = one MFMA step and its tail, 63 / 64 / 65 = a staging chunk, 130 = three chunks; frames: pairs
# interleaved with invalid frames (2 n + 7), and for the small counts also 200 frames, where whole chunks hold no usable pair
@pytest.mark.parametrize("n_pairs,F", [(3, None), (3, 200), (4, None), (5, None), (5, 200), (63, None), (64, None), (65, None),
                                       (130, None)])
@pytest.mark.parametrize("n_problems", [1, 70])
def test_device_matches_host_build(n_pairs, F, n_problems):
  ta, va, tb, vb, Xs, Zs = hh.interleaved_problem(1000 * n_pairs + n_problems, n_pairs, F=F, n_rows=n_problems)
  idx = np.arange(n_problems)
  both = np.concatenate([ta, tb]), np.concatenate([va, vb])            # one table that holds both sides
  for invert in (False, True):
    a = (hh.ref_inverse(ta), va, hh.ref_inverse(tb), vb) if invert else (ta, va, tb, vb)
    dev = _compare(a + (idx, idx), invert, f"n={n_pairs} F={ta.shape[1]} x{n_problems} two tables invert={int(invert)}")
    assert np.all(dev[3] == OK) and np.all(dev[2] == n_pairs)
    assert np.abs(dev[0] - Xs).max() <= 1e-9 and np.abs(dev[1] - Zs).max() <= 1e-9       # (exact data)
    t, v = (hh.ref_inverse(both[0]), both[1]) if invert else both
    one = _compare((t, v, t, v, idx, idx + n_problems), invert, f"n={n_pairs} F={ta.shape[1]} x{n_problems} one table invert={int(invert)}")
    for u, w in zip(one, dev):
      assert u.tobytes() == w.tobytes()                                   # the same problems through the single upload


def test_device_matches_host_build_on_the_noisy_chain_of_cfg5_40():
  poses, valid, _, (C_, F, B) = hh.camera_board_chain("cfg5_40", noise_seed=7)
  ia, ib, _ = hh.camera_pair_problems(valid, C_, B)
  dev = _compare((poses, valid, poses, valid, ia, ib), True, f"cfg5_40 noisy chain")
  assert len(ia) == 216 and np.all(dev[3] == OK)
  again = tables.hand_eye_batch(poses, valid, poses, valid, ia, ib, invert=True)
  for a, b in zip(dev, again):
    assert a.tobytes() == b.tobytes()                                     # two calls return the same bits


def _timing():
  ms, n = _lib.call_ms("hand_eye", range(4))
  return list(ms.values()), n


def test_empty_launches():
  ta, va, tb, vb, _, _ = hh.interleaved_problem(5, 6, n_rows=2)
  X, Z, n, st, err = tables.hand_eye_batch(ta, va, tb, vb, [], [])
  assert X.shape == (0, 4, 4) and err.shape == (0, ta.shape[1]) and _timing()[1] == 0
  none = np.zeros_like(va)
  X, Z, n, st, err = tables.hand_eye_batch(ta, none, tb, vb, [0, 1], [0, 1])
  ms, launched = _timing()
  assert launched == 0 and ms[1] == 0.0 and ms[2] == 0.0                  # no upload, no kernel
  assert np.array_equal(X, np.broadcast_to(np.eye(4), X.shape)) and np.array_equal(Z, X)
  assert (n == 0).all() and (st == TOO_FEW).all() and not err.any()
  # ... and a regular call afterwards
  assert (tables.hand_eye_batch(ta, va, tb, vb, [0, 1], [0, 1])[3] == OK).all() and _timing()[1] == 2


def test_problems_without_a_result_sit_between_solved_ones():
  ta, va, tb, vb, Xs, Zs = hh.interleaved_problem(9, 10, n_rows=6)
  use = np.flatnonzero(va[1] & vb[1])
  va[1, use[2:]] = False                                                  # row 1: two usable pairs
  tb[3, :, :3, :3] = tb[3, 0, :3, :3]
  ta[3, :, :3, :3] = ta[3, 0, :3, :3]                                      # row 3: pure translations
  va[4] = False                                                           # row 4: nothing
  idx = np.arange(6)
  dev = _compare((ta, va, tb, vb, idx, idx), False, "mixed statuses")
  assert list(dev[3]) == [OK, TOO_FEW, OK, DEGENERATE, TOO_FEW, OK] and list(dev[2]) == [10, 2, 10, 10, 0, 10]
  for k in (1, 3, 4):
    assert np.array_equal(dev[0][k], np.eye(4)) and np.array_equal(dev[1][k], np.eye(4)) and not dev[4][k].any()
  for k in (0, 2, 5):
    assert np.abs(dev[0][k] - Xs[k]).max() <= 1e-9 and np.abs(dev[1][k] - Zs[k]).max() <= 1e-9
  # outputs that are not asked for
  s = tables.HandEyeInputs(ta, va, tb, vb, idx, idx).struct()
  X = np.empty((6, 4, 4))
  _lib.check(_lib.load().mcba_hand_eye(C.byref(s), X.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, None))
  assert X.tobytes() == dev[0].tobytes()
  with pytest.raises(_lib.McbaError, match="outside"):
    tables.hand_eye_batch(ta, va, tb, vb, [6], [0])


@pytest.mark.parametrize("name", ["tiny_handeye", "cfg5_handeye"])
def test_hand_eye_calibration_initialise(name):
  """the truth's frame poses and the robot's poses give back the truth's world_wrt_base / gripper_wrt_camera (1e-9: exact data, up
  to 400 pairs; the margin covers the ring rig's near-common axis), and the bundle adjustment from there does not end above its start"""
  rig = synthetic.make_rig(name)
  truth = calibration.from_rig(rig, 'truth')
  he = rig.truth.hand_eye
  hec = hand_eye.HandEyeCalibration.initialise(truth, np.linalg.inv(he.base_wrt_gripper))
  assert isinstance(hec.calib.motion, hand_eye.HandEyeMotion)
  assert hec.calib.optimize.camera_poses is False and hec.calib.optimize.cameras is False
  dw = np.abs(hec.model.world_wrt_base - he.world_wrt_base).max()
  dg = np.abs(hec.gripper_wrt_camera - he.gripper_wrt_camera).max()
  print(f"{name}: |world_wrt_base - truth| {dw:.1e}, |gripper_wrt_camera - truth| {dg:.1e}")
  assert dw <= 1e-9 and dg <= 1e-9
  assert np.abs(hec.base_wrt_world @ he.world_wrt_base - np.eye(4)).max() <= 1e-9
  assert np.array_equal(hec.valid, rig.frame_valid)
  cost = lambda c: float(np.sum(np.square(c.reprojection_error)))
  out = hec.bundle_adjust()
  assert isinstance(out, hand_eye.HandEyeCalibration) and out.gripper_wrt_base is hec.gripper_wrt_base
  print(f"{name}: cost {cost(hec.calib):.6f} -> {cost(out.calib):.6f} px^2")
  assert cost(out.calib) <= cost(hec.calib)
  assert set(out.cameras_wrt_gripper) == set(truth.cameras.names)


def test_detections_to_bundle_adjustment_of_a_non_overlapping_rig():
  """detections -> Workspace.initialise_poses(is_non_overlapping=True) -> bundle_adjust on cfg5_40: the camera-pose start is the
  one HandEye computes over the host build on the same pose table (same picks; candidates within the device-against-host
  tolerance), and the optimum is the one the fixture's own initial guess reaches, within 1e-6 px.
  exclude_bad_poses=False: the default rejection at 1 px keeps 137 of the fixture's 261 views (its detections carry gross outlier
  corners), which leaves cameras (cam0, cam1) without a single board pair of 3 common frames -- no hand-eye start exists there, in
  the reference either; all 259 converged views are kept, as tests/test_gpu_pose_table.py does for cfg1."""
  rig = L.golden_rig("cfg5_40")
  own = calibration.from_rig(rig)
  truth = calibration.from_rig(rig, 'truth')
  tight = dict(tolerance=1e-15, xtol=1e-15, gtol=1e-15, max_iterations=300, solver="native")
  want = own.bundle_adjust(**tight)
  ws = Workspace()
  # the default call: the rejection leaves cameras (cam0, cam1) without a candidate, and the error says so
  with pytest.raises(ValueError, match=r"no hand-eye candidate for cameras \(cam0, cam1\)"):
    ws.initialise_poses(own.point_table, list(own.boards), list(truth.cameras), is_non_overlapping=True)
  assert int(ws.pose_table.valid.sum()) < int((rig.valid.sum(axis=3) >= 4).sum())                 # (the rejection ran)
  init = ws.initialise_poses(own.point_table, list(own.boards), list(truth.cameras), exclude_bad_poses=False, is_non_overlapping=True)
  names = list(init.camera_poses.names)
  # the same start over the host build
  host = hand_eye.HandEye(ws.pose_table, names, solver=hh.hand_eye_batch)
  host_init = host.initialise_camera_poses()
  rev = hand_eye.HandEye(ws.pose_table, names, solver=lambda *a, **k: hh.hand_eye_batch(*a, reversed_order=True, **k))
  rev.initialise_camera_poses()
  dev = ws.hand_eye
  assert dev.picks == host.picks and dev.reference_camera == host.reference_camera
  assert len(dev.handeye_df) == len(host.handeye_df) == len(rev.handeye_df) > 0
  key = "slaveCam_wrt_masterCam"
  Xd, Xh, Xr = (np.array([d[key] for d in h.handeye_df]) for h in (dev, host, rev))
  tol = np.maximum(1e-10, 100.0 * _diff(Xh, Xr))
  assert np.all(_diff(Xd, Xh) <= tol), float((_diff(Xd, Xh) / tol).max())
  cam_d = np.array([dev.cam_init[k] for k in names])
  cam_h = np.array([host_init[k] for k in names])
  print(f"cfg5_40: |cam_init - host| {np.abs(cam_d - cam_h).max():.1e} (tolerance {tol.max():.1e})")
  assert np.abs(cam_d - cam_h).max() <= tol.max()
  assert np.array_equal(init.camera_poses.poses, cam_d) and np.abs(cam_d[0] - np.eye(4)).max() <= 1e-12
  got = init.enable(**rig.optimize).bundle_adjust(**tight)
  rms = lambda c: float(np.sqrt(np.mean(np.square(c.reprojection_error))))
  print(f"cfg5_40: {len(dev.handeye_df)} hand-eye candidates, reference camera {dev.reference_camera}, |candidates - host| "
        f"{_diff(Xd, Xh).max():.1e}, rms from the hand-eye start {rms(got):.12f} px, from the fixture's x0 {rms(want):.12f} px "
        f"(difference {rms(got) - rms(want):+.2e}), at the initialisation {rms(init):.3f} px")
  assert abs(rms(got) - rms(want)) <= 1e-6
