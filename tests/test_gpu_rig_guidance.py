"""mcba_rig_view_information on the device (k_rig_gram, k_focus_gram, k_rig_assemble, k_rig_score, k_rig_base_add) against the g++ build
of the same header (rigview_host_lib), and Calibration.suggest_rig_views end to end.  Statuses, counts and picks are equal; A, Q and
the posterior (relative to the matrix's largest entry), gain (relative to 1 + gain) and focus_rms (relative) agree within 100 x what
contraction alone does -- the difference between two HOST builds of the header, -ffp-contract=off against -ffp-contract=fast, over the
same call (measured here on the CPU, printed; profiles/rig_guidance_parity.txt).  The inputs are ones on which the two host builds
pick the same views (asserted)."""
import numpy as np
import pytest

from multical_amd import guidance, synthetic, uncertainty

import guidance_host_lib as gl
import rigview_host_lib as rl
from util import mirror

pytestmark = pytest.mark.gpu
CLASSES = dict(A=("A", "Q", "posterior"), gain=("gain", "pick_gain", "round_gain"),
               focus_rms=("focus_rms", "focus_before", "pick_focus_rms", "round_focus_rms"))
FIELDS = tuple(name for names in CLASSES.values() for name in names)
COUNTS = ("status", "n_visible", "n_cameras", "picks", "focus_status", "focus_n")
MIXED = [3, 4, 5]                  # 12 coefficients, 14 with the tilt, Kannala-Brandt
ALL = list(range(9))


def distance(a, b, name):
  """the largest difference of an output between two back-ends, in the units of the module's docstring"""
  x, y = np.asarray(getattr(a, name), dtype=np.float64), np.asarray(getattr(b, name), dtype=np.float64)
  assert np.array_equal(np.isnan(x), np.isnan(y)), name
  if x.size == 0:
    return 0.0
  d = np.nan_to_num(np.abs(x - y))
  if name in CLASSES["A"]:
    side = x.shape[-1] * x.shape[-2]
    return float((d.reshape(-1, side).max(axis=1) / np.maximum(np.abs(y).reshape(-1, side).max(axis=1), 1e-300)).max())
  if name in CLASSES["gain"]:
    return float((d / (1.0 + np.nan_to_num(np.abs(y)))).max())
  return float((d / np.maximum(np.nan_to_num(np.abs(y)), 1e-300)).max())


def compare(rig, factors, boards, views, focus, label, **kwargs):
  dev = rl.run(rig, factors, boards, views, focus, "device", with_rounds=True, **kwargs)
  host = rl.run(rig, factors, boards, views, focus, None, with_rounds=True, **kwargs)
  fast = rl.run(rig, factors, boards, views, focus, "fast", with_rounds=True, **kwargs)
  for name in COUNTS:
    assert np.array_equal(getattr(fast, name), getattr(host, name)), (label, name, "the two host builds")
    assert np.array_equal(getattr(dev, name), getattr(host, name)), (label, name)
  bad = host.status != guidance.OK
  assert np.isnan(dev.gain[bad]).all() and (dev.A[bad] == 0).all(), label
  worst = 0.0
  for kind, names in CLASSES.items():
    got, contraction = (max(distance(other, host, name) for name in names) for other in (dev, fast))
    print(f"{label}: {kind}: device - host {got:.3g}, contraction alone (two host builds) {contraction:.3g}")
    assert got <= 100.0 * contraction, (label, kind, got, contraction)
    worst = max(worst, got / contraction if contraction > 0 else 0.0)
  print(f"{label}: {int((~bad).sum())} of {bad.size} views OK; worst device / contraction ratio {worst:.3g}")
  return dev


def focus_of(rig, reference=0, distance=1.0, grid=(8, 6)):
  return guidance.RigFocus(reference, list(range(len(rig.cameras))), uncertainty.grid_of((gl.W_IMG, gl.H_IMG), grid), distance)


def views_of(rig, n, seed, distance=0.8, min_points=4, board=0):
  return [guidance.RigView(board, rl.rig_pose(rig, seed + k, distance + 0.05 * (k % 3), shift=0.02 + 0.02 * (k % 3)), min_points) for k in range(n)]


@pytest.mark.parametrize("P", [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193])
def test_points_per_view_at_step_lane_wave_and_chunk_edges(P):
  """a half-filled last MFMA K-step (odd P), lanes past the view's end, one and two waves, one and several rounds of chunks; a mixed
  group (Brown-Conrady with 12 and 14 coefficients, Kannala-Brandt).  Two corners leave the rotation about their line free whoever
  sees them; ONE corner seen by three cameras gives six equations for the six unknowns of the frame pose -- a pivot at the rule's
  edge --, so that case runs with two cameras, where the frame pose is plainly undetermined"""
  rig = rl.group(MIXED if P > 1 else MIXED[1:])
  fac = rl.device_factors(rig, rl.stored_factor(rig, 20, P))
  dev = compare(rig, fac, [rl.board(P, 0.012 if P < 130 else 0.007)], views_of(rig, 4, 10 * P, min_points=1), focus_of(rig), f"P = {P}", n=1)
  assert (dev.n_visible == P).mean() > 0.9 and (dev.n_cameras == len(rig.cameras)).all()
  assert (dev.status == (guidance.OK if P >= 3 else guidance.DEGENERATE)).all()


@pytest.mark.parametrize("r", [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 114, 127, 128])
def test_factor_widths_at_the_block_edges_and_the_lds_limit(r):
  """r at the 16-wide register blocks of k_rig_assemble, odd and even (the LDS stride of k_rig_score), the flagship's 114, and 128:
  k_rig_score's 132 KiB of dynamic LDS, requested through the function attribute"""
  rig = rl.group(MIXED)
  fac = rl.device_factors(rig, rl.stored_factor(rig, r, 1000 + r))
  criterion = "focus" if r % 2 else "gain"
  dev = compare(rig, fac, [rl.board(30)], views_of(rig, 5, 2000 + r), focus_of(rig, 1, np.inf if r % 3 == 0 else 1.5), f"r = {r}", n=3,
                criterion=criterion)
  assert (dev.status == guidance.OK).all() and dev.A.shape == (5, r, r) and (dev.picks >= 0).all() and dev.focus_status == guidance.OK


@pytest.mark.parametrize("V,n", [(1, 0), (2, 1), (5, 3), (300, 3)])
def test_views_per_call_and_picks(V, n):
  rig = rl.group(MIXED)
  fac = rl.device_factors(rig, rl.stored_factor(rig, 24, V))
  for criterion in ("focus", "gain"):
    dev = compare(rig, fac, [rl.board(16)], views_of(rig, V, 3000), focus_of(rig, 2, 1.2), f"V = {V}, n = {n}, by {criterion}", n=n,
                  criterion=criterion)
    assert (dev.status == guidance.OK).all() and (dev.picks[:min(n, V)] >= 0).all() and (dev.picks[V:] == -1).all()
  assert guidance.last_rig_call_ms()[1] == 3 * V


@pytest.mark.parametrize("members,towards,distance,want", [([0, 8], 0, 0.45, 1), ([4, 5], 0, 0.8, 2), (MIXED, 1, 0.8, 3), (ALL, 4, 1.5, 9)],
                         ids=["one", "two", "three", "nine"])
def test_cameras_contributing_per_view(members, towards, distance, want):
  rig = rl.group(members)
  fac = rl.device_factors(rig, rl.stored_factor(rig, 40, len(members)))
  views = [guidance.RigView(0, rl.rig_pose(rig, 4000 + k, distance, towards=towards), 20) for k in range(3)]
  dev = compare(rig, fac, [rl.board(36)], views, focus_of(rig, towards, 2.0), f"{want} cameras", n=2, min_cameras=1)
  assert (dev.n_cameras == want).all() and (dev.status == guidance.OK).all()


def test_a_camera_below_min_points_statuses_and_repeatability():
  rig = rl.group(MIXED)
  pts = rl.board(36)
  line = np.stack([np.linspace(-0.05, 0.05, 36), np.zeros(36), np.zeros(36)], axis=1)
  fac = rl.device_factors(rig, rl.stored_factor(rig, 33, 5))
  far = rl.rig_pose(rig, 4, 0.45, shift=0.1, towards=0)
  base = rl.run(rig, fac, [pts], [guidance.RigView(0, far, 1)], n=0, min_cameras=1)
  k, short = int(base.n_visible[0].min()), int(np.argmin(base.n_visible[0]))
  assert 0 < k < 36
  behind = far.copy()
  behind[2, 3] = -5.0
  views = views_of(rig, 4, 5000) + [guidance.RigView(0, far, k), guidance.RigView(0, far, k + 1), guidance.RigView(1, far, 4),
                                     guidance.RigView(0, behind, 1)]
  for n in (1, 3):
    dev = compare(rig, fac, [pts, line], views, focus_of(rig), f"statuses, n = {n}", n=n, min_cameras=2)
    assert list(dev.n_cameras[4:]) == [3, 2, 3, 0] and dev.n_visible[5, short] == k
    assert list(dev.status[4:]) == [guidance.OK, guidance.OK, guidance.DEGENERATE, guidance.TOO_FEW]
  loose = compare(rig, rl.device_factors(rig, rl.stored_factor(rig, 33, 5), loose=[short]), [pts, line], views, focus_of(rig), "a loose camera",
                  n=2, min_cameras=2, criterion="gain")
  assert loose.status[5] == guidance.OK and (loose.status[:5] == guidance.UNCONSTRAINED).all() and loose.focus_status == guidance.UNCONSTRAINED
  assert list(loose.picks) == [5, -1]
  one = rl.run(rig, fac, [pts, line], views, focus_of(rig), "device", n=3, with_rounds=True)
  two = rl.run(rig, fac, [pts, line], views, focus_of(rig), "device", n=3, with_rounds=True)
  for name in FIELDS + COUNTS:
    assert np.asarray(getattr(one, name)).tobytes() == np.asarray(getattr(two, name)).tobytes(), name
  assert guidance.last_rig_call_ms()[1] == 3 * len(views)
  empty = rl.run(rig, fac, [pts], [], focus_of(rig), "device", n=2)
  assert (empty.picks == -1).all() and guidance.last_rig_call_ms()[1] == 0
  with pytest.raises(Exception, match=r"r = 129.*smaller cameras= group"):
    rl.run(rig, [(np.zeros((24, 129)), False)] * 3, [pts], views, None, "device")


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_calibration_suggest_rig_views():
  c = mirror(synthetic.make_rig("tiny")).enable(cameras=True)
  dev = c.suggest_rig_views(n=3)
  host, fast = rl.on_host(c.suggest_rig_views, n=3), rl.on_fast(c.suggest_rig_views, n=3)      # (the covariance is the device's in all three)
  assert dev.poses.shape == (3, 4, 4) and dev.status == guidance.OK and dev.reference == 0 and list(dev.cameras) == [0, 1]
  for other in (dev, fast):
    assert np.array_equal(other.candidate_index, host.candidate_index) and (other.candidate_index >= 0).all()
    assert np.array_equal(other.n_visible, host.n_visible) and np.array_equal(other.scores.status, host.scores.status)
  assert (dev.n_cameras == 2).all()
  for name in ("gain", "focus_rms_before", "focus_rms_after"):
    got, contraction = distance(dev, host, name), distance(fast, host, name)
    print(f"tiny: {name}: device - host {got:.3g}, contraction alone (two host builds) {contraction:.3g}")
    assert got <= 100.0 * contraction, (name, got, contraction)
  chain = np.concatenate([[dev.focus_rms_before], dev.focus_rms_after])
  assert (np.diff(chain) < 0).all() and (dev.gain > 0).all()
  # before any view the focus is the transfer-uncertainty map of camera 0 into camera 1 at the focus distance
  u = c.projection_uncertainty(cameras=[1], reference=0, distance=dev.focus_distance)
  ok = u.status[0] == uncertainty.OK
  want = np.sqrt((u.cov[0][..., 0, 0] + u.cov[0][..., 1, 1])[ok].sum() / ok.sum())
  assert dev.scores.focus_n == ok.sum() and abs(dev.focus_rms_before - want) <= 1e-8 * want
  c.report_rig_view_suggestions(n=2)
  # the single-camera planner is as it was
  assert c.suggest_views(n=1).status.tolist() == [guidance.OK, guidance.OK]
