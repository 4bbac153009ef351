"""mcba_view_information on the device (k_view_schur, k_view_score, k_base_add) against the g++ build of the same header
(guidance_host_lib), and Calibration.suggest_views end to end.  Statuses, visible counts and picks are equal; S (relative to the
view's largest entry), gain (relative to 1 + gain) and focus_rms (relative) agree within 100 x what contraction alone does -- the
difference between two HOST builds of the header, -ffp-contract=off against -ffp-contract=fast, over the same call (measured here on
the CPU, printed; profiles/guidance_parity.txt)."""
import numpy as np
import pytest

from multical_amd import guidance, synthetic, uncertainty

import guidance_host_lib as gl
from util import mirror

pytestmark = pytest.mark.gpu
N_CAMERAS = 9
# the three quantities and the outputs that carry each: a call's spread is taken over all of them (one scalar alone -- the
# focus_before of a call with one camera -- is often the same in both host builds to the last bit)
CLASSES = dict(S=("S", "Q", "posterior"), gain=("gain", "pick_gain", "round_gain"),
               focus_rms=("focus_rms", "focus_before", "pick_focus_rms", "round_focus_rms"))
FIELDS = tuple(name for names in CLASSES.values() for name in names)


def distance(a, b, name):
  """the largest difference of an output between two back-ends, in the units of the module's docstring"""
  x, y = np.asarray(getattr(a, name), dtype=np.float64), np.asarray(getattr(b, name), dtype=np.float64)
  assert np.array_equal(np.isnan(x), np.isnan(y)), name
  if x.size == 0:
    return 0.0
  d = np.nan_to_num(np.abs(x - y))
  if name in ("S", "Q", "posterior"):
    return float((d.reshape(len(d), -1).max(axis=1) / np.maximum(np.abs(y).reshape(len(y), -1).max(axis=1), 1e-300)).max())
  if name in CLASSES["gain"]:
    return float((d / (1.0 + np.nan_to_num(np.abs(y)))).max())
  return float((d / np.maximum(np.nan_to_num(np.abs(y)), 1e-300)).max())


def compare(factors, boards, views, foci, label, **kwargs):
  dev = gl.run(factors, boards, views, foci, "device", with_rounds=True, **kwargs)
  host = gl.run(factors, boards, views, foci, None, with_rounds=True, **kwargs)
  fast = gl.run(factors, boards, views, foci, "fast", with_rounds=True, **kwargs)
  for name in ("status", "n_visible", "focus_status", "focus_n_visible", "picks"):
    assert np.array_equal(getattr(dev, name), getattr(host, name)), (label, name)
    assert np.array_equal(getattr(fast, name), getattr(host, name)), (label, name)
  bad = host.status != guidance.OK
  assert np.isnan(dev.gain[bad]).all() and (dev.S[bad] == 0).all(), label
  worst = 0.0
  for kind, names in CLASSES.items():
    got, contraction = (max(distance(other, host, name) for name in names) for other in (dev, fast))
    print(f"{label}: {kind}: device - host {got:.3g}, contraction alone (two host builds) {contraction:.3g}")
    assert got <= 100.0 * contraction, (label, kind, got, contraction)
    worst = max(worst, got / contraction if contraction > 0 else 0.0)
  print(f"{label}: {int((~bad).sum())} of {bad.size} views OK; worst device / contraction ratio {worst:.3g}")
  return dev


def factor_set(r_of, seed=0):
  """factors of all nine cameras: r_of(c) columns each"""
  return [gl.device_factor(c, gl.stored_factor(c, r_of(c), seed + c)) for c in range(N_CAMERAS)]


def foci_of(grid=(8, 6), distance=np.inf):
  return [guidance.Focus(c, distance, grid=uncertainty.grid_of((gl.W_IMG, gl.H_IMG), grid)) for c in range(N_CAMERAS)]


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 257])
def test_points_per_view_at_step_lane_wave_and_chunk_edges(P):
  """a half-filled last MFMA K-step (odd P), lanes past the view's end, one and two waves, one and several rounds; every camera
  family and every nuisance count in one call"""
  views = [guidance.View(c, 0, gl.pose(P + c, distance=0.5 if P < 130 else 0.7), nn, 1) for c in range(N_CAMERAS) for nn in (0, 3, 6)]
  dev = compare(factor_set(lambda c: 4 + gl.n_dist(c), P), [gl.board(P, 0.012 if P < 130 else 0.008)], views, foci_of(), f"P = {P}", n=1)
  assert (dev.n_visible > 0).all() and (dev.status[::3] == guidance.OK).all()
  if P >= 3:
    assert (dev.status == guidance.OK).mean() > 0.9 and (dev.n_visible == P).mean() > 0.9


@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 257])
def test_views_per_call(V):
  views = [guidance.View(i % N_CAMERAS, 0, gl.pose(1000 + i), (0, 3, 6)[i % 3], 4) for i in range(V)]
  dev = compare(factor_set(lambda c: 5, V), [gl.board(9)], views, foci_of((5, 4)), f"V = {V}", n=3, criterion="gain")
  assert (dev.status == guidance.OK).all()
  assert guidance.last_call_ms()[1] >= 0


@pytest.mark.parametrize("nn", [0, 3, 6])
@pytest.mark.parametrize("r", [1, 4, 9, 16, 18])
def test_factor_widths_at_the_tile_edge(r, nn):
  """r + n_nuisance from 1 to 24: one tile (<= 16 columns) and three"""
  c = 4                                                     # the 14-coefficient camera: 18 columns of its own
  views = [guidance.View(c, 0, gl.pose(2000 + i), nn, 4) for i in range(5)]
  fac = gl.empty_factors()
  fac[c] = gl.device_factor(c, gl.stored_factor(c, r, 10 * r + nn))
  foci = [guidance.Focus(k, 1.5, grid=uncertainty.grid_of((gl.W_IMG, gl.H_IMG), (8, 6))) if k == c else None for k in range(N_CAMERAS)]
  dev = compare(fac, [gl.board(70)], views, foci, f"r = {r}, n_nuisance = {nn}", n=3)
  assert (dev.status == guidance.OK).all() and dev.S.shape == (5, r, r)


def test_sparse_visibility_and_the_last_chunk():
  """every other corner visible; only the corners of the last chunk visible; nothing visible; one corner short of min_points"""
  full = gl.board(300, 0.006)
  away = np.array([50.0, 0.0, 0.0])
  every_other = full + np.where((np.arange(300) % 2 == 1)[:, None], away, 0.0)
  last_chunk = full + np.where((np.arange(300) < 256)[:, None], away, 0.0)
  nothing = full + away
  boards = [full, every_other, last_chunk, nothing]
  views = [guidance.View(c, b, gl.pose(3000 + c, distance=0.6), 6, m) for c in (0, 5, 7) for b, m in ((0, 4), (1, 150), (1, 151), (2, 4), (3, 1))]
  dev = compare(factor_set(lambda c: 6, 3), boards, views, foci_of(), "sparse visibility", n=2)
  assert list(dev.n_visible[:5]) == [300, 150, 150, 44, 0]
  assert list(dev.status[:5]) == [guidance.OK, guidance.OK, guidance.TOO_FEW, guidance.OK, guidance.TOO_FEW]


def test_statuses_mixed_families_and_repeatability():
  pts = gl.board(40)
  line = np.stack([np.linspace(-0.05, 0.05, 40), np.zeros(40), np.zeros(40)], axis=1)
  fac = factor_set(lambda c: 3 + c)
  fac[2] = (fac[2][0], True)                                # a loose intrinsic
  fac[3] = (np.zeros((4 + gl.n_dist(3), 0)), False)         # everything held
  views = [guidance.View(c, b, gl.pose(4000 + 3 * c + b), 6, 4) for c in range(N_CAMERAS) for b in (0, 1)]
  views += [guidance.Focus(c, 2.0, pixels=np.random.default_rng(c).uniform([0, 0], [gl.W_IMG - 1, gl.H_IMG - 1], (70, 2)), n_nuisance=6)
            for c in (1, 5, 8)]
  for n in (1, 3):
    dev = compare(fac, [pts, line], views, foci_of(distance=2.0), f"statuses, n = {n}", n=n)
    assert (dev.status[4:6] == guidance.UNCONSTRAINED).all() and (dev.status[6:8] == guidance.OK).all() and (dev.gain[6:8] == 0).all()
    assert (dev.status[1:18:2][[0, 1, 4, 5, 6, 7, 8]] == guidance.DEGENERATE).all()
    assert (dev.picks[2] == -1).all() and (dev.picks[3] == -1).all() and (dev.picks[0, 0] >= 0)
  one = gl.run(fac, [pts, line], views, foci_of(distance=2.0), "device", n=3, with_rounds=True)
  two = gl.run(fac, [pts, line], views, foci_of(distance=2.0), "device", n=3, with_rounds=True)
  for name in FIELDS + ("status", "n_visible", "picks"):
    assert np.asarray(getattr(one, name)).tobytes() == np.asarray(getattr(two, name)).tobytes(), name
  assert guidance.last_call_ms()[1] == 14 + 3 + 7           # the views and foci of the cameras that are served
  empty = gl.run(fac, [pts], [], None, "device", n=2)
  assert (empty.picks == -1).all() and guidance.last_call_ms()[1] == 0


# ---- end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "tiny_rolling"])
def test_calibration_suggest_views(name):
  c = mirror(synthetic.make_rig(name)).enable(cameras=True)
  dev = c.suggest_views(n=3)
  with gl.host_backend():
    host = c.suggest_views(n=3)
  C = c.size.cameras
  assert dev.poses.shape == (C, 3, 4, 4) and (dev.status == guidance.OK).all()
  assert np.array_equal(dev.candidate_index, host.candidate_index) and (dev.candidate_index >= 0).all()
  assert np.array_equal(dev.n_visible, host.n_visible) and np.array_equal(dev.scores.status, host.scores.status)
  assert np.allclose(dev.gain, host.gain, rtol=1e-9) and np.allclose(dev.focus_rms_after, host.focus_rms_after, rtol=1e-8)
  assert np.allclose(dev.focus_rms_before, host.focus_rms_before, rtol=1e-9)
  chain = np.concatenate([dev.focus_rms_before[:, None], dev.focus_rms_after], axis=1)
  assert (np.diff(chain, axis=1) < 0).all() and (dev.gain > 0).all()
  # the first pick is the candidate the uncertainty map agrees with: the intrinsics-only focus RMS before any view is that of
  # projection_uncertainty's map with the implied rotation fitted out, so it cannot exceed the plain map's RMS
  u = c.projection_uncertainty(cameras=[0], hold=None)
  assert dev.focus_rms_before[0] <= np.sqrt(np.nanmean(u.cov[0][..., 0, 0] + u.cov[0][..., 1, 1])) * (1 + 1e-9)
  c.report_view_suggestions(n=2)
