"""mcba_reconstruction_pairs on the device (k_reconstruction_pairs) against the g++ build of the same header
(length_uncertainty_host_lib), Calibration.length_errors end to end, and the entry inside the one resource cache of the handle-less
families.  Statuses and view masks are equal exactly, NaN patterns are equal.  cov_diff_cal and cov_diff_noise in whitened form
|L^-1 (C_dev - C_host) L^-T| with L L^T = C_host, cross_cal as |d|_ij / sqrt(C_a,ii C_b,jj) (it is not symmetric), the two variances
of the length relative: within 100 x what contraction alone does -- the difference between two HOST builds of the header,
-ffp-contract=off against -ffp-contract=fast, over the same pairs (measured here on the CPU, printed); a floor of 1e-13 only where
those two return the same bytes.  T = 8 pairs per tile: the a ends in rows 0 .. 7 of the MFMA tile, the b ends in rows 8 .. 15."""
import numpy as np
import pytest

from multical_amd import _lib, reconstruction, synthetic

import length_uncertainty_host_lib as ll
import reconstruction_uncertainty_host_lib as rl
from test_length_uncertainty_host import check_first_order_law, law_case
from util import mirror

pytestmark = pytest.mark.gpu
mats = reconstruction.covariance_matrices
cross = reconstruction.cross_matrices
T = 8


def volume_points(n, seed=0, G=3):
  """n points in front of the group, the first of them on its axis; every 11th behind it and every 13th far to one side"""
  rng = np.random.default_rng(seed)
  pts = rng.uniform([-0.3, -0.25, 1.0 + 0.15 * G], [0.3, 0.25, 3.0 + 0.15 * G], (n, 3))
  pts[0] = [0.0, 0.0, 2.0]
  pts[10::11, 2] *= -1.0
  pts[12::13, 0] += 2.5
  return pts


def random_pairs(n_points, k, seed):
  """k pairs over n_points points; the first is (0, 1 mod n); every 7th pair is a point with itself"""
  rng = np.random.default_rng(1000 + seed)
  pairs = rng.integers(0, n_points, size=(k, 2))
  pairs[0] = [0, 1 % n_points]
  pairs[6::7, 1] = pairs[6::7, 0]
  return pairs


def relative(got, want):
  with np.errstate(invalid="ignore", divide="ignore"):
    d = np.abs(got - want) / np.abs(want)
  return np.where(got == want, 0.0, d)


def compare(model, jobs, pairs, label, sigma2=0.3, margin=0.0):
  dev = ll.run(model, jobs, pairs, sigma2, margin, "device")
  host = ll.run(model, jobs, pairs, sigma2, margin)
  fast = ll.run(model, jobs, pairs, sigma2, margin, "fast")
  for k in ("status", "views_a", "views_b"):
    assert np.array_equal(dev[k], host[k]) and np.array_equal(fast[k], host[k]), (label, k)
  assert dev.length.tobytes() == host.length.tobytes() or np.abs(dev.length - host.length).max() <= 4e-16 * np.abs(host.length).max(), label
  ok = host.status == reconstruction.OK
  for k in ll.COVARIANCES:
    assert np.array_equal(np.isnan(dev[k]), np.isnan(host[k])) and np.isnan(dev[k][~ok]).all(), (label, k)
  if not ok.any():
    return dev
  # the covariances of the two ends, for the scale of cross_cal: the point entry of the host build over the same jobs
  point = rl.run(model, jobs, sigma2, margin)
  first = np.concatenate([[0], np.cumsum([len(j.points) for j in jobs])])
  at = np.concatenate([first[j] + np.asarray(p, dtype=np.int64).reshape(-1, 2) for j, p in enumerate(pairs)])
  Ca, Cb = mats(point.cov_cal)[at[ok, 0]], mats(point.cov_cal)[at[ok, 1]]
  measures = dict(cov_diff_cal=lambda x, y: rl.whitened_difference(mats(x[ok]), mats(y[ok])),
                  cov_diff_noise=lambda x, y: rl.whitened_difference(mats(x[ok]), mats(y[ok])),
                  cross_cal=lambda x, y: ll.cross_difference(cross(x[ok]), cross(y[ok]), Ca, Cb))
  for k, measure in measures.items():
    contraction, got = measure(fast[k], host[k]).max(), measure(dev[k], host[k]).max()
    same = fast[k].tobytes() == host[k].tobytes()
    print(f"{label} {k}: {int(ok.sum())} of {ok.size} pairs OK; device - host {got:.3g}, contraction alone (two host builds) "
          f"{contraction:.3g}{' (the same bytes)' if same else ''}")
    assert got <= (1e-13 if same else 100.0 * contraction), (label, k)
  # the variances of the length are u^T C u of covariances that agree as above: |d var| <= w (var + 1e-6 lambda_max) with w the whitened
  # difference of C (whose floor is 1e-6 lambda_max), and the evaluation of u^T C u itself adds 1000 eps |C|
  for k, c in (("length_var_cal", "cov_diff_cal"), ("length_var_noise", "cov_diff_noise")):
    measured = np.isfinite(host[k]) & ok
    if not measured.any():
      continue
    w = rl.whitened_difference(mats(dev[c][measured]), mats(host[c][measured]))
    size = np.abs(host[c][measured]).max(axis=1)
    bound = w * (host[k][measured] + 3e-6 * size) + 1000.0 * np.finfo(np.float64).eps * size
    d = np.abs(dev[k][measured] - host[k][measured])
    print(f"{label} {k}: worst |device - host| / bound {np.max(d / np.maximum(bound, 1e-300)) if (bound > 0).any() else 0.0:.3g}; worst "
          f"relative difference {relative(dev[k][measured], host[k][measured]).max():.3g}")
    assert (d <= bound).all(), (label, k)
  return dev


def job(model, ref, r, n, seed, masks=None):
  return rl.job_of(model, ref, rl.random_factors(model, r, seed)[0], volume_points(n, seed, len(model.cameras)), masks)


# ---- 1 .. 3: counts, widths, groups --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, T - 1, T, T + 1, 4 * T - 1, 4 * T, 4 * T + 1, 16 * T + 1])
def test_pair_counts_at_tile_and_wave_edges(k):
  m, _ = rl.group_rig(3, 3)
  dev = compare(m, [job(m, None if k % 2 else 1, 17, 33, k)], [random_pairs(33, k, k)], f"{k} pairs")
  assert dev.status[0] == reconstruction.OK and reconstruction.last_pair_call_ms()[1] == k


@pytest.mark.parametrize("r", [0, 1, 15, 16, 17, 33, 128])
def test_factor_widths_at_column_tile_edges(r):
  m, _ = rl.group_rig(5, 3)
  for ref in (None, 2):
    dev = compare(m, [job(m, ref, r, 33, r)], [random_pairs(33, 3 * T + 3, r)], f"r = {r} reference {ref}")
    if r == 0:
      ok = dev.status == reconstruction.OK
      assert (dev.cov_diff_cal[ok] == 0).all() and (dev.cross_cal[ok] == 0).all()


@pytest.mark.parametrize("G", [2, 3, 5, 8])
@pytest.mark.parametrize("ref", [None, "last"], ids=["rig", "camera"])
def test_group_sizes_with_mixed_families(G, ref):
  m, _ = rl.group_rig(G % 9, G)
  dev = compare(m, [job(m, None if ref is None else G - 1, 20, 40, G)], [random_pairs(40, 2 * T + 5, G)], f"G = {G} reference {ref}")
  assert (dev.status == reconstruction.OK).mean() > 0.5 and max(bin(int(v)).count("1") for v in dev.views_a) == G


# ---- 4: the geometries of one job ----------------------------------------------------------------------------------------------
def test_pair_geometries_of_one_job():
  """40 points: (first, last), (last, first), (k, k); one point in every pair of a tile; a tile whose a ends are all failed points and
  whose b ends are OK, and the reverse; masks that remove the first, the last and a middle slot from one end only"""
  m, _ = rl.group_rig(1, 5)
  n = 40
  pts = volume_points(n, 2, 5)
  failed = np.flatnonzero(pts[:, 2] < 0)                       # (behind the group: 10, 21, 32)
  good = [i for i in range(n) if i not in set(failed) and i not in set(range(12, n, 13))]
  assert len(failed) == 3 and len(good) >= 30
  masks = np.full(n, 0b11111, dtype=np.uint64)
  masks[good[1]], masks[good[2]], masks[good[3]] = 0b11110, 0b01111, 0b11011
  pairs = [[0, n - 1], [n - 1, 0]] + [[k, k] for k in (0, good[5], failed[0], n - 1)]
  pairs += [[0, 0]] * (T - len(pairs) % T)                                     # (fill the tile)
  pairs += [[good[4], good[6 + t]] for t in range(T)]                          # one point in every pair of a tile
  pairs += [[failed[t % 3], good[10 + t]] for t in range(T)]                   # a ends all failed, b ends OK
  pairs += [[good[10 + t], failed[t % 3]] for t in range(T)]                   # and the reverse
  pairs += [[good[1], good[7]], [good[7], good[1]], [good[2], good[8]], [good[8], good[2]], [good[3], good[9]], [good[9], good[3]]]
  pairs = np.array(pairs)
  factors = rl.random_factors(m, 30, 2)[0]
  dev = compare(m, [rl.job_of(m, 4, factors, pts, masks)], [pairs], "geometries")
  OK, TF = reconstruction.OK, reconstruction.TOO_FEW
  # every end is the point the pair names: its views and its status are those of the point entry (host build) for THAT point
  point, unmasked = rl.run(m, [rl.job_of(m, 4, factors, pts, masks)]), rl.run(m, [rl.job_of(m, 4, factors, pts)])
  assert np.array_equal(dev.views_a, point.views[pairs[:, 0]]) and np.array_equal(dev.views_b, point.views[pairs[:, 1]])
  sa, sb = point.status[pairs[:, 0]], point.status[pairs[:, 1]]
  assert np.array_equal(dev.status, np.where(sa != OK, sa, sb))
  for i, slot in ((1, 0), (2, 4), (3, 2)):                     # (the masks do remove a view, from that end only)
    assert (unmasked.views[good[i]] >> np.uint64(slot)) & np.uint64(1) and not (point.views[good[i]] >> np.uint64(slot)) & np.uint64(1)
    assert point.views[good[6 + i]] == unmasked.views[good[6 + i]]
  assert np.allclose(cross(dev.cross_cal)[0], cross(dev.cross_cal)[1].T, rtol=1e-9, atol=1e-300)
  assert (dev.cov_diff_cal[[2, 3]] == 0).all() and (dev.length[[2, 3]] == 0).all() and dev.status[4] == TF
  assert (dev.status[2 * T:3 * T] == TF).all() and (dev.status[3 * T:4 * T] == TF).all() and (dev.status[T:2 * T] == OK).all()
  assert (dev.views_a[2 * T:3 * T] == 0).all() and (dev.views_b[2 * T:3 * T] != 0).all() and (dev.views_b[3 * T:4 * T] == 0).all()
  assert (dev.status[4 * T:] == OK).all()


# ---- 5, 6 --------------------------------------------------------------------------------------------------------------------
def test_two_jobs_of_different_group_width_and_pair_count_share_a_call():
  """G = 8 with r = 40 over 37 points and 19 pairs (its last tile holds 3) and G = 2 with r = 7 over 18 points and 11 pairs: the second
  job's pairs index ITS points, its first tile is its own, and the call takes the wide stage"""
  big, _ = rl.group_rig(0, 8)
  maps, rng = rl.stored_maps(big), np.random.default_rng(5)
  small = reconstruction.Job([6, 2], 2, [(maps[c] @ (1e-4 * rng.normal(size=(maps[c].shape[1], 7))), False) for c in (6, 2)],
                             volume_points(18, 6, 2), np.array([3] * 17 + [1], dtype=np.uint64))
  p_big, p_small = random_pairs(37, 19, 1), random_pairs(18, 11, 2)
  p_small[-1] = [17, 0]
  dev = compare(big, [job(big, None, 40, 37, 4), small], [p_big, p_small], "G = 8 | G = 2")
  assert max(bin(int(v)).count("1") for v in dev.views_a[:19]) == 8 and dev.views_a[19:].max() == 3
  assert dev.status[-1] == reconstruction.TOO_FEW
  alone = ll.run(big, [small], [p_small], 0.3, 0.0, "device")
  assert all(np.asarray(alone[k]).tobytes() == np.asarray(dev[k][19:]).tobytes() for k in ll.RAW)


def test_a_call_whose_pairs_all_fail():
  m, _ = rl.group_rig(3, 3)
  pts = np.tile([[0.0, 0.0, -2.0]], (20, 1)) + np.arange(20)[:, None] * [0.01, 0.0, 0.0]
  f = rl.random_factors(m, 9, 1)[0]
  dev = compare(m, [rl.job_of(m, None, f, pts), rl.job_of(m, 1, f, pts[:3] + [5.0, 0, 4.0])], [random_pairs(20, 2 * T + 1, 3), [[0, 1], [2, 2]]],
                "behind | to one side")
  assert (dev.status == reconstruction.TOO_FEW).all() and np.isfinite(dev.length).all()
  assert all(np.isnan(dev[k]).all() for k in ll.COVARIANCES)


# ---- 7: one cache, the same bytes ------------------------------------------------------------------------------------------
def test_repeatable_and_the_point_entry_keeps_its_bytes_around_a_pair_call():
  m, _ = rl.group_rig(4, 5)
  jobs = [job(m, 2, 50, 100, 7), job(m, None, 9, 20, 8)]
  pairs = [random_pairs(100, 61, 7), random_pairs(20, 9, 8)]
  own = lambda: ll.raw_bytes(ll.run(m, jobs, pairs, 0.3, 0.0, "device"))

  def point_entry():
    out = rl.run(m, jobs, 0.3, 0.0, "device")
    return b"".join(out[k].tobytes() for k in ("cov_cal", "cov_noise", "n_views", "views", "status"))

  before = point_entry()
  first = own()
  assert own() == first and reconstruction.last_pair_call_ms()[1] == 70
  assert point_entry() == before and reconstruction.last_call_ms()[1] == 120
  assert own() == first
  with pytest.raises(RuntimeError) as e:
    ll.run(m, jobs, [pairs[0], [[0, 20]]], 0.3, 0.0, "device")
  message = "mcba_reconstruction_pairs: pairs: pair 61 (0 of job 1): index 20 is outside [0, n = 20)"
  assert message in str(e.value) and message in _lib.load().mcba_last_error().decode()
  assert own() == first and point_entry() == before


# ---- 8: end to end ---------------------------------------------------------------------------------------------------------
def test_calibration_length_errors():
  """on the tiny golden rig with the covariance from the device: length is |X_a - X_b| of triangulate(); every valid pair has a finite
  studentised error and a positive std_cal; at least half of the default pairs are valid in at least one frame (a property of
  `tiny` under the default inlier mask); the median |studentised| is printed"""
  c = mirror(synthetic.make_rig("tiny")).enable(cameras=True)
  e = c.length_errors()
  t = c.triangulate()
  F, B, K = e.valid.shape
  assert e.pairs.shape == (B, K, 2) and K == c.size.points
  f, b, k = np.nonzero(e.valid)
  Xa, Xb = t.points[f, b, e.pairs[b, k, 0]], t.points[f, b, e.pairs[b, k, 1]]
  assert np.abs(e.length[f, b, k] - np.linalg.norm(Xa - Xb, axis=1)).max() <= 1e-12
  assert np.isfinite(e.studentized[e.valid]).all() and (e.std_cal[e.valid] > 0).all() and (e.std_noise[e.valid] > 0).all()
  assert np.isnan(e.studentized[~e.valid]).all()
  both = t.valid[np.arange(F)[:, None, None], np.arange(B)[None, :, None], e.pairs[None, :, :, 0]] & \
      t.valid[np.arange(F)[:, None, None], np.arange(B)[None, :, None], e.pairs[None, :, :, 1]]
  assert not (e.valid & ~both).any() and e.valid.sum() >= 0.9 * both.sum()
  share = e.valid.any(axis=0).mean()
  s = e.studentized[e.valid]
  print(f"tiny: {int(e.valid.sum())} valid pairs of {int(both.sum())} with both corners triangulated; {100 * share:.0f} % of the default "
        f"pairs valid in a frame; median |studentised| {np.median(np.abs(s)):.3f}, RMS {np.sqrt(np.mean(s ** 2)):.3f}; length error RMS "
        f"{1e3 * e.overall.rms:.4f} mm; median std calibration {1e3 * np.median(e.std_cal[e.valid]):.4f} mm, noise "
        f"{1e3 * np.median(e.std_noise[e.valid]):.4f} mm")
  assert share >= 0.5
  assert np.allclose(e.error[e.valid], e.length[e.valid] - e.board_length[e.valid], rtol=0, atol=0)


def test_the_report_runs():
  import logging
  c = mirror(synthetic.make_rig("tiny")).enable(cameras=True)
  records = []
  handler = logging.Handler()
  handler.emit = records.append
  logging.getLogger("calibration").addHandler(handler)
  try:
    logging.getLogger("calibration").setLevel(logging.INFO)
    c.report_length_uncertainty("test", reference=0)
  finally:
    logging.getLogger("calibration").removeHandler(handler)
  lines = [r.getMessage() for r in records]
  print("\n".join(lines))
  bars = [l for l in lines if "calibration/noise/naive" in l]
  assert len(bars) == c.size.cameras - 1 and any("studentised" in l for l in lines), lines


# ---- 9: the first-order law --------------------------------------------------------------------------------------------------
def test_first_order_law():
  m, factors, pts, ref, pairs = law_case()
  out = ll.run(m, [rl.job_of(m, ref, factors, pts)], [pairs], backend="device")
  check_first_order_law(out, m, ref, pts)
