"""The corner refinement on the CPU: the g++ build of csrc/mcba_subpix.h (tests/subpix_host) against the independent numpy restatement
(tests/subpix_reference.py) on the planted images, its statuses and refusals, the table and detection wrappers, and the header under
AddressSanitizer + UBSan in a stand-alone program.

Measured (profiles/subpix_parity.txt): at a fixed count the host build and the restatement differ by at most 1.4e-14 px, where
rounding alone predicts about 1e-13; the bound asserted is the 1e-9 px of the feature's contract."""
import re

import numpy as np
import pytest

import host_build
import subpix_host_lib as shl
import subpix_reference as ref
from multical_amd import _lib, subpix, tables
from multical_amd.structs import Table, struct

CASES = ref.planted_cases()
DTYPES = [np.uint8, np.float32]
EPS = 1e-4


def _host(case, dtype, fixed):
  name, img, truth, w, r = CASES[case]
  return shl.refine_on_host(ref.as_dtype(img, dtype), ref.starts(truth, r), window=w, max_iter=30, eps=0.0 if fixed else EPS)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_fixed_count_parity(case, dtype):
  """eps = 0, 30 iterations: the host build is within 1e-9 px of the restatement (the iteration reaches a fixed point, so rounding
  differences do not grow)"""
  R, S, I, Q = ref.reference_run(case, True)
  hR, hS, hI, hQ = _host(case, dtype, True)
  worst = np.abs(hR - R).max()
  print(f"{CASES[case][0]} {np.dtype(dtype).name}: host build - restatement {worst:.3e} px")
  assert worst <= 1e-9
  assert (hS == S).all() and (hI == I).all()
  assert np.abs(hQ - Q).max() <= 1e-9 * np.abs(Q).max()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_reference_criteria(case, dtype):
  """eps = 1e-4, 30 iterations: every corner stops on eps under the restatement (asserted for the restatement), and the host build
  agrees in position, iterations and status, and is no further from the truth"""
  name, img, truth, w, r = CASES[case]
  R, S, I, Q = ref.reference_run(case, False)
  assert (S == ref.OK).all() and I.max() <= ref.MAX_ITERATIONS_MEASURED
  hR, hS, hI, hQ = _host(case, dtype, False)
  assert (hS == S).all()
  assert np.abs(hR - R).max() <= EPS
  assert np.abs(hI.astype(int) - I).max() <= 1
  err_ref, err_host = np.linalg.norm(R - truth, axis=1), np.linalg.norm(hR - truth, axis=1)
  err_start = np.linalg.norm(ref.starts(truth, r) - truth, axis=1)
  assert (err_host <= err_ref + 1e-9).all()
  assert (err_host < err_start).all()


@pytest.mark.parametrize("case", range(len(CASES)))
def test_wave_order_reducer(case):
  """the host build that sums in the order of the device's lanes and butterfly: within 1e-9 px of the one in row order"""
  name, img, truth, w, r = CASES[case]
  for fixed in (True, False):
    kw = dict(window=w, max_iter=30, eps=0.0 if fixed else EPS)
    serial = shl.refine_on_host(img, ref.starts(truth, r), **kw)
    wave = shl.refine_in_wave_order(img, ref.starts(truth, r), **kw)
    assert np.abs(wave[0] - serial[0]).max() <= (1e-9 if fixed else EPS)
    assert (wave[1] == serial[1]).all() and np.abs(wave[2].astype(int) - serial[2]).max() <= (0 if fixed else 1)
    assert np.abs(wave[3] - serial[3]).max() <= 1e-9 * np.abs(serial[3]).max()


def test_measured_errors_to_truth():
  """the worst error to the truth of the restatement is the measured one of every planted case"""
  measured = [0.124, 0.086, 0.059, 0.043, 0.033, 0.024]
  for case, want in enumerate(measured):
    R = ref.reference_run(case, False)[0]
    assert abs(np.linalg.norm(R - CASES[case][2], axis=1).max() - want) < 1e-3


@pytest.mark.parametrize("image,window,radius", [("A", (7, 3), 1.0), ("B", (15, 1), 1.0)])
def test_non_square_windows(image, window, radius):
  img, truth = ref.image_a() if image == "A" else ref.image_b()
  start = ref.starts(truth, radius)
  R, S, I, Q = ref.refine(img, start, window)
  assert (S == ref.OK).all()
  for dtype in DTYPES:
    hR, hS, hI, hQ = shl.refine_on_host(ref.as_dtype(img, dtype), start, window=window)
    assert (hS == S).all() and np.abs(hR - R).max() <= EPS and np.abs(hI.astype(int) - I).max() <= 1
    assert (np.linalg.norm(hR - truth, axis=1) < np.linalg.norm(start - truth, axis=1)).all()
  # the window is not the transposed one
  tR = shl.refine_on_host(img, start, window=window[::-1])[0]
  assert np.abs(tR - R).max() > 1e-6


def test_zero_zone():
  """(two iterations: the centre pixel has i = j = 0 and enters a, b, d only, so the zone (0, 0) changes the path of the iteration
  and the quality, not its fixed point)"""
  A, truth = ref.image_a()
  start = ref.starts(truth, 2.0)
  kw = dict(window=5, max_iter=2, eps=0.0)
  plain = shl.refine_on_host(A, start, zero_zone=-1, **kw)
  for zone in ((-1, -1), (5, 5), (7, 7), (2, 5), (5, 0), (0, -1)):      # none, oversize, oversize or absent on one axis
    again = shl.refine_on_host(A, start, zero_zone=zone, **kw)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, plain)), zone
  for zone in ((0, 0), (1, 1), (4, 4), (3, 0)):
    R, S, I, Q = ref.refine(A, start, 5, zero_zone=zone, max_iter=2, eps=0.0)
    hR, hS, hI, hQ = shl.refine_on_host(A, start, zero_zone=zone, **kw)
    assert np.abs(hR - plain[0]).max() > 1e-7, zone
    assert np.abs(hR - R).max() <= 1e-9 and (hS == S).all(), zone
    assert np.abs(hQ - Q).max() <= 1e-9 * np.abs(Q).max()


@pytest.mark.parametrize("case", shl.status_cases(), ids=lambda c: c[0])
def test_status_cases(case):
  name, img, corners, kw = case
  window = kw["window"]
  R, S, I, Q = ref.refine(img, corners, window, max_iter=kw.get("max_iter", 30), eps=kw.get("eps", EPS))
  for dtype in DTYPES:
    hR, hS, hI, hQ = shl.refine_on_host(ref.as_dtype(img, dtype), corners, **kw)
    assert (hS == S).all() and (hI == I).all()
    assert np.array_equal(np.isnan(hR), np.isnan(R)) and np.nanmax(np.abs(hR - R), initial=0.0) <= 1e-9
    assert np.array_equal(np.isnan(hQ), np.isnan(Q))
    assert np.nanmax(np.abs(hQ - Q), initial=0.0) <= 1e-9 * max(np.nanmax(np.abs(Q), initial=0.0), 1.0)
    kept = np.isin(hS, [subpix.REVERTED, subpix.INVALID, subpix.SINGULAR])
    assert hR[kept].tobytes() == np.asarray(corners, dtype=np.float64)[kept].tobytes()
  if name.startswith("border-w"):
    assert (I == 3).sum() >= 12            # most border starts run all three iterations through the replicate border
  if name == "constant":
    assert (S == subpix.SINGULAR).all() and (hQ == 0.0).all() and (hI == 1).all()
  if name == "invalid":
    assert (S == subpix.INVALID).all() and np.isnan(hQ).all() and (hI == 0).all()
  if name == "away":
    assert np.isin(S, [subpix.REVERTED, subpix.MAX_ITER]).all() and (S == subpix.REVERTED).any()
  if name == "one-iteration":
    assert (S == subpix.MAX_ITER).all() and (hI == 1).all()


def test_refused_arguments():
  A, truth = ref.image_a()

  def refused(pattern, images=A, corners=truth, **kw):
    with pytest.raises(RuntimeError, match=pattern):
      shl.refine_on_host(images, corners, **kw)

  for window in (0, 16, (5, 0), (16, 5), -1):
    refused("half window must be 1 .. 15", window=window)
  for max_iter in (0, 101, -3):
    refused("max_iter must be 1 .. 100", max_iter=max_iter)
  for eps in (-1e-9, np.nan, np.inf):
    refused("eps must be finite and not negative", eps=eps)
  of = np.zeros(len(truth), dtype=np.int32)
  of[7] = 3
  of[9] = -1
  refused("corner 7 names image 3 of 3", images=np.stack([A, A, A]), image_of_corner=of)
  of[7] = 0
  refused("corner 9 names image -1 of 3", images=np.stack([A, A, A]), image_of_corner=of)
  refused("image sizes must be 2 ..", images=A[:1])
  refused("image sizes must be 2 ..", images=np.ascontiguousarray(A[:, :1]))
  with pytest.raises(TypeError):
    shl.refine_on_host(A.astype(np.float64), truth)
  with pytest.raises(ValueError, match="grey"):
    shl.refine_on_host(np.zeros((1, 8, 8, 3), dtype=np.uint8), truth)
  # no corners: returns at once, with or without an image
  for images in (A, np.zeros((0, 96, 128), dtype=np.uint8)):
    out = shl.refine_on_host(images, np.zeros((0, 2)))
    assert [len(a) for a in out] == [0, 0, 0, 0]
  refused("corners but no image", images=np.zeros((0, 96, 128), dtype=np.uint8))


def _table_inputs():
  """a 2-camera x 3-frame table with two image sizes (camera 1 sees crops) and empty views; float32 points"""
  A, tA = ref.image_a()
  B, tB = ref.image_b()
  crop = (80, 120)
  images = [np.stack([A, B, A]), np.stack([B[:crop[0], :crop[1]], A[:crop[0], :crop[1]], B[:crop[0], :crop[1]]])]
  P = 25
  points, valid = np.zeros((2, 3, 2, P, 2), dtype=np.float32), np.zeros((2, 3, 2, P), dtype=bool)
  noisy_a, noisy_b = ref.starts(tA, 1.0), ref.starts(tB, 1.0, seed=3)
  points[0, 0, 0], valid[0, 0, 0] = noisy_a, True
  points[0, 1, 1, :8], valid[0, 1, 1, :8] = noisy_b, True
  points[0, 2, 0, ::2], valid[0, 2, 0, ::2] = noisy_a[::2], True
  inside = (tA[:, 0] < crop[1] - 8) & (tA[:, 1] < crop[0] - 8)
  points[1, 1, 0, inside], valid[1, 1, 0, inside] = noisy_a[inside], True
  points[1, 2, 1, :3], valid[1, 2, 1, :3] = noisy_b[:3], True       # (camera 1, frame 0 and several boards: empty views)
  points[~valid] = -7.0
  return images, Table.create(points=points, valid=valid)


def test_refine_point_table():
  images, table = _table_inputs()
  calls = []
  with shl.host_backend():
    entry = subpix._entry
    subpix._entry = lambda name: (calls.append(name), entry(name))[1]
    try:
      out, status = tables.refine_point_table(images, table, window=4)
    finally:
      subpix._entry = entry
  assert len(calls) == 2                                   # one call per image size
  assert out.points.dtype == np.float32 and out.points.shape == table.points.shape
  assert np.array_equal(out.valid, table.valid)
  assert (out.points[~table.valid] == -7.0).all() and (status[~table.valid] == subpix.INVALID).all()
  for c, f, b in np.ndindex(2, 3, 2):
    v = table.valid[c, f, b]
    if not v.any():
      continue
    R, S = shl.refine_on_host(images[c][f], table.points[c, f, b][v].astype(np.float64), window=4)[:2]
    assert out.points[c, f, b][v].tobytes() == R.astype(np.float32).tobytes()
    assert np.array_equal(status[c, f, b][v], S)
  assert (status[table.valid] == subpix.OK).all()
  # drop: the slots of those statuses lose `valid`, and only those
  far = np.array(table.points)
  far[0, 0, 0, 0] += 7.5
  moved = Table.create(points=far, valid=table.valid)
  with shl.host_backend():
    kept, st = tables.refine_point_table(images, moved, window=4)
    dropped, st2 = tables.refine_point_table(images, moved, window=4, drop=("singular", "reverted", "left_image"))
  bad = np.isin(st, [subpix.SINGULAR, subpix.REVERTED, subpix.LEFT_IMAGE])
  assert bad[0, 0, 0, 0] and np.array_equal(kept.valid, table.valid)
  assert np.array_equal(st, st2) and np.array_equal(dropped.valid, table.valid & ~bad)


def test_subpix_corners_keeps_dtype():
  A, truth = ref.image_a()
  start = ref.starts(truth, 2.0)
  for dtype in (np.float32, np.float64):
    det = struct(corners=start.astype(dtype), ids=np.arange(len(start)))
    out = shl.on_host(subpix.subpix_corners, A, det, 5)
    assert out.corners.dtype == dtype and out.corners.shape == start.shape and np.array_equal(out.ids, det.ids)
    R = shl.refine_on_host(A, start.astype(dtype).astype(np.float64), window=5, zero_zone=-1, max_iter=30, eps=EPS)[0]
    assert out.corners.tobytes() == R.astype(dtype).tobytes()
    assert np.linalg.norm(out.corners - truth, axis=1).max() < 0.07


def test_sanitized_program(tmp_path):
  """the border and INVALID cases in a stand-alone program under AddressSanitizer + UBSan (CPU only, nothing loaded into Python)"""
  r = host_build.sanitized_program("subpix_host", "subpix_sanitize_main.cpp", tmp_path)
  assert r.returncode == 0 and "subpix sanitize run: ok" in r.stdout, r.stdout + r.stderr


def test_symbols_declared_and_bound():
  header = open(host_build.ROOT + "/include/mcba.h").read()
  bound = {name for name, _, _ in _lib.SYMBOLS}
  for name in ("mcba_refine_corners", "mcba_debug_subpix_ms"):
    assert re.search(r"\b%s\(" % name, header) and name in bound
  for name, value in subpix.STATUS_NAMES.items():
    assert re.search(r"#define MCBA_SUBPIX_%s %d\b" % (name.upper(), value), header)
