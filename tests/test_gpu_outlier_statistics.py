"""GPU (MI355X): the device order statistics and the rejection of the outlier loop on PLANTED error tables -- k_selm_init / hist / pick /
next / fold / finish behind select_ranks_multi and error_stats_impl, k_reject, k_err_sums / k_sum2, the active-view refresh, and the
two quantile lerps (error_stats_with_quantiles in C, Handle.error_stats in Python).

Geometry cannot produce the values a radix select goes wrong on (proj + e - proj quantises to about 2^-43 px), so the tables of
tests/error_tables.py are written into the handle with mcba_debug_set_error_table: ties, all-zero, keys that differ in the last
9 / 20 bits only, subnormals, 10^+-300 with +inf, and keys whose digit sits on a bin edge in every pass.  Invalid slots are planted
with NaN: the hook has to ignore them.  Rigs: `tiny` (972 slots), `tiny_edge` (an invalid camera, an invalid frame, an empty frame),
`tiny_bigboard` at 21 frames (68 544 slots: the grid stride of k_selm_next wraps) and at 81 frames (264 384 slots: those of
k_selm_hist and k_err_sums wrap), and copies of `tiny` with exactly 1, 2, 3 and 5 valid points (0 for the refusal).

Every reference is numpy on the planted table.  Selected values, quantiles, masks and counts are compared bit for bit (quantiles
with NaN == NaN: numpy's lerp yields NaN next to +inf and both lerps of the product must do the same); sums of squares to the
project's 1e-12 relative against math.fsum.  Frame-sharded selection (W > 1) stays with tests/test_sharded_calibrate.py."""
import copy
import ctypes as C
import functools
import math

import numpy as np
import pytest

import error_tables as et
from multical_amd import synthetic
from multical_amd._lib import McbaError
from multical_amd.backend import Handle
from util import load_golden, mirror, oracle

pytestmark = pytest.mark.gpu

SMALL_RIGS = ["tiny", "tiny_edge", "tiny_n1", "tiny_n2", "tiny_n3", "tiny_n5"]
LARGE_RIGS = ["bigboard21", "bigboard81"]
CASES = [(r, t) for r in SMALL_RIGS for t in et.TABLES] + [(r, t) for r in LARGE_RIGS for t in et.LARGE_TABLES]
FINITE_CASES = [(r, t) for r, t in CASES if t not in ("wide", "digit_edges")]       # (no +inf: the C report takes finite tables)
cases = pytest.mark.parametrize("rig,table", CASES, ids=[f"{r}-{t}" for r, t in CASES])
finite_cases = pytest.mark.parametrize("rig,table", FINITE_CASES, ids=[f"{r}-{t}" for r, t in FINITE_CASES])
QUANTILES = [0, .25, .5, .75, 1, .95, .123, 1 / 3, 1e-9, 1 - 1e-9]
FIVE = [0, .25, .5, .75, 1]


def cut_valid(rig, k):
  """copy of the rig with exactly k valid points, spread over its views"""
  rig = copy.deepcopy(rig)
  idx = np.flatnonzero(rig.valid)
  keep = idx[np.linspace(0, idx.size - 1, k).astype(np.int64)] if k > 0 else idx[:0]
  assert np.unique(keep).size == k
  valid = np.zeros(rig.valid.size, dtype=bool)
  valid[keep] = True
  rig.valid = valid.reshape(rig.valid.shape)
  rig.points = np.where(rig.valid[..., None], rig.points, 0).astype(rig.points.dtype)
  return rig


@functools.lru_cache(maxsize=None)
def make_rig(name):
  if name == "tiny_edge":
    return load_golden(name)[1]
  if name.startswith("tiny_n"):
    return cut_valid(synthetic.make_rig("tiny"), int(name[6:]))
  if name.startswith("bigboard"):
    return synthetic.make_rig("tiny_bigboard", frames=int(name[8:]))
  return synthetic.make_rig(name)


class Case(object):
  """One rig with its handle; the handle is shared by the tests of the module (each starts from the full inlier set)."""

  def __init__(self, name):
    self.name = name
    self.rig = make_rig(name)
    self.c = mirror(self.rig)
    self.x = np.ascontiguousarray(self.c.param_vec, dtype=np.float64).copy()
    self.x2 = self.x + 1e-3 * np.random.default_rng(5).normal(size=self.x.size)
    self.h = Handle(self.c)
    _, self.valid = self.h.reprojection_error(self.x)
    self.n = int(self.valid.sum())

  def values(self, table):
    return et.make(table, self.n)

  def plant(self, e):
    """full inlier set, then the table with e on the valid slots (NaN elsewhere); returns the [C,F,B,P] table"""
    self.h.set_inliers(None)
    t = et.plant(self.valid, e)
    self.h.debug_set_error_table(self.x, t)
    return t


@pytest.fixture(scope="module")
def case():
  made = {}

  def get(name):
    if name not in made:
      made[name] = Case(name)
    return made[name]

  yield get
  for cs in made.values():
    cs.h.close()


def raw_stats(h, x, ranks, inliers_only=False):
  """mcba_error_stats as the C ABI has it: (values, n, sum_sq)"""
  ranks = np.ascontiguousarray(ranks, dtype=np.int64)
  x = np.ascontiguousarray(x, dtype=np.float64)
  vals = np.full(ranks.size, np.nan)
  n, ssq = C.c_int64(-1), C.c_double(np.nan)
  dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
  rc = h.lib.mcba_error_stats(h.h, dp(x), int(inliers_only), int(ranks.size),
                              ranks.ctypes.data_as(C.POINTER(C.c_int64)) if ranks.size else None, dp(vals) if ranks.size else None,
                              C.byref(n), C.byref(ssq))
  if rc != 0:
    raise McbaError(h.lib.mcba_last_error().decode())
  return vals, n.value, ssq.value


def quantiles_of(e, q):
  with np.errstate(invalid="ignore"):      # (inf - inf next to +inf: NaN is the expected value)
    return np.quantile(e, q)


def same_bits(got, want):
  """bit for bit, NaN == NaN"""
  got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
  nan = np.isnan(want)
  return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == want[~nan].tobytes()


def sum_sq_reference(e):
  """(kind, reference) of the sum of squares: finite, normal squares -> math.fsum; otherwise numpy's own sum, for its class"""
  with np.errstate(over="ignore", under="ignore"):
    sq = np.square(e)
  if np.isfinite(sq).all() and (sq >= et.DBL_MIN).all():
    return "fsum", math.fsum(sq)
  ref = float(sq.sum())
  return ("inf" if np.isinf(ref) else "0" if ref == 0 else "finite"), ref


def check_sum_sq(got, reference, what):
  """math.fsum to 1e-12 relative (the project's tolerance for these sums); otherwise numpy's class: both inf, or both 0"""
  kind, ref = reference
  if kind == "fsum":
    assert abs(got - ref) <= 1e-12 * ref, (what, got, ref)
  else:
    assert np.isinf(ref) == np.isinf(got) and (ref == 0) == (got == 0) and not np.isnan(got), (what, got, ref)
  return kind


def rms_of(e):
  with np.errstate(under="ignore"):
    return math.sqrt(math.fsum(np.square(e)) / e.size) if e.size else 0.0


def describe(cs, table, e):
  return f"[outlier statistics] {cs.name:<10} {table:<11} n={e.size:<6} slots={cs.valid.size:<6} tie groups={len(et.tie_groups(e)):<5}"


@cases
def test_order_statistics(case, rig, table):
  """raw mcba_error_stats: every rank list of error_tables.rank_lists == np.sort(e)[ranks], n and the sum of squares"""
  cs = case(rig)
  e = cs.values(table)
  cs.plant(e)
  lists = et.rank_lists(e, np.random.default_rng(7))
  nsel, sums = set(), sum_sq_reference(e)
  for ranks in lists:
    vals, n, ssq = raw_stats(cs.h, cs.x, ranks)
    assert n == e.size
    assert vals.tobytes() == et.order_statistics(e, ranks).tobytes(), (ranks, vals, et.order_statistics(e, ranks))
    kind = check_sum_sq(ssq, sums, ranks)
    nsel.add(et.distinct_selections(ranks))
  _, n, ssq = raw_stats(cs.h, cs.x, [])       # (no selection: the sums alone)
  assert n == e.size
  check_sum_sq(ssq, sums, "no ranks")
  if e.size >= 40:
    assert set(et.SELECTION_COUNTS) <= nsel
  print(f"{describe(cs, table, e)} calls={len(lists)} distinct selections per call={sorted(nsel)} sum_sq against {kind}")


@cases
def test_python_quantiles(case, rig, table):
  """Handle.error_stats == np.quantile at ten points, over all valid points and over the inliers of a planted rejection"""
  cs = case(rig)
  e = cs.values(table)
  t = cs.plant(e)
  with np.errstate(invalid="ignore"):      # (the host lerp next to +inf warns as numpy's own does)
    mse, rms, q, n = cs.h.error_stats(cs.x, quantiles=QUANTILES)
  assert n == e.size
  assert same_bits(q, quantiles_of(e, QUANTILES)), (q, quantiles_of(e, QUANTILES))
  kind = check_sum_sq(mse * n, sum_sq_reference(e), "mse")
  thr = np.nextafter(np.sort(e)[e.size // 2], np.inf)          # keeps the median's tie group: never an empty inlier set
  mask = (t < thr) & cs.valid
  assert cs.h.reject_outliers(cs.x, thr) == (int(mask.sum()), e.size)
  ei = t[mask]
  with np.errstate(invalid="ignore"):
    _, _, qi, ni = cs.h.error_stats(cs.x, quantiles=QUANTILES, inliers_only=True)
  assert ni == ei.size and ni >= 1
  assert same_bits(qi, quantiles_of(ei, QUANTILES)), (qi, quantiles_of(ei, QUANTILES))
  print(f"{describe(cs, table, e)} quantiles={len(QUANTILES)} NaN quantiles={int(np.isnan(q).sum())} inliers={ni} mse against {kind}")


@finite_cases
def test_c_quantiles(case, rig, table):
  """mcba_adjust_outliers(num_adjustments = 0), the report alone: five quantiles == np.quantile, counts exact, both RMS to 1e-12,
  after a planted rejection"""
  cs = case(rig)
  e = cs.values(table)
  t = cs.plant(e)
  thr = np.nextafter(np.sort(e)[(3 * e.size) // 4], np.inf)
  mask = (t < thr) & cs.valid
  assert cs.h.reject_outliers(cs.x, thr) == (int(mask.sum()), e.size)
  x, rounds, out_mask = cs.h.adjust_outliers(cs.x, num_adjustments=0)
  assert len(rounds) == 1 and np.array_equal(x, cs.x) and np.array_equal(out_mask, mask)
  r = rounds[0]
  assert same_bits(r.quantiles, quantiles_of(e, FIVE)), (r.quantiles, quantiles_of(e, FIVE))
  assert (r.n, r.n_inliers) == (e.size, int(mask.sum()))
  for got, ref in ((r.rms, rms_of(e)), (r.rms_inliers, rms_of(t[mask]))):
    assert abs(got - ref) <= 1e-12 * ref, (got, ref)
  print(f"{describe(cs, table, e)} report: n={r.n} inliers={r.n_inliers} rms={r.rms:.6g} rms_inliers={r.rms_inliers:.6g}")


def thresholds_of(e):
  s = np.sort(e)
  groups = et.tie_groups(e)
  groups = [g for g in groups if np.isfinite(s[g[0]])]
  inner = [g for g in groups if g[0] > 0] or groups                 # a group with smaller values below it, if there is one
  v = s[max(inner, key=lambda g: g[1] - g[0])[0]] if len(inner) else s[e.size // 3]
  return [("tie group", v), ("next after it", np.nextafter(v, np.inf)), ("median", s[e.size // 2]), ("zero", 0.0),
          ("smallest subnormal", 5e-324), ("+inf", np.inf)]


@cases
def test_rejection_thresholds(case, rig, table):
  """k_reject: get_inliers() == (table < thr) & valid, the returned counts and n_residuals, with the threshold on a tie group (strict
  <: the whole group goes), one ulp above it (it stays), the median, 0 (empty set), the smallest subnormal and +inf"""
  cs = case(rig)
  e = cs.values(table)
  t = cs.plant(e)
  kept = []
  for what, thr in thresholds_of(e):
    with np.errstate(invalid="ignore"):
      mask = (t < thr) & cs.valid
    n_in, n_valid = cs.h.reject_outliers(cs.x, thr)
    got = cs.h.get_inliers()
    assert np.array_equal(got, mask), (what, thr, int(got.sum()), int(mask.sum()))
    assert (n_in, n_valid) == (int(mask.sum()), e.size), (what, thr)
    assert cs.h.n_residuals == 2 * int(mask.sum()), (what, thr)
    if thr == 0.0:
      assert cs.h.n_residuals == 0 and cs.h.residuals(cs.x).size == 0          # the empty set (no solve on it)
    if thr == np.inf:
      assert n_in == int(np.isfinite(e).sum())
    kept.append(n_in)
  assert kept[1] > kept[0]                                                      # the group the strict < dropped is back
  print(f"{describe(cs, table, e)} inliers at [tie group, next after, median, 0, 5e-324, +inf]={kept}")


def test_state_after_rejection_equals_set_inliers(case):
  """After a rejection that leaves 0, 1, 63, 64, 65, 128, 129 and all points in the views of tiny_bigboard, residuals and normal
  equations are byte-identical to those of a fresh handle given the same mask through set_inliers (both routes feed the same
  deterministic kernels from the same view counts), and match the oracle with that mask."""
  cs = case("bigboard21")
  counts = [0, 1, 63, 64, 65, 128, 129, et.ALL]
  e, ks = et.view_edges(cs.valid, counts)
  t = cs.plant(e)
  mask = (t < 1.0) & cs.valid
  per_view = mask.sum(axis=-1)
  npts = cs.valid.sum(axis=-1)
  assert np.array_equal(per_view[ks >= 0], np.minimum(ks, npts)[ks >= 0])
  realised = {int(k) for k in per_view[(ks >= 0) & (ks < npts)]} | ({et.ALL} if ((ks >= 0) & (ks >= npts)).any() else set())
  assert realised >= set(counts)
  assert cs.h.reject_outliers(cs.x, 1.0) == (int(mask.sum()), e.size)
  assert np.array_equal(cs.h.get_inliers(), mask)
  oc = oracle(cs.rig).copy(inlier_mask=mask)
  with Handle(cs.c) as fresh:
    fresh.set_inliers(mask)
    for i, x in enumerate((cs.x, cs.x2)):
      if i == 1:      # another x: the rejection's state must not depend on the planted table any more
        assert cs.h.n_residuals == fresh.n_residuals == 2 * int(mask.sum())
      r, rf = cs.h.residuals(x), fresh.residuals(x)
      assert r.tobytes() == rf.tobytes()
      ro = oc.evaluate(x)
      assert r.shape == ro.shape and np.abs(r - ro).max() < 1e-9
      cost, g, diag = cs.h.normal_equations(x)
      H = cs.h.dense_hessian()
      cost_f, g_f, diag_f = fresh.normal_equations(x)
      H_f = fresh.dense_hessian()
      assert cost == cost_f and g.tobytes() == g_f.tobytes() and diag.tobytes() == diag_f.tobytes() and H.tobytes() == H_f.tobytes()
      assert abs(cost - 0.5 * ro @ ro) <= 1e-12 * 0.5 * ro @ ro
  print(f"[outlier statistics] {cs.name} view_edges: views={int((ks >= 0).sum())} per-view inlier counts realised={sorted(realised, key=str)} "
        f"inliers={int(mask.sum())} of {e.size}: residuals, cost, gradient, diagonal, H at two x byte-identical to set_inliers")


@pytest.mark.parametrize("rig", ["tiny", "tiny_edge"])
def test_hook_poisons_nothing(case, rig):
  """a planted table serves calls at its own x only: statistics at another x are those of the true table there, and the first x
  then gets its true table back"""
  cs = case(rig)
  e = cs.values("ties")
  cs.plant(e)
  ranks = [0, e.size // 2, e.size - 1, e.size // 3]
  assert raw_stats(cs.h, cs.x, ranks)[0].tobytes() == et.order_statistics(e, ranks).tobytes()
  for x in (cs.x2, cs.x):
    err, valid = cs.h.reprojection_error(x)
    assert np.array_equal(valid, cs.valid)
    true = err[valid]
    vals, n, ssq = raw_stats(cs.h, x, ranks)
    assert n == true.size and vals.tobytes() == et.order_statistics(true, ranks).tobytes()
    assert vals.tobytes() != et.order_statistics(e, ranks).tobytes()
    check_sum_sq(ssq, sum_sq_reference(true), "true table")
    _, _, q, _ = cs.h.error_stats(x, quantiles=QUANTILES)
    assert same_bits(q, quantiles_of(true, QUANTILES))
  print(f"[outlier statistics] {cs.name} planted at x, asked at x2 and again at x: the true tables answer")


def test_refusals(case):
  """NaN and -0.0 at a valid slot, and a frame-sharded handle, are refused with their messages and leave the handle working; a rank
  on a handle without a valid point is the existing rank error"""
  cs = case("tiny_edge")
  e = cs.values("smooth")
  first = tuple(np.argwhere(cs.valid)[0])
  last = tuple(np.argwhere(cs.valid)[-1])
  for slot, bad, message in ((first, np.nan, "error table: NaN at valid entry"), (last, -0.0, "error table: negative-signed value"),
                             (first, -1.0, "error table: negative-signed value")):
    cs.plant(e)
    e2 = cs.values("low20")
    t = et.plant(cs.valid, e2)
    t[slot] = bad
    with pytest.raises(McbaError, match=message):
      cs.h.debug_set_error_table(cs.x, t)
    # nothing of the refused table was written (the table planted before still answers), and the next plant works
    ranks = [0, 1, e.size // 2, e.size - 1]
    assert raw_stats(cs.h, cs.x, ranks)[0].tobytes() == et.order_statistics(e, ranks).tobytes()
    cs.plant(e2)
    assert raw_stats(cs.h, cs.x, ranks)[0].tobytes() == et.order_statistics(e2, ranks).tobytes()
  F = cs.valid.shape[1]
  with Handle(cs.c, frame_range=(0, F // 2)) as shard:
    with pytest.raises(McbaError, match="error table: a frame-sharded handle is not supported"):
      shard.debug_set_error_table(cs.x, et.plant(cs.valid, e))
  empty = case("tiny_n0")
  assert empty.n == 0
  with pytest.raises(McbaError, match="rank out of range"):
    raw_stats(empty.h, empty.x, [0])
  vals, n, ssq = raw_stats(empty.h, empty.x, [])
  assert (n, ssq) == (0, 0.0)
  mse, rms, q, n = empty.h.error_stats(empty.x)                                  # the reference's single zero
  assert (mse, rms, n) == (0.0, 0.0, 1) and q.tobytes() == np.zeros(5).tobytes()
  print("[outlier statistics] refused: NaN, -0.0, -1.0 at a valid slot, a frame shard, a rank on a handle without a valid point")


@pytest.mark.parametrize("rig,table", [("tiny", "ties"), ("bigboard81", "ties"), ("bigboard81", "digit_edges")])
def test_determinism(case, rig, table):
  """the same calls twice: the same bytes (integer atomics only)"""
  cs = case(rig)
  e = cs.values(table)
  runs = []
  for _ in range(2):
    cs.plant(e)
    lists = et.rank_lists(e, np.random.default_rng(7))[:12]
    vals = b"".join(raw_stats(cs.h, cs.x, ranks)[0].tobytes() for ranks in lists)
    ssq = raw_stats(cs.h, cs.x, [])[2]
    counts = cs.h.reject_outliers(cs.x, np.sort(e)[e.size // 2])
    runs.append((vals, np.float64(ssq).tobytes(), counts, cs.h.get_inliers().tobytes(), cs.h.n_residuals))
  assert runs[0] == runs[1]
  print(f"{describe(cs, table, e)} two runs: values, sum of squares, counts, mask identical")
