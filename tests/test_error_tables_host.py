"""CPU: every planted error table of tests/error_tables.py has the property it is named for, and the rank lists reach every
distinct-selection count -- the preconditions of tests/test_gpu_outlier_statistics.py, checked without a GPU."""
import numpy as np
import pytest

import error_tables as et
from multical_amd import synthetic

SIZES = [1, 2, 3, 5, 478, 972, 4001, 70000]     # 478: valid points of the `tiny` rig


def counts_of(e):
  return np.unique(e, return_counts=True)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", et.TABLES)
def test_every_table_is_seeded_and_in_the_select_premise(name, n):
  e = et.make(name, n)
  assert e.dtype == np.float64 and e.shape == (n,)
  assert not np.isnan(e).any() and not np.signbit(e).any()          # err >= +0: the bit pattern is monotone
  assert e.tobytes() == et.make(name, n).tobytes()
  assert n < 100 or name in ("zeros", "constant") or e.tobytes() != et.make(name, n, seed=1).tobytes()
  k = et.keys_of(np.sort(e))
  assert np.all(k[1:] >= k[:-1])


def test_smooth_is_distinct_and_finite():
  e = et.make("smooth", 4001)
  assert np.unique(e).size == e.size and np.isfinite(e).all() and (e > 0).all()
  assert np.all(np.square(e) >= et.DBL_MIN)


def test_zeros_constant_two_valued():
  assert et.make("zeros", 972).tobytes() == np.zeros(972).tobytes()       # +0.0, not -0.0
  assert np.unique(et.make("constant", 972)).size == 1 and et.make("constant", 5)[0] > 0
  for n in (2, 3, 972):
    v, c = counts_of(et.make("two_valued", n))
    assert list(v) == [0.25, 3.0] and c.min() >= 1


@pytest.mark.parametrize("n", [478, 897, 972, 70000])
def test_ties_multiplicities(n):
  v, c = counts_of(et.make("ties", n))
  assert (c >= 8).sum() >= 10
  assert c.max() == 40 and v.size >= 13
  assert c.min() <= 2 or n < 820                                           # single values and pairs next to the large groups
  g = et.tie_groups(et.make("ties", n))
  assert len(g) == (c >= 2).sum() and np.all(g[:, 1] - g[:, 0] + 1 == c[c >= 2])


@pytest.mark.parametrize("n", [478, 897, 70000])
def test_low9_and_low20_share_their_high_bits(n):
  k = et.keys_of(et.make("low9", n))
  assert np.unique(k >> np.uint64(9)).size == 1 and np.unique(k).size >= 256          # top 55 bits shared
  for p in range(5):
    assert np.unique(et.digits(et.make("low9", n), p)).size == 1
  k = et.keys_of(et.make("low20", n))
  assert np.unique(k >> np.uint64(20)).size == 1
  assert np.unique(et.digits(et.make("low20", n), 4)).size >= 256 and np.unique(k).size >= 0.9 * min(n, 1 << 18)


def test_subnormal_table():
  e = et.make("subnormal", 4001)
  assert (e == 0).sum() >= 100 and (e == et.DBL_MIN).sum() >= 20
  sub = e[(e > 0) & (e < et.DBL_MIN)]
  assert np.unique(sub).size >= 250 and et.keys_of(sub).max() <= 300
  assert np.all(np.square(e) == 0)                                          # sum of squares underflows to exactly 0


def test_wide_table():
  e = et.make("wide", 972)
  assert np.isinf(e).sum() == 4 and (e == 0).sum() == 4
  f = e[np.isfinite(e) & (e > 0)]
  assert f.min() < 1e-250 and f.max() > 1e250
  assert np.unique(et.digits(e, 0)).size >= 500                             # the first pass alone nearly separates them
  assert np.isinf(et.make("wide", 3)).sum() == 1


@pytest.mark.parametrize("n", [897, 70000])
def test_digit_edges_touch_the_named_bins(n):
  e = et.make("digit_edges", n)
  assert np.isinf(e).sum() == 3 and (e == 0).sum() >= 3      # (all six digits 0 is 0.0 as well)
  for p in range(6):
    want = et.FIRST_DIGIT_EDGES if p == 0 else et.LAST_DIGIT_EDGES if p == 5 else et.DIGIT_EDGES
    hist = np.bincount(et.digits(e, p), minlength=1 << et.BITS[p])
    assert np.all(hist[list(want)] > 0), (p, hist[list(want)])
    extra = {1024} if p == 1 else set()                                    # (+inf: exponent bit 52)
    assert set(np.flatnonzero(hist)) <= set(want) | extra, p
  top = e[et.digits(e, 0) == 1023]
  assert np.isfinite(top).sum() > 0 and np.isinf(top).sum() == 3            # the top binade and +inf


@pytest.mark.parametrize("name,frames", [("tiny", None), ("tiny_bigboard", 21)])
def test_view_edges_realise_the_counts(name, frames):
  rig = synthetic.make_rig(name, frames=frames)
  valid = rig.valid
  counts = [0, 1, 63, 64, 65, 128, 129, et.ALL]
  values, ks = et.view_edges(valid, counts)
  assert values.shape == (int(valid.sum()),) and set(np.unique(values)) <= {0.5, 2.0}
  table = et.plant(valid, values)
  assert np.isnan(table[~valid]).all()
  kept = ((table < 1.0) & valid).sum(axis=-1)
  npts = valid.sum(axis=-1)
  seen = set()
  for view in np.ndindex(*ks.shape):
    if npts[view] == 0:
      assert ks[view] == -1
      continue
    assert kept[view] == min(ks[view], npts[view])
    # the valid points behind the first k are the rejected ones
    idx = np.flatnonzero(valid[view])
    assert np.all(table[view][idx[:kept[view]]] == 0.5) and np.all(table[view][idx[kept[view]:]] == 2.0)
    if ks[view] <= npts[view]:
      seen.add(int(kept[view]) if ks[view] < npts[view] else et.ALL)
  if name == "tiny_bigboard":      # 816-point views hold every count
    assert seen == {0, 1, 63, 64, 65, 128, 129, et.ALL}


@pytest.mark.parametrize("name", et.TABLES)
@pytest.mark.parametrize("n", [1, 2, 3, 5, 897, 70000])
def test_rank_lists_cover_the_selection_counts(name, n):
  e = et.make(name, n)
  lists = et.rank_lists(e, np.random.default_rng(3))
  assert lists and all(len(l) >= 1 and all(0 <= r < n for r in l) for l in lists)
  assert lists == et.rank_lists(e, np.random.default_rng(3))
  got = {et.distinct_selections(l) for l in lists}
  if n >= 40:
    assert set(et.SELECTION_COUNTS) <= got
    assert {len(l) for l in lists} >= set(range(1, 14))
    flat = {r for l in lists for r in l}
    assert {0, 1, 2, n - 3, n - 2, n - 1, n // 2} <= flat
    groups = et.tie_groups(e)
    if len(groups) <= 64:
      assert all(first in flat and last in flat for first, last in groups)
    else:
      assert sum(first in flat and last in flat for first, last in groups) >= 64
    assert any(len(l) == 2 and l[1] == l[0] + 1 for l in lists) and any(len(l) == 2 and l[0] == l[1] + 1 for l in lists)
    assert any(len(set(l)) < len(l) for l in lists)
  else:
    assert got >= set(range(1, (n + 1) // 2 + 1))
  ref = np.sort(e)
  for l in lists[:5]:
    assert et.order_statistics(e, l).tobytes() == ref[l].tobytes()


def test_distinct_selections_follow_the_sharing_rule():
  assert et.distinct_selections([5, 6]) == 1 and et.distinct_selections([6, 5]) == 2
  assert et.distinct_selections([5, 6, 7]) == 2 and et.distinct_selections([5, 5, 6, 5]) == 1
  assert et.distinct_selections([0, 2, 4, 6, 8, 10, 12]) == 7
