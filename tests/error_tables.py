"""TEST INFRASTRUCTURE: planted per-point error tables for the device order statistics (k_selm_*) and the rejection (k_reject), and
the rank lists the selection is asked for.

The radix select of mcba_error_stats walks the IEEE bit pattern of the errors in six passes: digits of 11, 11, 11, 11, 11 and 9 bits
at shifts 53, 42, 31, 20, 9 and 0 (the first digit holds the sign bit, so a non-negative double reaches 0 .. 1023 there).  Every
generator below is named for the property of that walk it aims at and returns `n` float64 values >= +0 (never NaN, never -0.0) for
the valid slots of a table, in the C order of the validity mask: `plant(valid, values)` makes the [C,F,B,P] table.  All are seeded:
the same (name, n, seed) gives the same bytes.  tests/test_error_tables_host.py checks each generator's property on the CPU."""
import numpy as np

SHIFTS = (53, 42, 31, 20, 9, 0)
BITS = (11, 11, 11, 11, 11, 9)
SEL_MAX = 6                      # selections per batch of select_ranks_multi
DBL_MIN = np.finfo(np.float64).tiny
ONE_KEY = np.uint64(0x3FF0000000000000)     # 1.0: its low 20 bits are zero
INF_KEY = np.uint64(0x7FF0000000000000)
# digits a pass is steered to: first / last bin of a lane's 32-bin range in k_selm_pick (lanes 0, 1 and 63), and of the 16 lanes the
# 512-bin last pass leaves populated
DIGIT_EDGES = (0, 31, 32, 63, 2016, 2047)
LAST_DIGIT_EDGES = (0, 31, 32, 511)
FIRST_DIGIT_EDGES = (0, 31, 32, 63, 1023)   # what a non-negative double reaches; 1023 = the top binade and +inf


def keys_of(e):
  return np.ascontiguousarray(e, dtype=np.float64).view(np.uint64)


def from_keys(k):
  return np.ascontiguousarray(k, dtype=np.uint64).view(np.float64)


def digits(e, p):
  """digit of pass p of every value"""
  return ((keys_of(e) >> np.uint64(SHIFTS[p])) & np.uint64((1 << BITS[p]) - 1)).astype(np.int64)


def smooth(n, rng):
  """the control: distinct values of a smooth distribution, like reprojection errors of a noisy rig"""
  return rng.gamma(2.0, 0.3, size=n)


def zeros(n, rng):
  """noise-free data: one tie group of +0.0"""
  return np.zeros(n)


def constant(n, rng):
  return np.full(n, 0.7310585786300049)


def ties(n, rng):
  """tie groups of multiplicity 40, 39, .. 1 (then again, on fresh values, while n lasts) in random positions"""
  mult = np.resize(np.arange(40, 0, -1), max(1, 40 * (n // 820 + 1)))
  vals = np.sort(rng.uniform(0.05, 3.0, size=mult.size))
  out = np.repeat(vals[rng.permutation(mult.size)], mult)[:n]
  return out[rng.permutation(out.size)]


def two_valued(n, rng):
  out = np.where(rng.random(n) < 0.7, 0.25, 3.0)
  if n >= 2:
    out[:2] = (3.0, 0.25)
  return out


def low9(n, rng):
  """keys that differ in the 9 bits of the last pass only"""
  return from_keys(ONE_KEY + rng.integers(0, 512, size=n).astype(np.uint64))


def low20(n, rng):
  """keys that differ in the last two passes only"""
  return from_keys(ONE_KEY + rng.integers(0, 1 << 20, size=n).astype(np.uint64))


def subnormal(n, rng):
  """+0.0, the first 300 subnormals and DBL_MIN"""
  pool = np.concatenate([np.zeros(60, dtype=np.uint64), np.arange(1, 301, dtype=np.uint64), np.repeat(keys_of([DBL_MIN]), 20)])
  return from_keys(pool[rng.integers(0, pool.size, size=n)])


def wide(n, rng):
  """10^U(-300, 300) with a few +inf and a few zeros"""
  out = 10.0 ** rng.uniform(-300.0, 300.0, size=n)
  few = min(4, n // 3)
  where = rng.permutation(n)[:2 * few]
  out[where[:few]] = np.inf
  out[where[few:]] = 0.0
  return out


def digit_edges(n, rng):
  """every pass's digit on an edge value; the combinations are drawn at random, +inf and 0.0 ride along"""
  pick = lambda edges: np.asarray(edges, dtype=np.uint64)[rng.integers(0, len(edges), size=n)]
  d = [pick(FIRST_DIGIT_EDGES)] + [pick(DIGIT_EDGES) for _ in range(4)] + [pick(LAST_DIGIT_EDGES)]
  # first digit 1023 with bit 52 set is exponent 0x7FF: +inf when the rest is zero, NaN otherwise -- keep those in the top binade
  top = d[0] == 1023
  d[1] = np.where(top & (d[1] >= 1024), d[1] - np.uint64(1984), d[1])      # 2016 -> 32, 2047 -> 63
  key = np.zeros(n, dtype=np.uint64)
  for p in range(6):
    key |= d[p] << np.uint64(SHIFTS[p])
  few = min(3, n // 3)
  where = rng.permutation(n)[:2 * few]
  key[where[:few]] = INF_KEY
  key[where[few:]] = 0
  return from_keys(key)


GENERATORS = dict(smooth=smooth, zeros=zeros, constant=constant, ties=ties, two_valued=two_valued, low9=low9, low20=low20,
                  subnormal=subnormal, wide=wide, digit_edges=digit_edges)
TABLES = list(GENERATORS)
LARGE_TABLES = ["smooth", "ties", "low9", "digit_edges"]    # what the two large rigs run


def make(name, n, seed=0):
  """n values of the named table"""
  rng = np.random.default_rng([seed, TABLES.index(name), n])
  e = np.ascontiguousarray(GENERATORS[name](n, rng), dtype=np.float64)
  assert e.shape == (n,) and not np.isnan(e).any() and not np.signbit(e).any(), name
  return e


ALL = "all"


def view_edges(valid, counts):
  """0.5 on the first k valid points of each view and 2.0 on the rest, k cycling through `counts` over the views that hold a valid
  point (ALL = every point of the view; a view with fewer than k points is all 0.5): a threshold of 1.0 leaves min(k, points)
  inliers in the view.  Returns (values for the valid slots, k of every view [C,F,B] with -1 on views without a valid point)."""
  valid = np.asarray(valid, dtype=bool)
  table = np.zeros(valid.shape)
  ks = np.full(valid.shape[:3], -1, dtype=np.int64)
  i = 0
  for view in np.ndindex(*valid.shape[:3]):
    idx = np.flatnonzero(valid[view])
    if idx.size == 0:
      continue
    k = counts[i % len(counts)]
    k = idx.size if k == ALL else int(k)
    i += 1
    ks[view] = k
    table[view][idx[:k]] = 0.5
    table[view][idx[k:]] = 2.0
  return table[valid], ks


def plant(valid, values, fill=np.nan):
  """[C,F,B,P] table with `values` on the valid slots; `fill` (NaN: the hook must ignore it) on the others"""
  valid = np.asarray(valid, dtype=bool)
  table = np.full(valid.shape, fill, dtype=np.float64)
  table[valid] = values
  return table


def order_statistics(e, ranks):
  return np.sort(np.asarray(e, dtype=np.float64))[np.asarray(ranks, dtype=np.int64)]


def tie_groups(e):
  """(first rank, last rank) of every run of two or more equal values in ascending order"""
  s = np.sort(np.asarray(e, dtype=np.float64))
  if s.size == 0:
    return np.zeros((0, 2), dtype=np.int64)
  start = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
  end = np.concatenate([start[1:], [s.size]]) - 1
  keep = end > start
  return np.stack([start[keep], end[keep]], axis=1)


def distinct_selections(ranks):
  """number of selections error_stats_impl makes for a rank list: a rank equal to an earlier selection, or one above it, shares it"""
  sel = []
  for r in ranks:
    if not any(s == r or s + 1 == r for s in sel):
      sel.append(int(r))
  return len(sel)


SELECTION_COUNTS = (1, 2, 3, 4, 5, 6, 7, 12, 13)     # below, at and above one batch; two batches exactly; two and one


def rank_lists(e, rng):
  """Rank lists (each a list of ints in [0, n)) for one table:
    * the pool -- ranks 0, 1, 2, n - 3 .. n - 1, n // 2, the first and last rank of every tie group (64 groups at the most, evenly
      picked) and 40 random ranks -- cut into lists of length 1 .. 13 in turn (a pool of fewer than 91 ranks is walked again);
    * for each k of SELECTION_COUNTS a list of k pool ranks no two of which are equal or adjacent (k distinct selections exactly),
      as far as n allows, in random order; for k = 6, 7, 12 and 13 also with every rank followed by the one above it (2 k ranks, k
      selections: the sharing of the next value in the first, second and third batch);
    * lists with repeated ranks, and adjacent pairs as (r, r + 1) and as (r + 1, r): inside a tie group, across its upper edge, at
      both ends of the table."""
  e = np.asarray(e, dtype=np.float64)
  n = e.size
  if n == 0:
    return []
  clip = lambda r: int(min(max(r, 0), n - 1))
  groups = tie_groups(e)
  if len(groups) > 64:
    groups = groups[np.linspace(0, len(groups) - 1, 64).astype(np.int64)]
  pool = [clip(r) for r in (0, 1, 2, n - 3, n - 2, n - 1, n // 2)]
  pool += [int(r) for g in groups for r in g]
  pool += [int(r) for r in rng.integers(0, n, size=40)]
  lists, i, length = [], 0, 1
  while i < max(len(pool), 91):            # (a short pool is walked again: every length 1 .. 13 occurs)
    lists.append([pool[j % len(pool)] for j in range(i, i + length)])
    i += length
    length = length % 13 + 1
  apart = []
  for r in sorted(set(pool) | set(int(r) for r in rng.integers(0, n, size=40))):
    if not apart or r >= apart[-1] + 2:
      apart.append(r)
  for k in SELECTION_COUNTS:
    if k <= len(apart):
      lists.append([int(r) for r in rng.permutation(apart)[:k]])
  below = [r for r in apart if r + 1 < n]
  for k in (6, 7, 12, 13):                     # ... and each followed by its successor: the shared (k+1)-th value of every batch
    if k <= len(below):
      lists.append([int(r) + d for r in rng.permutation(below)[:k] for d in (0, 1)])
  pairs =[0, n - 2, n // 2]
  for first, last in groups[:6]:
    pairs += [first, last - 1, last]           # inside the group (twice) and across its upper edge
  for r in dict.fromkeys(clip(r) for r in pairs):
    if r + 1 < n:
      lists += [[r, r + 1], [r + 1, r], [r, r, r + 1, r, r + 1], [r + 1, r + 1, r, r]]
    else:
      lists.append([r, r])
  return lists
