"""The grid-stride rounds of every capped-grid kernel of the handle-less families, on small inputs.

k_point_ops, k_undistort_map, k_remap_cubic (16 instantiations), k_warp_points, k_triangulate, k_projection_uncertainty, k_projdiff_map,
k_reconstruction_uncertainty<4|8> and k_reconstruction_pairs<4|8> walk their work in a grid-stride loop whose second round needs
2^20 workgroups' worth of work (2048 for k_warp_points) at the built-in caps.  mcba_debug_set_grid_cap lowers the cap, so that a
workgroup takes a second and a tenth tile here: it re-derives slice, tile and job from the tile index, re-stages camera and job
records of another width over the old ones in LDS, and reuses the MFMA stage that the round before left its partial sums in.

Every case runs its call once with the built-in cap and checks that result against the g++ build of the same header exactly as the
family's own test file does (the same helpers, the same tolerances).  Then it runs the call again under the caps 1, 2, 3,
workgroups - 1 and workgroups and asserts that EVERY OUTPUT ARRAY IS BYTE-IDENTICAL to the first run: the result of an item does not
depend on the workgroup that computed it, and every sum has a fixed order, so no tolerance is involved.  After every call
mcba_debug_last_capped_grid must report min(cap, workgroups of the call), with the workgroup count worked out here from the shapes:
a cap that did not reach the launch fails the test.  Before every capped call an uncapped call of the same shapes on other values
fills the cached output buffers, so that a tile which a capped launch leaves out cannot show the right bytes of the call before."""
import functools

import numpy as np
import pytest

from multical_amd import _lib, compare, correction, reconstruction, triangulate, uncertainty, undistort

import correction_host_lib as ch
import length_uncertainty_host_lib as ll
import projdiff_host_lib as pl
import reconstruction_uncertainty_host_lib as rl
import triangulate_host_lib as th
import uncertainty_host_lib as ul
import undistort_host_lib as uh
import undistort_reference as ref
import test_gpu_length_uncertainty as t_length
import test_gpu_projection_diff as t_projdiff
import test_gpu_projection_uncertainty as t_uncertainty
import test_gpu_reconstruction_uncertainty as t_recon
import test_gpu_triangulate as t_triangulate

pytestmark = pytest.mark.gpu

CAMERAS = uh.fixture_cameras()
W, H = uh.IMAGE_SIZE
THREADS = 256                                   # work items of a workgroup of the point, map, flat-remap, warp, query kernels
TILE_W, TILE_H = 256, 4                         # the row path of k_remap_cubic
ROW_SIZE, FLAT_SIZE = (516, 5), (57, 5)         # three x-tiles (the last holds one group of 4) x two y-tiles (the last holds one row); Wd % 4 != 0


def ceil_div(a, b):
  return -(-a // b)


@pytest.fixture
def grid_cap():
  """mcba_debug_set_grid_cap for the test; the built-in caps are back after it"""
  yield _lib.set_grid_cap
  _lib.set_grid_cap(0)


def caps_of(workgroups):
  """1: one workgroup sees every tile and every job change; 2, 3: workgroups alternate between jobs and frames; workgroups - 1:
  workgroup 0 alone takes a second round; workgroups: today's launch"""
  return sorted({1, 2, 3, workgroups - 1, workgroups} - {0})


def blob(arrays):
  return [np.ascontiguousarray(a).tobytes() for a in arrays]


def check_rounds(grid_cap, label, workgroups, call, arrays_of, check_against_host, decoy):
  """call(): the device call; arrays_of(result): its output arrays; check_against_host(result): the family's own comparison;
  decoy(): a call of the same shapes on other values.  The output buffers of a call come back from the library's resource cache
  with the bytes the call before left in them, and they are not cleared: a tile that a capped call never wrote would still hold the
  right answer of the call before.  So an uncapped decoy call goes before every capped one, and what a capped call leaves out is
  the decoy's."""
  assert workgroups >= 2, label
  grid_cap(0)
  base = call()
  assert _lib.last_capped_grid() == workgroups, (label, "built-in cap")
  check_against_host(base)
  want = blob(arrays_of(base))
  for cap in caps_of(workgroups):
    grid_cap(0)
    other = blob(arrays_of(decoy()))
    assert [len(o) for o in other] == [len(w) for w in want] and other[0] != want[0], (label, "the decoy")
    grid_cap(cap)
    got = call()
    assert _lib.last_capped_grid() == min(cap, workgroups), (label, cap)
    for i, (g, w) in enumerate(zip(blob(arrays_of(got)), want)):
      same = g == w                                                  # (not in the assert: pytest would render both byte strings)
      assert same, f"{label}: output {i} under a grid cap of {cap} of {workgroups} workgroups differs from the uncapped call"
  grid_cap(0)
  assert caps_of(workgroups)[0] < workgroups
  return base


def test_the_cap_is_refused_when_negative_and_restored_by_zero(grid_cap):
  X = np.tile([[0.1, -0.05, 1.0]], (3 * THREADS, 1))
  with pytest.raises(_lib.McbaError, match="grid cap"):
    grid_cap(-1)
  undistort.project_points(CAMERAS[:1], X)
  assert _lib.last_capped_grid() == 3
  grid_cap(2)
  undistort.project_points(CAMERAS[:1], X)
  assert _lib.last_capped_grid() == 2
  grid_cap(0)
  undistort.project_points(CAMERAS[:1], X)
  assert _lib.last_capped_grid() == 3


# ---- k_point_ops, k_undistort_map ------------------------------------------------------------------------------------------------
def zoomed(cams, factor=0.5):
  return np.stack([uh.zoomed_out(c, factor) for c in cams])


def test_point_ops(grid_cap):
  """n = 1000 over all fixture cameras: four workgroups; project, and undistort with R and P"""
  n = 1000
  rng = np.random.default_rng(1100)
  of = rng.integers(0, len(CAMERAS), n).astype(np.int32)
  X = np.concatenate([rng.uniform(-0.3, 0.3, (n, 2)), np.ones((n, 1))], axis=1) * rng.uniform(0.5, 3.0, (n, 1))

  def project_matches_host(uv):
    assert np.abs(uv - uh.on_host(undistort.project_points, CAMERAS, X, of)).max() < 1e-9
  check_rounds(grid_cap, "project_points", ceil_div(n, THREADS), lambda: undistort.project_points(CAMERAS, X, of), lambda uv: [uv],
               project_matches_host, lambda: undistort.project_points(CAMERAS, X * [1.1, 0.9, 1.0], of))

  px = rng.uniform(0.0, 1.0, (n, 2)) * [W - 1, H - 1]
  fisheye = np.array([ref.is_fisheye(c) for c in CAMERAS])[of]
  px[fisheye & (np.arange(n) % 3 == 0)] = [5000.0, 4000.0]          # a fisheye camera cannot have produced this pixel
  kwargs = dict(R=np.stack([uh.small_rotation((1.0 + c, -2.0, 0.5 * c)) for c in range(len(CAMERAS))]), P=zoomed(CAMERAS))

  def undistort_matches_host(result):
    got, status = result
    want, want_status = uh.on_host(undistort.undistort_points, CAMERAS, px, of, **kwargs)
    assert np.array_equal(status, want_status)
    ok = status == undistort.UNDISTORT_OK
    assert np.isnan(got[~ok]).all() and np.abs(got[ok] - want[ok]).max() < 1e-9
    assert (~ok).any() and ok.sum() > 800
  check_rounds(grid_cap, "undistort_points", ceil_div(n, THREADS), lambda: undistort.undistort_points(CAMERAS, px, of, **kwargs),
               lambda r: list(r), undistort_matches_host, lambda: undistort.undistort_points(CAMERAS, px[::-1].copy(), of, **kwargs))


def test_undistort_map(grid_cap):
  """257 x 5 over all cameras: 41 workgroups, camera and row change inside a workgroup"""
  size = (257, 5)
  kwargs = dict(R=uh.small_rotation(), P=zoomed(CAMERAS, 0.8))

  def matches_host(got):
    want = uh.on_host(undistort.undistort_maps, CAMERAS, size, **kwargs)
    assert got.shape == (len(CAMERAS), size[1], size[0], 2) and got.dtype == np.float32
    assert uh.ulp_distance(got, want).max() <= 1
  check_rounds(grid_cap, "undistort_maps", ceil_div(len(CAMERAS) * size[0] * size[1], THREADS),
               lambda: undistort.undistort_maps(CAMERAS, size, **kwargs), lambda m: [m], matches_host,
               lambda: undistort.undistort_maps(CAMERAS, size, P=zoomed(CAMERAS, 0.6)))


# ---- k_remap_cubic: map-fed and fused, both formats x both channel counts, row path and flat path ----------------------------------
def remap_workgroups(slices, n_images, size):
  """slices: what the tile loop of the row path runs over (images; fused: cameras)"""
  wd, hd = size
  if wd % 4 == 0:
    return slices * ceil_div(hd, TILE_H) * ceil_div(wd, TILE_W)
  return ceil_div(ceil_div(n_images * hd * wd, 4), THREADS)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_remap_through_maps(grid_cap, dtype, channels):
  """five images over two maps, source 130 x 70, the edge coordinates planted: 30 tiles on the row path, 2 workgroups on the flat one"""
  hs, ws = 70, 130
  images = uh.noise_image(200 + channels, (5, hs, ws) + ((3,) if channels == 3 else ()), dtype)
  negative = (255 - images).astype(dtype)
  of = [1, 0, 1, 1, 0]
  for size in (ROW_SIZE, FLAT_SIZE):
    maps = uh.random_maps(300 + size[0], 2, size[1], size[0], hs, ws)

    def matches_host(got):
      want = uh.on_host(undistort.remap, images, maps, of, border=6.0)
      assert got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()
    check_rounds(grid_cap, f"remap {size}", remap_workgroups(5, 5, size), lambda: undistort.remap(images, maps, of, border=6.0),
                 lambda r: [r], matches_host, lambda: undistort.remap(negative, maps, of, border=77.0))


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_fused_remap(grid_cap, dtype, channels):
  """eleven images over the eight cameras, camera 2 without an image and camera 6 with three: 48 tiles on the row path (a workgroup
  meets the empty camera between two that have images), 4 workgroups on the flat one.  As in test_gpu_undistort.py the fused call is
  the map-fed one through the device's own maps byte for byte (the maps against the host build: test_undistort_map)"""
  n = len(CAMERAS) + 3
  of = (np.arange(n) * 5 % len(CAMERAS)).astype(np.int32)
  of[of == 2] = 6
  assert (of == 6).sum() == 3 and set(of) == set(range(len(CAMERAS))) - {2}
  images = uh.noise_image(400 + channels, (n, H, W) + ((3,) if channels == 3 else ()), dtype)
  negative = (255 - images).astype(dtype)
  kwargs = dict(P=zoomed(CAMERAS))
  for size in (ROW_SIZE, FLAT_SIZE):
    def matches_remap(fused):
      two = undistort.remap(images, undistort.undistort_maps(CAMERAS, size, **kwargs), of)
      assert fused.shape == two.shape and fused.tobytes() == two.tobytes()
      assert len(np.unique(fused)) > 4
    check_rounds(grid_cap, f"undistort_images {size}", remap_workgroups(len(CAMERAS), n, size),
                 lambda: undistort.undistort_images(CAMERAS, images, of, image_size=size, **kwargs), lambda r: [r], matches_remap,
                 lambda: undistort.undistort_images(CAMERAS, negative, of, image_size=size, border=77.0, **kwargs))


# ---- k_warp_points, and k_remap_cubic behind the corrected entry -------------------------------------------------------------------
def fields_for(sizes, nx, ny, seed=3):
  """N(0, 1 px) control values scaled so that the worst camera's fold bound is 0.15"""
  f = ch.random_field(seed, sizes, nx, ny)
  return ch.scaled(f, 0.15 / f.fold_bound().max())


@pytest.mark.parametrize("direction", ["forward", "inverse"])
def test_warp_points(grid_cap, direction):
  """n = 1000 over two cameras of different size: four workgroups; the bars of test_gpu_correction.py"""
  n = 1000
  f = fields_for([(W, H), (64, 48)], 5, 4)
  px, of = ch.point_cases(f.image_sizes, f.nx, f.ny, n, 11)
  warp = f.correct if direction == "forward" else f.uncorrect

  def matches_host(result):
    got, st = result
    want, st_host = ch.on_host(warp, px, of)
    assert got.shape == (n, 2) and np.array_equal(st, st_host) and np.array_equal(np.isnan(got), np.isnan(want))
    ok = st_host == correction.WARP_OK
    assert np.array_equal(ok, np.isfinite(px).all(axis=1)) and ok.sum() > 900
    bar = 32.0 * ch.U * (np.abs(px[ok]).max(axis=1) + np.abs(f.coefficients).max()) if direction == "forward" else 1e-10
    assert (np.abs(got[ok] - want[ok]).max(axis=1) <= bar).all()
  check_rounds(grid_cap, f"warp_points {direction}", ceil_div(n, THREADS), lambda: warp(px, of), lambda r: list(r), matches_host,
               lambda: warp(px + 3.0, of))


def test_corrected_images(grid_cap):
  """mcba_undistort_images_corrected at 516 x 5: k_warp_map (a two-dimensional grid, not capped) feeds the map-fed k_remap_cubic, 18
  tiles; as in test_gpu_correction.py the call is remap through the corrected maps byte for byte"""
  cams = [uh.fixture_camera(name) for name in ("tiny", "tiny_fisheye", "tiny_rational")]
  f = fields_for([(W, H)] * 3, 5, 4)
  wd, hd = ROW_SIZE
  P = np.stack([np.diag([wd / W, hd / H, 1.0]) @ c.intrinsic for c in cams])          # the result spans the source
  of = np.array([2, 0, 2], dtype=np.int32)
  images = uh.noise_image(23, (3, H, W, 3), np.uint8)

  def matches_remap(got):
    want = undistort.remap(images, undistort.undistort_maps(cams, ROW_SIZE, P=P, correction=f), of, border=3.0)
    assert got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()
    assert got.tobytes() != undistort.undistort_images(cams, images, of, ROW_SIZE, P=P, border=3.0).tobytes()
  check_rounds(grid_cap, "undistort_images_corrected", remap_workgroups(3, 3, ROW_SIZE),
               lambda: undistort.undistort_images(cams, images, of, ROW_SIZE, P=P, border=3.0, correction=f), lambda r: [r], matches_remap,
               lambda: undistort.undistort_images(cams, 255 - images, of, ROW_SIZE, P=P, border=77.0, correction=f))


# ---- k_triangulate -------------------------------------------------------------------------------------------------------------
TRI_F, TRI_M_MAX = 3, 513


@functools.lru_cache(maxsize=None)
def triangulate_case(Cn, rolling):
  """the rig at the largest M and its host result, once (a point does not depend on its neighbours: see test_gpu_triangulate.py)"""
  rig = th.make_rig(Cn, TRI_F, TRI_M_MAX, rolling)
  return rig, th.run(rig, sigma=1.0)


@pytest.mark.parametrize("rolling", [False, True], ids=["static", "rolling"])
@pytest.mark.parametrize("M", [257, 513])
@pytest.mark.parametrize("Cn", [2, 8])
def test_triangulate(grid_cap, Cn, M, rolling):
  """three frames of two or three tiles each: six or nine rounds, and the camera records in LDS change frame between two rounds of
  a workgroup (under a cap of 1: twice; under 2 and an odd tile count: a workgroup alternates)"""
  rig, want = triangulate_case(Cn, rolling)
  part = t_triangulate.first_points(rig, M)
  label = f"C={Cn} F={TRI_F} M={M}{' rolling' if rolling else ''}"
  base = check_rounds(grid_cap, label, TRI_F * ceil_div(M, THREADS), lambda: th.run(part, backend="device", sigma=1.0),
                      lambda r: [r[k] for k in ("points", "cov", "sse", "error", "n_views", "status")],
                      lambda got: t_triangulate.compare(got, want, M, label),
                      lambda: th.run(part, backend="device", sigma=1.0, points=part.points + 0.5))
  assert (base.status == triangulate.OK).sum() > M


# ---- k_projection_uncertainty ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["as listed", "reversed"])
def test_projection_uncertainty(grid_cap, order):
  """the call of test_two_jobs_of_different_width_share_a_call with a third job: lists of 257 and 513 queries and a grid of 85 (2 + 3 +
  1 tiles), three record widths, an unconstrained column (the staged record then begins with a unit column) in the second job only"""
  m = ul.rig()
  p = m.stored_count(1, 5)
  loose = np.zeros(p, dtype=bool)
  loose[5 + m.n_dist[1] + 3] = True                                  # x of camera 1's pose: at infinity no pixel depends on it
  jobs = [t_uncertainty.job_of(4, None, 1.5, 3, pixels=t_uncertainty.spread_pixels(257, 3)),
          uncertainty.Job(1, 5, np.inf, ul.random_spd(p, 4), loose, pixels=t_uncertainty.spread_pixels(513, 4)),
          t_uncertainty.job_of(6, 7, 2.0, 2, grid=uncertainty.grid_of(ul.uh.IMAGE_SIZE, (17, 5)))]
  if order == "reversed":
    jobs = jobs[::-1]
  tiles = sum(ceil_div(j.n, THREADS) for j in jobs)
  assert tiles == 6
  doubled = [uncertainty.Job(j.camera, j.reference, np.inf if j.rho == 0 else 1.0 / j.rho, 2.0 * j.sigma, j.loose, grid=j.grid, pixels=j.pixels)
             for j in jobs]

  def matches_host(base):
    dev = t_uncertainty.compare(jobs, f"three jobs {order}")
    assert blob(dev) == blob(base)
  base = check_rounds(grid_cap, f"projection_uncertainty {order}", tiles, lambda: ul.run(m, jobs, "device"), lambda r: list(r), matches_host,
                      lambda: ul.run(m, doubled, "device"))
  first = np.concatenate([[0], np.cumsum([j.n for j in jobs])])
  for j, job in enumerate(jobs):
    assert (base[2][first[j]:first[j + 1]] == uncertainty.OK).mean() > 0.5, (order, j)


# ---- k_projdiff_map ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["transfer first", "intrinsics first"])
def test_projection_diff(grid_cap, order):
  """the call of test_jobs_of_every_kind_share_a_call_and_a_failed_fit_leaves_its_neighbours_alone with at least 257 queries a job (two
  tiles each): a transfer job, a job whose fit failed, a rigid fit and a job without a fit.  A job without calibration A does not
  stage camera a and R_ba | t_ba: after a transfer job that part of the record in LDS is the transfer job's"""
  px = pl.spread_pixels(300, 3)
  jobs = [compare.Job(5, 1, 1.5, pixels=px),
          pl.fit_job(2, np.inf, compare.ROTATION, fit_pixels=pl.inner_pixels(1), pixels=px[:257]),
          pl.fit_job(4, 1.5, compare.RIGID, pixels=px[:257]),
          pl.fit_job(7, 1.5, compare.NONE, grid=uncertainty.grid_of(pl.IMAGE_SIZE, (20, 13)))]
  if order == "intrinsics first":
    jobs = jobs[::-1]
  failed = 1 if order == "transfer first" else 2
  tiles = sum(ceil_div(j.n, THREADS) for j in jobs)
  assert tiles == 8 and all(j.n >= 257 for j in jobs)

  def matches_host(base):
    dev = t_projdiff.compare_runs(jobs, f"four jobs, {order}")
    assert pl.bytes_of(dev) == pl.bytes_of(base)
  base = check_rounds(grid_cap, f"projection_diff {order}", tiles, lambda: pl.run(jobs, "device"),
                      lambda r: [r[k] for k in ("diff", "magnitude", "landing", "status", "transform", "fit_info")], matches_host,
                      lambda: pl.run(jobs, "device", pl.rigs()[::-1]))
  first = np.concatenate([[0], np.cumsum([j.n for j in jobs])])
  for j in range(4):
    status = base.status[first[j]:first[j + 1]]
    if j == failed:
      assert base.fit_info[j, 4] == compare.FIT_TOO_FEW and (status == compare.NO_FIT).all()
    else:
      assert base.fit_info[j, 4] == compare.FIT_OK and (status == compare.OK).mean() > 0.5, (order, j)


# ---- k_reconstruction_uncertainty, k_reconstruction_pairs ------------------------------------------------------------------------
def recon_jobs(wide, order):
  """(rig of eight cameras, [wide job, narrow job] in that or the other order).  wide: G = 8 (the kernels' <8> form) or 3 (<4>) with
  r = 40 (three column tiles) over 33 points, slot 1 masked out of every third point, the points 10, 21, 32 behind the group (TOO_FEW)
  and 12, 25 far to one side; narrow: G = 2 with r = 7 (one column tile) over 17 points, the last of them left with one view."""
  big, _ = rl.group_rig(0, 8)
  maps, rng = rl.stored_maps(big), np.random.default_rng(5)

  def job(group, reference, r, n, seed, masks):
    factors = [(maps[c] @ (1e-4 * rng.normal(size=(maps[c].shape[1], r))), False) for c in group]
    return reconstruction.Job(group, reference, factors, t_recon.volume_points(n, seed, len(group)), masks)
  group = list(range(8)) if wide == 8 else [1, 4, 6]
  every = (1 << len(group)) - 1
  masks = np.array([every & ~2 if i % 3 == 1 else every for i in range(33)], dtype=np.uint64)
  jobs = [job(group, None if wide == 8 else 4, 40, 33, 4, masks), job([6, 2], 2, 7, 17, 6, np.array([3] * 16 + [1], dtype=np.uint64))]
  return big, jobs[::-1] if order == "narrow first" else jobs


def recon_decoys(jobs):
  """the same jobs with twice the factors (run with another sigma2 as well)"""
  return [reconstruction.Job(j.group, j.reference, [(2.0 * Wc, loose) for Wc, loose in j.factors], j.points, j.masks) for j in jobs]


@pytest.mark.parametrize("order", ["wide first", "narrow first"])
@pytest.mark.parametrize("wide", [3, 8], ids=["G3-G2", "G8-G2"])
def test_reconstruction_uncertainty(grid_cap, wide, order):
  """3 + 2 tiles: the stage of a round holds the partial sums of the round before, and the next job has another G (another row stride
  of the stage) and another ldw; Pt and St carry a failed point into the next round"""
  big, jobs = recon_jobs(wide, order)
  tiles = sum(ceil_div(len(j.points), 16) for j in jobs)
  assert tiles == 5
  keys = ("cov_cal", "cov_noise", "n_views", "views", "status")

  def matches_host(base):
    dev = t_recon.compare(big, jobs, f"G = {wide} | G = 2, {order}")
    assert blob(dev[k] for k in keys) == blob(base[k] for k in keys)
  base = check_rounds(grid_cap, f"reconstruction_uncertainty {wide} {order}", tiles, lambda: rl.run(big, jobs, 0.3, 0.0, "device"),
                      lambda r: [r[k] for k in keys], matches_host, lambda: rl.run(big, recon_decoys(jobs), 0.7, 0.0, "device"))
  wide_at = 0 if order == "wide first" else 17
  status, n_views = base.status[wide_at:wide_at + 33], base.n_views[wide_at:wide_at + 33]
  assert (status[[10, 21, 32]] == reconstruction.TOO_FEW).all() and (status == reconstruction.OK).sum() >= 25
  assert n_views.max() == wide and ((base.views[wide_at:wide_at + 33][1::3] & np.uint64(2)) == 0).all()
  narrow_at = 33 if order == "wide first" else 0
  assert base.status[narrow_at + 16] == reconstruction.TOO_FEW and base.n_views[narrow_at:narrow_at + 17].max() == 2


@pytest.mark.parametrize("order", ["wide first", "narrow first"])
@pytest.mark.parametrize("wide", [3, 8], ids=["G3-G2", "G8-G2"])
def test_reconstruction_pairs(grid_cap, wide, order):
  """the same two jobs with 17 and 9 pairs (3 + 2 tiles): pairs of a point with itself, pairs with a failed a end and with a failed b
  end, whose rows of Pt, Nz and St keep the round before's values"""
  big, jobs = recon_jobs(wide, order)
  p_wide, p_narrow = t_length.random_pairs(33, 17, 1), t_length.random_pairs(17, 9, 2)
  p_wide[1], p_wide[2], p_wide[9], p_wide[16] = [10, 0], [0, 21], [32, 5], [3, 3]
  p_narrow[-1] = [16, 0]
  pairs = [p_wide, p_narrow] if order == "wide first" else [p_narrow, p_wide]
  tiles = sum(ceil_div(len(p), 8) for p in pairs)
  assert tiles == 5 and (p_wide[6] == p_wide[6][::-1]).all()

  def matches_host(base):
    dev = t_length.compare(big, jobs, pairs, f"G = {wide} | G = 2, {order}")
    assert ll.raw_bytes(dev) == ll.raw_bytes(base)
  base = check_rounds(grid_cap, f"reconstruction_pairs {wide} {order}", tiles, lambda: ll.run(big, jobs, pairs, 0.3, 0.0, "device"),
                      lambda r: [r[k] for k in ll.RAW], matches_host, lambda: ll.run(big, recon_decoys(jobs), pairs, 0.7, 0.0, "device"))
  wide_at = 0 if order == "wide first" else 9
  status = base.status[wide_at:wide_at + 17]
  assert (status[[1, 2, 9]] == reconstruction.TOO_FEW).all() and (status == reconstruction.OK).sum() >= 8
  assert (base.length[wide_at + 6] == 0) and (base.length[wide_at + 16] == 0)
  assert base.status[(17 if order == "wide first" else 0) + 8] == reconstruction.TOO_FEW
