"""No GPU: the residual field on the host -- the g++ build of csrc/mcba_residual_field.h against an independent
scipy / dense numpy restatement (residual_field_reference), the numpy algebra of multical_amd.residual_field against the same
quantities from the dense rows, and planted fields.

Bounds: a Gram entry against another summation of the same products, |dG_ij| <= 4 n 2^-53 A_ij with n the rows of the slice and A
the Gram matrix of the absolute rows (the standard summation bound, not a measurement); weights against scipy's B-splines 1e-14;
the algebra 1e-9 relative.  The planted-noisy test asserts orderings only; the clean run's |z| and cv_gain are printed
(profiles/residual_field_parity.txt keeps a run).
"""
import functools

import numpy as np
import pytest

from multical_amd import residual_field as rf, synthetic
from multical_amd.structs import struct

import residual_field_host_lib as hl
import residual_field_reference as ref

SIGMA2 = 0.04


# ---- 1. weights ---------------------------------------------------------------------------------------------------------------
def test_weights_partition_of_unity_and_scipy():
  rng = np.random.default_rng(0)
  t = np.concatenate([rng.random(1000), [0.0, 1.0, 0.5, 2.0 ** -40, 1.0 - 2.0 ** -53]])
  w = hl.weights(t)
  assert (w >= 0.0).all()
  assert np.abs(w.sum(axis=1) - 1.0).max() <= 4 * 2.0 ** -52
  assert np.abs(w - rf.cubic_weights(t)).max() <= 1e-15          # the numpy twin the field maps are drawn with
  W, H, nx, ny = 1936, 1216, 5, 4
  px = np.column_stack([rng.random(1000) * W, rng.random(1000) * H])
  edges = np.array([[0.0, 0.0], [W, 0.0], [0.0, H], [W, H], [W, 0.37 * H], [0.61 * W, H], [0.0, 0.5 * H], [0.25 * W, 0.0]])
  px = np.vstack([px, edges])
  col, w16, inside = hl.rows(px, (W, H), nx, ny)
  assert inside.all()
  dense = np.zeros((px.shape[0], rf.n_control(nx, ny)))
  dense[np.arange(px.shape[0])[:, None], col] = w16
  assert (w16 >= 0.0).all() and np.abs(w16.sum(axis=1) - 1.0).max() <= 4 * 2.0 ** -52
  err = np.abs(dense - ref.basis(px, (W, H), nx, ny)).max()
  print(f"  weights against scipy BSpline: max |d| = {err:.3e}")
  assert err <= 1e-14
  assert np.abs(dense - rf.basis(px, (W, H), nx, ny)).max() <= 1e-15


def test_cell_edges_and_outside():
  W, n = 1936, 5
  assert hl.cell(W, W, n) == (n - 1, 1.0)          # exactly on W: the last interval, fraction 1
  assert hl.cell(0.0, W, n) == (0, 0.0)
  i, t = hl.cell(W / n, W, n)
  assert (i, t) == (1, 0.0)
  _, _, inside = hl.rows([[-1e-9, 5.0], [W + 1e-9, 5.0], [5.0, -1e-9], [5.0, 1216 + 1e-9], [np.nan, 5.0], [W, 1216]], (W, 1216), 5, 4)
  assert inside.tolist() == [False, False, False, False, False, True]


def test_outside_pixel_is_counted_and_does_not_enter():
  t = hl.tables("tiny")
  base = hl.gram(t.projected, t.observed, t.valid, t.inlier, t.sizes)
  assert (base.outside == 0).all()
  c, f, b, p = np.argwhere(t.inlier)[7]
  obs = t.observed.copy()
  obs[c, f, b, p, 0] = t.sizes[c][0] + 0.5
  moved = hl.gram(t.projected, obs, t.valid, t.inlier, t.sizes)
  assert moved.outside[c] == 1 and moved.outside.sum() == 1
  assert moved.count.sum() == base.count.sum() - 1 and moved.count[c, f % 5] == base.count[c, f % 5] - 1
  assert moved.coverage.sum() == base.coverage.sum() - 1
  G, count, outside = ref.dense_gram(struct(projected=t.projected, observed=obs, valid=t.valid, inlier=t.inlier, sizes=t.sizes), 5, 4, 5)
  assert np.array_equal(count, moved.count) and np.array_equal(outside, moved.outside)
  assert hl.worst_ratio(G, moved) <= 1.0


# ---- 2. Gram --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hl.FIXTURES)
@pytest.mark.parametrize("grid", [(1, 1), (5, 4), (7, 3)])
def test_gram_against_dense_numpy(name, grid):
  t = hl.tables(name)
  nx, ny = grid
  for inliers_only, n_folds in ((True, 5), (False, 3)):
    host = hl.gram(t.projected, t.observed, t.valid, t.inlier, t.sizes, nx, ny, n_folds, inliers_only, coverage=(16, 12))
    G, count, outside = ref.dense_gram(t, nx, ny, n_folds, inliers_only)
    assert np.array_equal(host.count, count) and np.array_equal(host.outside, outside)
    assert np.array_equal(host.coverage, ref.coverage(t, 16, 12))
    assert np.array_equal(host.gram, np.swapaxes(host.gram, -1, -2))
    ratio = hl.worst_ratio(G, host)
    print(f"  {name} {nx}x{ny} folds={n_folds} inliers_only={inliers_only}: rows {int(count.sum())}, worst |d| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert host.count.sum() + outside.sum() == (t.inlier if inliers_only else t.valid).sum()


# ---- 3. algebra -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hl.FIXTURES)
def test_algebra_against_dense(name):
  t = hl.tables(name)
  nx, ny, n_folds = 5, 4, 5
  host = hl.gram(t.projected, t.observed, t.valid, t.inlier, t.sizes, nx, ny, n_folds)
  for c in range(t.valid.shape[0]):
    R, frame, _ = ref.camera_rows(t, c, nx, ny)
    want = ref.analyse_dense(R, frame, n_folds, nx, ny, SIGMA2)
    got = rf.fit_camera(host.gram[c], host.count[c], nx, ny, SIGMA2)
    rel = lambda a, b: abs(a - b) / abs(b)
    e_c = np.abs(got.coefficients - want["c"]).max() / np.abs(want["c"]).max()
    errs = dict(c=e_c, sse=rel(got.sse, want["sse"]), cv_gain=rel(got.cv_gain, want["cv_gain"]), T=rel(got.T, want["T"]),
                nu=rel(got.nu, want["nu"]), rms=rel(got.rms, want["rms"]), systematic_rms=rel(got.systematic_rms, want["systematic_rms"]))
    print(f"  {name} camera {c}: n={got.n} " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert got.n == R.shape[0]
    assert max(errs.values()) <= 1e-9
    assert abs(got.explained - want["explained"]) <= 1e-9 and abs(got.z - want["z"]) <= 1e-9 * max(1.0, abs(want["z"]))


def test_field_map_and_report_lines():
  t = hl.tables("tiny")
  host = hl.gram(t.projected, t.observed, t.valid, t.inlier, t.sizes)
  out = rf.analyse(host.gram, host.count, host.outside, host.coverage, t.sizes, 5, 4, SIGMA2)
  assert out.field.shape == (2, 12, 16, 2) and out.field_std.shape == (2, 12, 16) and out.pixels.shape == (2, 12, 16, 2)
  assert np.isfinite(out.field).all() and (out.field_std > 0).all()
  c = 1
  b = ref.basis(out.pixels[c].reshape(-1, 2), t.sizes[c], 5, 4)
  assert np.abs(b @ out.coefficients[c] - out.field[c].reshape(-1, 2)).max() <= 1e-12
  R, frame, _ = ref.camera_rows(t, c, 5, 4)
  root = ref.penalty_root(5, 4, SIGMA2, 1.0, 100.0)
  M = np.linalg.inv(R[:, :-2].T @ R[:, :-2] + root.T @ root)
  std = np.sqrt(SIGMA2 * np.einsum("ij,jk,ik->i", b, M, b))
  assert np.abs(std / out.field_std[c].ravel() - 1.0).max() <= 1e-7
  listed = rf.analyse(host.gram, host.count, host.outside, host.coverage, t.sizes, 5, 4, SIGMA2, pixels=[[10.0, 20.0], [-5.0, 3.0]])
  assert listed.field.shape == (2, 2, 2) and np.isfinite(listed.field[:, 0]).all() and np.isnan(listed.field[:, 1]).all()
  lines = rf.report_lines(out, ["left", "right"], "stage")
  assert len(lines) == 2 and all("cv_gain=" in line and " z=" in line and "max |field|=" in line for line, _ in lines)


# ---- 4. planted, exact ----------------------------------------------------------------------------------------------------------
def test_planted_field_is_recovered_exactly():
  t = hl.tables("tiny_rolling")
  nx = ny = 1
  # a camera that sees the whole image: inliers in every one of 4 x 4 cells (16 control points, one interval each way)
  cov = hl.gram(t.projected, t.observed, t.valid, t.inlier, t.sizes, nx, ny, 1, coverage=(4, 4)).coverage
  cams = [c for c in range(cov.shape[0]) if (cov[c, 0] > 0).all()]
  assert cams, f"no camera of the fixture covers the image: {cov[:, 0]}"
  rng = np.random.default_rng(3)
  c_true = 0.5 * rng.normal(size=(len(t.sizes), 16, 2))     # control values of the size of a real residual field: half a pixel
  proj = t.observed.copy()
  for c in cams:
    m = t.inlier[c]
    proj[c][m] = t.observed[c][m] + ref.basis(t.observed[c][m], t.sizes[c], nx, ny) @ c_true[c]
  host = hl.gram(proj, t.observed, t.valid, t.inlier, t.sizes, nx, ny, 4)
  for c in cams:
    cond = np.linalg.cond(host.gram[c].sum(axis=0)[:16, :16])
    fit = rf.fit_camera(host.gram[c], host.count[c], nx, ny, SIGMA2, prior_px=1e9, tau0=1e9)
    err = np.abs(fit.coefficients - c_true[c]).max()
    print(f"  camera {c}: cond(B^T B) = {cond:.3e}, max |c - c*| = {err:.3e} px, 1 - explained = {1.0 - fit.explained:.3e}")
    assert err <= 1e-8
    assert fit.explained >= 1.0 - 1e-12


# ---- 5. planted, noisy ----------------------------------------------------------------------------------------------------------
PLANTED = dict(config="tiny", frames=24, seed=11, noise=0.2, camera=0, amplitude=0.5)


def planted_field(pixels, image_size, amplitude):
  """a smooth field of RMS about `amplitude` px over the image: half a period of a sine across the width and the height"""
  (W, H), u, v = image_size, pixels[..., 0], pixels[..., 1]
  return amplitude * np.sqrt(2.0) * np.stack([np.sin(np.pi * u / W) * np.cos(np.pi * v / H), np.cos(np.pi * u / W) * np.sin(np.pi * v / H)], axis=-1)


@functools.lru_cache(maxsize=None)
def planted_runs():
  """(clean, planted, s): the analysis of the rig's residuals at the TRUE parameters (projected = the noise-free detections of the
  same seed), without and with the field added to one camera's detections; s = the field's RMS at that camera's observations"""
  p = PLANTED
  exact = synthetic.make_rig(p["config"], frames=p["frames"], seed=p["seed"], noise=0.0, outlier_frac=0.0)
  noisy = synthetic.make_rig(p["config"], frames=p["frames"], seed=p["seed"], noise=p["noise"], outlier_frac=0.0)
  assert np.array_equal(exact.valid, noisy.valid)
  sizes = [tuple(int(v) for v in cam.image_size) for cam in noisy.init.cameras]
  out = []
  field = planted_field(noisy.points[p["camera"]], sizes[p["camera"]], p["amplitude"])
  for plant in (False, True):
    obs = noisy.points.copy()
    if plant:
      obs[p["camera"]] -= np.where(noisy.valid[p["camera"]][..., None], field, 0.0)      # residual = projected - observed = noise' + field
    g = hl.gram(exact.points, obs, noisy.valid, noisy.valid, sizes)
    out.append(rf.analyse(g.gram, g.count, g.outside, g.coverage, sizes, 5, 4, p["noise"] ** 2))
  s = float(np.sqrt(np.mean(np.sum(field[noisy.valid[p["camera"]]] ** 2, axis=-1))))
  return out[0], out[1], s


def test_planted_noisy_field_is_found():
  clean, planted, s = planted_runs()
  cam, other, sigma = PLANTED["camera"], 1 - PLANTED["camera"], PLANTED["noise"]
  print(f"  clean run:   |z| = {np.abs(clean.z)}, cv_gain = {clean.cv_gain}, rms = {clean.rms}")
  print(f"  planted run: z = {planted.z}, cv_gain = {planted.cv_gain}, systematic_rms = {planted.systematic_rms}, planted s = {s:.4f} px")
  assert outside_is_empty(clean) and outside_is_empty(planted)
  assert planted.cv_gain[cam] > clean.cv_gain[cam]
  assert planted.cv_gain[cam] > planted.cv_gain[other]
  assert planted.cv_gain[cam] > 0.5 * s * s / (s * s + sigma * sigma)
  assert planted.z[cam] > clean.z[cam]
  lines = rf.report_lines(planted, ["cam0", "cam1"])
  assert lines[cam][1] and not lines[other][1]


def outside_is_empty(result):
  return int(np.sum(result.outside)) == 0


# ---- the boundary -----------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_and_bound():
  import os
  from multical_amd import _lib, calibration
  sig = dict((s[0], s) for s in _lib.SYMBOLS)
  assert len(sig["mcba_residual_gram"][2]) == 13 and len(sig["mcba_debug_residual_gram_ms"][2]) == 2
  header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcba.h")).read()
  assert "int32_t mcba_residual_gram(mcba_handle h, const double* x, const int32_t* image_size /*[C][2] W,H*/," in header
  assert "int32_t mcba_debug_residual_gram_ms(double* ms /*[4]*/, int64_t* n_rows);" in header
  lib = _lib.load()
  assert hasattr(lib, "mcba_residual_gram") and hasattr(lib, "mcba_debug_residual_gram_ms")
  assert callable(calibration.Calibration.residual_field) and callable(calibration.Calibration.report_residual_field)
  assert _lib.MCBA_VERSION == 3   # no struct changes with the new entry point
