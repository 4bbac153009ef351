"""The warp of the residual field (csrc/mcba_warp.h) in its g++ build, against an independent numpy / scipy
restatement (correction_reference.py), and the Python layer on top of it (multical_amd.correction, the `correction` argument of the
undistort module, export / import) driven through that build.  No GPU.

Bars: field values and derivatives 32 * 2^-53 * max|coef| (16 non-negative weights that sum to 1, each from a handful of roundings);
a round trip of two Newton solves stopped at 1e-11 px and contracting by at most 0.5 a step 1e-10 px; against scipy's root 1e-9 px
(the project's fixed-x bar for pixels); maps 1 float32 ulp; images byte for byte.
"""
import json

import numpy as np
import pytest

from multical_amd import correction, export, import_calib, residual_field as rf, undistort
from multical_amd.correction import FieldCorrection
from multical_amd.structs import Table, struct

import correction_host_lib as ch
import correction_reference as ref
import host_build
import residual_field_host_lib as rfh
import undistort_host_lib as uh

W, H = ch.IMAGE_SIZE
CAMERAS = uh.fixture_cameras()
SEED_FIELD = 7         # N(0, 1 px) control values on 200 x 150 at 5 x 4 whose fold bound is below 0.2 (asserted where it is used)


def both_hosts():
  """the undistort module and the correction module served by their g++ builds"""
  import contextlib
  stack = contextlib.ExitStack()
  stack.enter_context(uh.host_backend())
  stack.enter_context(ch.host_backend())
  return stack


def seeded_field(n_cameras=1, nx=5, ny=4):
  f = ch.random_field(SEED_FIELD, [(W, H)] * n_cameras, nx, ny, 1.0 if n_cameras == 1 else 0.7)     # (0.7 px: every camera below 0.2)
  assert f.fold_bound().max() < 0.2, f.fold_bound()
  return f


# ---- 1. values and derivatives -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ch.GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_field_value_and_derivatives_against_scipy_bspline(grid):
  nx, ny = grid
  rng = np.random.default_rng(11)
  coef = rng.normal(size=((nx + 3) * (ny + 3), 2))
  px = np.concatenate([rng.uniform([0.0, 0.0], [W, H], (500, 2)), ch.edge_pixels((W, H), nx, ny)])
  e, J, e_only = ch.field_value_jacobian(coef, px, (W, H), nx, ny)
  want_e, want_J = ref.field(coef, px, (W, H), nx, ny)
  tol = 32.0 * ch.U * np.abs(coef).max()
  print(f"  {nx}x{ny}: value {np.abs(e - want_e).max():.2e}, derivative {np.abs(J - want_J).max():.2e}, bar {tol:.2e}")
  assert np.array_equal(e, e_only)
  assert np.abs(e - want_e).max() <= tol and np.abs(J - want_J).max() <= tol


def test_field_is_clamped_outside_the_image():
  f = seeded_field()
  v = np.linspace(0.0, H, 13)
  for outside, edge in (([-20.0, 0.0], [0.0, 0.0]), ([W + 20.0, 0.0], [float(W), 0.0]), ([-0.5, 0.0], [0.0, 0.0])):
    a = np.stack([np.full_like(v, outside[0]), v], axis=1)
    b = np.stack([np.full_like(v, edge[0]), v], axis=1)
    ea, Ja, _ = ch.field_value_jacobian(f.coefficients[0], a, (W, H), f.nx, f.ny)
    eb, Jb, _ = ch.field_value_jacobian(f.coefficients[0], b, (W, H), f.nx, f.ny)
    assert np.array_equal(ea, eb)                                    # bit for bit
    assert (Ja[:, :, 0] == 0.0).all() and np.array_equal(Ja[:, :, 1], Jb[:, :, 1])
  u = np.linspace(0.0, W, 13)
  ea, Ja, _ = ch.field_value_jacobian(f.coefficients[0], np.stack([u, np.full_like(u, H + 20.0)], axis=1), (W, H), f.nx, f.ny)
  eb, _, _ = ch.field_value_jacobian(f.coefficients[0], np.stack([u, np.full_like(u, float(H))], axis=1), (W, H), f.nx, f.ny)
  assert np.array_equal(ea, eb) and (Ja[:, :, 1] == 0.0).all()


def test_fold_bound_three_ways():
  for nx, ny in ch.GRIDS:
    f = ch.random_field(5, [(W, H), (64, 48)], nx, ny)
    L = f.fold_bound()
    for c in range(2):
      assert ch.fold_bound(f.coefficients[c], f.image_sizes[c], nx, ny) == pytest.approx(L[c], rel=1e-14)
    # L bounds the infinity norm of De: sampled on a dense grid
    u, v = np.meshgrid(np.linspace(0, W, 41), np.linspace(0, H, 31))
    J = ref.field(f.coefficients[0], np.stack([u.ravel(), v.ravel()], axis=1), (W, H), nx, ny)[1]
    assert np.abs(J).sum(axis=2).max() <= L[0] * (1.0 + 1e-12)


# ---- 2. the inverse warp ------------------------------------------------------------------------------------------------------
def test_inverse_round_trip_and_restatement():
  f = seeded_field()
  print(f"  fold bound {f.fold_bound()[0]:.4f}")
  rng = np.random.default_rng(13)
  px = np.concatenate([rng.uniform([-20.0, -20.0], [W + 20.0, H + 20.0], (2000, 2)), ch.edge_pixels((W, H), f.nx, f.ny)])
  q, st_f = ch.on_host(f.correct, px)
  back, st_i = ch.on_host(f.uncorrect, q)
  assert (st_f == correction.WARP_OK).all() and (st_i == correction.WARP_OK).all()
  err = np.abs(back - px).max()
  fwd = np.abs(q - ref.warp_forward(f.coefficients[0], px, (W, H), f.nx, f.ny)).max()
  print(f"  uncorrect(correct(p)) - p: {err:.2e} px; forward against the restatement {fwd:.2e} px")
  assert err <= 1e-10
  assert fwd <= 32.0 * ch.U * (np.abs(px).max() + np.abs(f.coefficients).max())
  some = rng.choice(len(px), 300, replace=False)
  inv, _ = ch.on_host(f.uncorrect, px[some])
  want = ref.warp_inverse_root(f.coefficients[0], px[some], (W, H), f.nx, f.ny)
  print(f"  inverse against scipy.optimize.root: {np.abs(inv - want).max():.2e} px")
  assert np.abs(inv - want).max() <= 1e-9
  # the inverse really inverts: w(w^-1(q)) = q
  assert np.abs(ref.warp_forward(f.coefficients[0], inv, (W, H), f.nx, f.ny) - px[some]).max() <= 1e-10


def test_non_finite_points():
  f = seeded_field()
  bad = np.array([[np.nan, 1.0], [1.0, np.nan], [np.inf, 1.0], [1.0, -np.inf], [-np.inf, np.inf], [10.0, 20.0]])
  for call in (f.correct, f.uncorrect):
    out, status = ch.on_host(call, bad)
    assert list(status) == [correction.WARP_NOT_CONVERGED] * 5 + [correction.WARP_OK]
    assert np.isnan(out[:5]).all() and np.isfinite(out[5]).all()


def test_points_camera_per_point_and_empty():
  sizes = [(W, H), (64, 48)]
  f = ch.scaled(ch.random_field(3, sizes, 5, 4), 0.25)
  px, of = ch.point_cases(sizes, 5, 4, 257, 1)
  out, status = ch.on_host(f.correct, px, of)
  for c in range(2):
    one = FieldCorrection(f.coefficients[c:c + 1], sizes[c:c + 1], 5, 4)
    want, st = ch.on_host(one.correct, px[of == c])
    assert np.array_equal(out[of == c], want, equal_nan=True) and np.array_equal(status[of == c], st)
  empty, st = ch.on_host(f.correct, np.zeros((0, 2)))
  assert empty.shape == (0, 2) and st.shape == (0,)


# ---- 3. the zero field --------------------------------------------------------------------------------------------------------
def test_zero_field_is_the_identity_bit_for_bit():
  z = ch.zero_field([(W, H)])
  rng = np.random.default_rng(17)
  px = np.concatenate([rng.uniform([-20.0, -20.0], [W + 20.0, H + 20.0], (500, 2)), ch.edge_pixels((W, H), 5, 4)])
  px = np.where(px == 0.0, 0.0, px)                   # (+0: p + 0 is p for every p but -0)
  for call in (z.correct, z.uncorrect):
    out, status = ch.on_host(call, px)
    assert np.array_equal(out.view(np.uint64), px.view(np.uint64)) and (status == correction.WARP_OK).all()


def test_zero_field_maps_are_the_uncorrected_maps():
  z = ch.zero_field([(W, H)] * len(CAMERAS))
  for label, kwargs in (("P=K", dict()), ("zoomed out", dict(P=np.stack([uh.zoomed_out(c) for c in CAMERAS]))),
                        ("rotated", dict(R=uh.small_rotation(), P=np.stack([uh.zoomed_out(c, 0.8) for c in CAMERAS])))):
    with both_hosts():
      plain = undistort.undistort_maps(CAMERAS, (W, H), **kwargs)
      corrected = undistort.undistort_maps(CAMERAS, (W, H), correction=z, **kwargs)
    assert np.array_equal(plain.view(np.uint32), corrected.view(np.uint32)), label


# ---- 4. maps and images -------------------------------------------------------------------------------------------------------
MAP_CASES = (("P=K", lambda c: dict()), ("zoomed out", lambda c: dict(P=uh.zoomed_out(c))),
             ("rotated", lambda c: dict(R=uh.small_rotation(), P=uh.zoomed_out(c, 0.8))))


@pytest.mark.parametrize("index", range(len(CAMERAS)), ids=uh.CAMERA_IDS)
def test_corrected_maps_match_restatement(index):
  cam = CAMERAS[index]
  f = FieldCorrection(seeded_field(len(CAMERAS)).coefficients[index:index + 1], [(W, H)], 5, 4)
  assert f.fold_bound().max() < 0.2
  for label, make in MAP_CASES:
    kwargs = make(cam)
    with both_hosts():
      got = undistort.undistort_maps([cam], (W, H), correction=f, **kwargs)[0]
      plain = undistort.undistort_maps([cam], (W, H), **kwargs)[0]
    want = ref.corrected_map(cam, (W, H), f.coefficients[0], (W, H), 5, 4, **kwargs)
    d = uh.ulp_distance(got, want)
    moved = np.nanmax(np.abs(got - plain))
    print(f"  {uh.CAMERA_IDS[index]} {label}: at most {int(d.max())} ulp, {int(np.isnan(got[..., 0]).sum())} NaN pixels, the field moves the map by up to {moved:.3f} px")
    assert got.shape == (H, W, 2) and got.dtype == np.float32
    assert np.array_equal(np.isnan(got), np.isnan(want)) and d.max() <= 1
    assert moved > 0.1                                       # (the field is really applied)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("wd", [8, 7], ids=["row", "flat"])
def test_corrected_images_are_remap_through_corrected_maps(dtype, channels, wd):
  f = seeded_field(len(CAMERAS))
  hd = 6
  P = np.stack([np.diag([wd / W, hd / H, 1.0]) @ c.intrinsic for c in CAMERAS])          # the small result spans the source
  of = np.array([3, 0, 7, 5, 0, 6, 1, 2, 4], dtype=np.int32)
  shape = (len(of), H, W) + ((3,) if channels == 3 else ())
  images = uh.noise_image(23, shape, dtype)
  with both_hosts():
    got = undistort.undistort_images(CAMERAS, images, of, (wd, hd), P=P, border=3.0, correction=f)
    maps = undistort.undistort_maps(CAMERAS, (wd, hd), P=P, correction=f)
    want = undistort.remap(images, maps, of, border=3.0)
  assert got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()
  assert len(np.unique(got)) > 4                              # (not one flat border)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals():
  f = seeded_field(2)
  px = np.array([[1.0, 2.0]])
  cams = CAMERAS[:2]

  def field(**over):
    d = dict(coefficients=f.coefficients, image_sizes=f.image_sizes, nx=f.nx, ny=f.ny)
    d.update(over)
    return FieldCorrection(**d)

  def struct_with(obj, **fields):
    s = obj.struct()
    for k, v in fields.items():
      setattr(s, k, v)
    return s

  with both_hosts():
    with pytest.raises(RuntimeError, match="the field set has 2 cameras, the camera set 3"):
      undistort.undistort_maps(CAMERAS[:3], (8, 4), correction=f)
    with pytest.raises(RuntimeError, match="the field set has 2 cameras, the camera set 1"):
      undistort.undistort_images(CAMERAS[:1], np.zeros((1, 8, 8), dtype=np.uint8), correction=f)
    nan = f.coefficients.copy()
    nan[1, 5, 0] = np.nan
    with pytest.raises(RuntimeError, match="a coefficient of camera 1 is not finite"):
      field(coefficients=nan).correct(px)
    with pytest.raises(RuntimeError, match="image size of camera 1 is not positive"):
      field(image_sizes=[(W, H), (W, 0)]).correct(px)
    with pytest.raises(RuntimeError, match="names camera"):
      f.correct(px, [2])
    with pytest.raises(RuntimeError, match="names camera"):
      undistort.undistort_images(cams, np.zeros((1, 8, 8), dtype=np.uint8), [2], correction=f)
    with pytest.raises(RuntimeError, match="images of 1 or 3 channels"):
      undistort.undistort_images(cams, np.zeros((1, 8, 8, 2), dtype=np.uint8), correction=f)
    with pytest.raises(RuntimeError, match="border value must be finite"):
      undistort.undistort_images(cams, np.zeros((1, 8, 8), dtype=np.uint8), border=np.inf, correction=f)
  # grids the struct can name but the object cannot be built with: through the entry itself
  import ctypes as C
  out, status = np.empty((1, 2)), np.empty(1, dtype=np.uint8)
  for over, message in ((dict(nx=0), "nx and ny must be at least 1"), (dict(ny=0), "nx and ny must be at least 1"),
                        (dict(nx=6, ny=4), "need 63 control points, more than 62")):
    s = struct_with(f, **over)
    with pytest.raises(RuntimeError, match=message):
      ch.entry("warp_points")(C.byref(s), 1, None, 0, px.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double)),
                              status.ctypes.data_as(C.POINTER(C.c_uint8)))


def test_fold_limit_passes_just_below_and_refuses_just_above():
  f = seeded_field()
  L = f.fold_bound()[0]
  below, above = ch.scaled(f, 0.2 * (1.0 - 1e-9) / L), ch.scaled(f, 0.2 * (1.0 + 1e-9) / L)
  assert below.fold_bound()[0] < 0.2 < above.fold_bound()[0]
  px = np.array([[10.0, 20.0], [-5.0, 160.0]])
  back, status = ch.on_host(below.uncorrect, ch.on_host(below.correct, px)[0])
  assert (status == correction.WARP_OK).all() and np.abs(back - px).max() <= 1e-10
  for call in (above.correct, above.uncorrect):
    with pytest.raises(RuntimeError, match="the field folds the image"):
      ch.on_host(call, px)
  with both_hosts():
    with pytest.raises(RuntimeError, match="the field folds the image"):
      undistort.undistort_maps(CAMERAS[:1], (8, 4), correction=above)


# ---- 6. planted field, exact ----------------------------------------------------------------------------------------------------
def test_planted_field_is_recovered_and_undone():
  p = ch.planted_exact()
  nx, ny = p.field.nx, p.field.ny
  # the residual at the truth parameters is exactly e(raw): projected = the noise-free detections
  e = np.zeros_like(p.exact)
  for c in range(len(p.sizes)):
    e[c][p.valid[c]] = ref.field(p.field.coefficients[c], p.raw[c][p.valid[c]], p.sizes[c], nx, ny)[0]
  assert np.abs((p.exact - p.raw) - e)[p.valid].max() <= 1e-10
  g = rfh.gram(p.exact, p.raw, p.valid, p.valid, p.sizes, nx, ny, 4, coverage=(4, 4))
  assert int(g.outside.sum()) == 0
  print(f"  cond(B^T B) = {[float(np.linalg.cond(g.gram[c].sum(axis=0)[:-2, :-2])) for c in range(len(p.sizes))]}")
  fit = rf.analyse(g.gram, g.count, g.outside, g.coverage, p.sizes, nx, ny, **ch.EXACT_FIT)
  err = np.abs(fit.coefficients - p.field.coefficients).max()
  print(f"  max |c - c*| = {err:.3e} px, rms {fit.rms}, systematic_rms {fit.systematic_rms}")
  assert err <= 1e-8
  fitted = FieldCorrection(fit.coefficients, p.sizes, nx, ny)
  table = ch.on_host(fitted.correct_table, Table.create(points=p.raw, valid=p.valid))
  undone = np.abs(table.points - p.exact)[p.valid].max()
  print(f"  correct_table(raw) - noise-free detections: {undone:.3e} px")
  assert isinstance(table, Table) and np.array_equal(table.valid, p.valid)
  assert undone <= 1e-8 + 1e-10
  # the sign: the planted field moved the detections by about its amplitude, the wrong direction would double that
  assert np.abs(p.raw - p.exact)[p.valid].max() > 0.1


# ---- 7. persistence -----------------------------------------------------------------------------------------------------------
def _small_calibration():
  from util import load_golden, mirror
  return mirror(load_golden("tiny")[1])


def test_json_round_trip(tmp_path):
  calib = _small_calibration()
  names = struct(camera=list(calib.camera_poses.names))
  files = [[f"{n}/image{i}.png" for i in range(2)] for n in names.camera]
  sizes = [tuple(int(v) for v in cam.image_size) for cam in calib.cameras]
  f = ch.random_field(29, sizes, 5, 4, 0.3)
  corrected = ch.on_host(calib.with_corrected_observations, f)
  assert corrected.correction is f and corrected.raw_point_table is calib.point_table
  export.export(str(tmp_path / "corrected.json"), corrected, names, files)
  back = import_calib.load_calibration(str(tmp_path / "corrected.json"))
  assert np.array_equal(back.correction.coefficients, f.coefficients) and back.correction.image_sizes == f.image_sizes
  assert (back.correction.nx, back.correction.ny) == (5, 4)
  # a calibration without a correction: the file it always had
  export.export(str(tmp_path / "plain.json"), calib, names, files)
  data = json.load(open(tmp_path / "plain.json"))
  assert sorted(data) == ["camera_poses", "cameras", "image_sets"]
  assert "correction" not in import_calib.load_calibration(str(tmp_path / "plain.json"))
  plain = dict(json.load(open(tmp_path / "corrected.json")))
  del plain["residual_correction"]
  assert json.dumps(plain, indent=2) == open(tmp_path / "plain.json").read()


def test_plain_export_is_byte_identical_without_the_correction_module(tmp_path):
  """in a fresh interpreter that never imports multical_amd.correction"""
  import subprocess
  import sys
  calib = _small_calibration()
  names = struct(camera=list(calib.camera_poses.names))
  files = [[f"{n}/image{i}.png" for i in range(2)] for n in names.camera]
  export.export(str(tmp_path / "here.json"), calib, names, files)
  script = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from util import load_golden, mirror\n"
            "from multical_amd import export\n"
            "from multical_amd.structs import struct\n"
            "calib = mirror(load_golden('tiny')[1])\n"
            "names = struct(camera=list(calib.camera_poses.names))\n"
            "files = [[f'{n}/image{i}.png' for i in range(2)] for n in names.camera]\n"
            "export.export(%r, calib, names, files)\n"
            "assert 'multical_amd.correction' not in sys.modules\n") % (host_build.ROOT, host_build.HERE, str(tmp_path / "fresh.json"))
  subprocess.run([sys.executable, "-c", script], check=True)
  assert open(tmp_path / "here.json", "rb").read() == open(tmp_path / "fresh.json", "rb").read()


def test_dict_round_trip_and_composition():
  f = seeded_field(2)
  g = FieldCorrection.from_dict(json.loads(json.dumps(f.to_dict())))
  assert np.array_equal(g.coefficients, f.coefficients) and g.image_sizes == f.image_sizes and (g.nx, g.ny) == (f.nx, f.ny)
  calib = _small_calibration()
  sizes = [tuple(int(v) for v in cam.image_size) for cam in calib.cameras]
  h = ch.random_field(31, sizes, 5, 4, 0.3)
  once = ch.on_host(calib.with_corrected_observations, h)
  twice = ch.on_host(once.with_corrected_observations, h)
  assert twice.raw_point_table is calib.point_table
  assert np.array_equal(once.point_table.points, twice.point_table.points, equal_nan=True)
  assert np.array_equal(once.point_table.valid, calib.point_table.valid)
  moved = once.with_param_vec(once.param_vec)
  assert moved.correction is h and moved.raw_point_table is calib.point_table     # (a copy keeps the correction)


# ---- 8. points through the corrected camera -----------------------------------------------------------------------------------
def test_corrected_camera_points():
  cams = CAMERAS[:2]
  f = seeded_field(2)
  rng = np.random.default_rng(37)
  X = np.concatenate([rng.uniform(-0.2, 0.2, (100, 2)), np.ones((100, 1))], axis=1)
  of = (np.arange(100) % 2).astype(np.int32)
  with both_hosts():
    raw, status = undistort.project_points(cams, X, of, correction=f)
    model = undistort.project_points(cams, X, of)
    xy, st = undistort.undistort_points(cams, raw, of, correction=f)
  assert (status == correction.WARP_OK).all() and (st == undistort.UNDISTORT_OK).all()
  assert np.abs(ch.on_host(f.correct, raw, of)[0] - model).max() <= 1e-10          # w(project_corrected(X)) = pi(X)
  assert np.abs(xy - X[:, :2]).max() * cams[0].intrinsic[0, 0] <= 1e-9             # undistort_corrected inverts project_corrected


# ---- 9. sanitiser ---------------------------------------------------------------------------------------------------------------
def test_sanitized_stand_alone_run(tmp_path):
  """AddressSanitizer + UBSan on a CPU executable of its own (nothing is loaded into Python, nothing is preloaded)"""
  r = host_build.sanitized_program("correction_host", "correction_sanitize_main.cpp", tmp_path)
  assert r.returncode == 0 and "correction sanitize run: ok" in r.stdout, r.stdout + r.stderr


# ---- the boundary ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_bound():
  import os
  from multical_amd import _lib, build
  sig = dict((s[0], s) for s in _lib.SYMBOLS)
  assert len(sig["mcba_warp_points"][2]) == 7 and len(sig["mcba_undistort_maps_corrected"][2]) == 7
  assert len(sig["mcba_undistort_images_corrected"][2]) == 15 and len(sig["mcba_debug_warp_ms"][2]) == 2
  header = open(os.path.join(host_build.ROOT, "include", "mcba.h")).read()
  for name in ("mcba_field_set", "mcba_warp_points", "mcba_undistort_maps_corrected", "mcba_undistort_images_corrected", "mcba_debug_warp_ms"):
    assert name in header
  assert build.SOURCES[-1] == "mcba_warp.hip"
