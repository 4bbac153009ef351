"""GPU (MI355X): the corrected entry points (mcba_warp_points, mcba_undistort_maps_corrected, mcba_undistort_images_corrected;
DESIGN.md 3.19) against the g++ build of the same header (tests/correction_host), and Calibration.residual_correction /
with_corrected_observations / refine_with_residual_field on top of them.

Bars: the forward warp 32 * 2^-53 * (|p| + max|coef|) (one addition on top of the field's 16 non-negative weights); the inverse
1e-10 px (two Newton solves stopped at 1e-11 px); statuses equal; maps 1 float32 ulp with an equal NaN pattern; images byte for byte.
Every comparison prints its worst deviation before it asserts (profiles/residual_correction_parity.txt keeps a run).
"""
import ctypes as C

import numpy as np
import pytest

from multical_amd import calibration, correction, synthetic, undistort
from multical_amd._lib import McbaError
from multical_amd.correction import WARP_POINTS_MAX_BLOCKS, WARP_THREADS, FieldCorrection

import correction_host_lib as ch
import undistort_host_lib as uh
from test_residual_field_host import PLANTED as NOISY, planted_field

pytestmark = pytest.mark.gpu

W, H = ch.IMAGE_SIZE
SIZES = [(W, H), (64, 48)]                       # two cameras of different image size
PIN5, FISH, RATIONAL = (uh.fixture_camera(name) for name in ("tiny", "tiny_fisheye", "tiny_rational"))


def both_hosts():
  import contextlib
  stack = contextlib.ExitStack()
  stack.enter_context(uh.host_backend())
  stack.enter_context(ch.host_backend())
  return stack


def fields_for(sizes, nx, ny, seed=3):
  """N(0, 1 px) control values scaled so that the worst camera's fold bound is 0.15"""
  f = ch.random_field(seed, sizes, nx, ny)
  return ch.scaled(f, 0.15 / f.fold_bound().max())


# ---- mcba_warp_points -----------------------------------------------------------------------------------------------------------
def _compare_points(f, n, seed):
  px, of = ch.point_cases(f.image_sizes, f.nx, f.ny, n, seed)
  worst = {}
  for name, dev_call in (("forward", f.correct), ("inverse", f.uncorrect)):
    got, st = dev_call(px, of)
    want, st_host = ch.on_host(dev_call, px, of)
    assert got.shape == (n, 2) and st.shape == (n,)
    assert np.array_equal(st, st_host) and np.array_equal(np.isnan(got), np.isnan(want))
    ok = st_host == correction.WARP_OK
    assert np.array_equal(ok, np.isfinite(px).all(axis=1))
    bar = 32.0 * ch.U * (np.abs(px[ok]).max(axis=1) + np.abs(f.coefficients).max()) if name == "forward" else np.full(int(ok.sum()), 1e-10)
    dev = np.abs(got[ok] - want[ok]).max(axis=1) if ok.any() else np.zeros(0)
    worst[name] = float(dev.max()) if dev.size else 0.0
    print(f"  n={n} {f.nx}x{f.ny} {name}: worst |device - host| = {worst[name]:.2e} px")
    assert (dev <= bar).all()
  return worst


@pytest.mark.parametrize("grid", [(1, 1), (5, 4), (7, 3)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_warp_points_sizes_and_edges(grid):
  f = fields_for(SIZES, *grid)
  for n in (0, 1, 63, 64, 65, 255, 256, 257):
    _compare_points(f, n, n + 1)


def test_warp_points_beyond_the_grid_cap():
  n = WARP_POINTS_MAX_BLOCKS * WARP_THREADS + 1      # the launcher caps its grid there: the last point is a lane's second one
  _compare_points(fields_for(SIZES, 5, 4), n, 5)
  ms, count = correction.last_call_ms()
  assert count == n and ms["kernel"] > 0.0 and ms["call"] >= ms["kernel"]


def test_round_trip_on_the_device():
  f = fields_for(SIZES, 5, 4)
  px, of = ch.point_cases(SIZES, 5, 4, 4096, 9)
  ok = np.isfinite(px).all(axis=1)
  q, st = f.correct(px[ok], of[ok])
  back, st_back = f.uncorrect(q, of[ok])
  err = np.abs(back - px[ok]).max()
  print(f"  uncorrect(correct(p)) - p on the device: {err:.2e} px")
  assert (st == 0).all() and (st_back == 0).all() and err <= 1e-10


# ---- mcba_undistort_maps_corrected ----------------------------------------------------------------------------------------------
def _map_kwargs(cams, label):
  if label == "identity":
    return dict()
  return dict(R=uh.small_rotation(), P=np.stack([uh.zoomed_out(c) for c in cams]))


@pytest.mark.parametrize("label", ["identity", "rotated-zoomed"])
@pytest.mark.parametrize("cams", [[PIN5], [PIN5, FISH, RATIONAL]], ids=["C1", "C3"])
@pytest.mark.parametrize("size", [(4, 1), (7, 3), (64, 4), (65, 5), (200, 150)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_corrected_maps(size, cams, label):
  f = fields_for([(W, H)] * len(cams), 5, 4, seed=len(cams))
  kwargs = _map_kwargs(cams, label)
  got = undistort.undistort_maps(cams, size, correction=f, **kwargs)
  again = undistort.undistort_maps(cams, size, correction=f, **kwargs)
  with both_hosts():
    want = undistort.undistort_maps(cams, size, correction=f, **kwargs)
  d = uh.ulp_distance(got, want)
  print(f"  {size} C={len(cams)} {label}: {int((d > 0).sum())} of {d.size} entries differ, at most {int(d.max())} ulp, "
        f"{int(np.isnan(got[..., 0]).sum())} NaN pixels")
  assert got.shape == (len(cams), size[1], size[0], 2) and got.dtype == np.float32
  assert np.array_equal(np.isnan(got), np.isnan(want)) and d.max() <= 1
  assert got.tobytes() == again.tobytes()
  zero = undistort.undistort_maps(cams, size, correction=ch.zero_field([(W, H)] * len(cams)), **kwargs)
  plain = undistort.undistort_maps(cams, size, **kwargs)
  assert zero.tobytes() == plain.tobytes()
  ms, count = correction.last_call_ms()
  assert count == len(cams) * size[0] * size[1]


# ---- mcba_undistort_images_corrected --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("wd", [8, 7], ids=["row", "flat"])
def test_corrected_images(dtype, channels, wd):
  cams = [PIN5, FISH, RATIONAL]
  f = fields_for([(W, H)] * 3, 5, 4)
  hd = 6
  P = np.stack([np.diag([wd / W, hd / H, 1.0]) @ c.intrinsic for c in cams])          # the small result spans the source
  of = np.array([2, 0, 2], dtype=np.int32)                                            # 3 images, camera 1 without one
  images = uh.noise_image(23, (3, H, W) + ((3,) if channels == 3 else ()), dtype)
  got = undistort.undistort_images(cams, images, of, (wd, hd), P=P, border=3.0, correction=f)
  maps = undistort.undistort_maps(cams, (wd, hd), P=P, correction=f)
  want = undistort.remap(images, maps, of, border=3.0)
  assert got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()
  assert len(np.unique(got)) > 4
  plain = undistort.undistort_images(cams, images, of, (wd, hd), P=P, border=3.0)
  assert got.tobytes() != plain.tobytes()                                             # (the field is really applied)


# ---- Calibration, end to end ------------------------------------------------------------------------------------------------------
def test_planted_exact_through_calibration():
  p = ch.planted_exact()
  calib = calibration.from_rig(ch.rig_with_points(p.rig, p.raw), which="truth")
  fitted = calib.residual_correction(nx=p.field.nx, ny=p.field.ny, n_folds=4, **ch.EXACT_FIT)
  err = np.abs(fitted.coefficients - p.field.coefficients).max()
  print(f"  max |c - c*| = {err:.3e} px")
  assert err <= 1e-8
  corrected = calib.with_corrected_observations(fitted)
  undone = np.abs(corrected.point_table.points - p.exact)[p.valid].max()
  rms = corrected.error_statistics(False).rms
  print(f"  correct_table(raw) - noise-free detections: {undone:.3e} px; rms of the corrected calibration at the truth {rms:.3e} px "
        f"(uncorrected {calib.error_statistics(False).rms:.3e})")
  assert undone <= 1e-8 + 1e-10 and rms <= 1e-7
  assert corrected.correction is fitted and corrected.raw_point_table is calib.point_table
  # composition: corrected again with the same correction, it is the raw table that is warped
  again = corrected.with_corrected_observations(fitted)
  assert again.point_table.points.tobytes() == corrected.point_table.points.tobytes()
  assert np.array_equal(again.point_table.valid, calib.point_table.valid)


def test_refine_with_residual_field_on_the_noisy_planted_rig(caplog):
  import logging
  q = NOISY
  noisy = synthetic.make_rig(q["config"], frames=q["frames"], seed=q["seed"], noise=q["noise"], outlier_frac=0.0)
  sizes = [tuple(int(v) for v in cam.image_size) for cam in noisy.init.cameras]
  obs = noisy.points.copy()
  obs[q["camera"]] -= np.where(noisy.valid[q["camera"]][..., None], planted_field(noisy.points[q["camera"]], sizes[q["camera"]], q["amplitude"]), 0.0)
  start = calibration.from_rig(ch.rig_with_points(noisy, obs)).bundle_adjust(solver="native", tolerance=1e-12)     # the uncorrected optimum
  sigma2 = q["noise"] ** 2
  before = start.residual_field(sigma2=sigma2)
  assert int(before.outside.sum()) == 0
  r0 = start.residuals()
  sse0 = float(r0 @ r0)
  out, records = start.refine_with_residual_field(rounds=3, sigma2=sigma2, solver="native", tolerance=1e-12)
  after = out.residual_field(sigma2=sigma2)
  assert int(after.outside.sum()) == 0
  joint = [r.joint for r in records]
  print(f"  uncorrected sse {sse0:.6f}; per round sse {[round(r.sse, 6) for r in records]}, penalty {[round(r.penalty, 6) for r in records]}, "
        f"joint {[round(j, 6) for j in joint]}")
  print(f"  cv_gain before {before.cv_gain}, after {after.cv_gain}; z before {before.z}, after {after.z} (recorded, not asserted)")
  assert len(records) == 3
  for a, b in zip(joint, joint[1:]):
    assert b <= a * (1.0 + 1e-9)
  assert records[-1].sse < sse0
  # the returned field is the fit of the RAW residuals at the parameters before the last adjustment
  raw_before_last = start.with_param_vec(records[-1].param_vec)
  want = raw_before_last.residual_field(sigma2=sigma2).coefficients
  dev = np.abs(out.correction.coefficients - want).max() / np.abs(want).max()
  print(f"  returned field against the fit at the penultimate parameters: {dev:.2e}")
  assert dev <= 1e-9
  assert np.array_equal(records[0].param_vec, start.param_vec) and out.raw_point_table is start.point_table
  with caplog.at_level(logging.INFO, logger="calibration"):
    out.report_residual_correction("end")
  lines = [r.getMessage() for r in caplog.records if "residual correction" in r.getMessage()]
  assert len(lines) == 2 and all(line.startswith("end ") and "fold bound=" in line and "rms before=" in line for line in lines)


# ---- refusals through the C ABI -----------------------------------------------------------------------------------------------------
def test_refusals():
  f = fields_for(SIZES, 5, 4)
  px = np.array([[1.0, 2.0]])
  cams = [PIN5, FISH]
  fc = fields_for([(W, H)] * 2, 5, 4)

  def field(**over):
    d = dict(coefficients=f.coefficients, image_sizes=f.image_sizes, nx=f.nx, ny=f.ny)
    d.update(over)
    return FieldCorrection(**d)

  with pytest.raises(McbaError, match="the field set has 2 cameras, the camera set 3"):
    undistort.undistort_maps([PIN5, FISH, RATIONAL], (8, 4), correction=fc)
  with pytest.raises(McbaError, match="the field set has 2 cameras, the camera set 1"):
    undistort.undistort_images([PIN5], np.zeros((1, 8, 8), dtype=np.uint8), correction=fc)
  nan = f.coefficients.copy()
  nan[1, 5, 0] = np.inf
  with pytest.raises(ValueError, match="a coefficient of camera 1 is not finite"):          # ("not finite": the ValueError convention)
    field(coefficients=nan).correct(px)
  with pytest.raises(McbaError, match="image size of camera 1 is not positive"):
    field(image_sizes=[(W, H), (0, 48)]).correct(px)
  with pytest.raises(McbaError, match="names camera"):
    f.correct(px, [2])
  with pytest.raises(McbaError, match="names camera"):
    undistort.undistort_images(cams, np.zeros((1, 8, 8), dtype=np.uint8), [2], correction=fc)
  with pytest.raises(McbaError, match="images of 1 or 3 channels"):
    undistort.undistort_images(cams, np.zeros((1, 8, 8, 2), dtype=np.uint8), correction=fc)
  with pytest.raises(McbaError, match="border value must be finite"):
    undistort.undistort_images(cams, np.zeros((1, 8, 8), dtype=np.uint8), border=np.inf, correction=fc)
  L = f.fold_bound().max()
  below, above = ch.scaled(f, 0.2 * (1.0 - 1e-9) / L), ch.scaled(f, 0.2 * (1.0 + 1e-9) / L)
  assert below.fold_bound().max() < 0.2 < above.fold_bound().max()
  assert (below.uncorrect(px)[1] == 0).all()
  for call in (above.correct, above.uncorrect):
    with pytest.raises(McbaError, match="the field folds the image"):
      call(px)
  with pytest.raises(McbaError, match="the field folds the image"):
    undistort.undistort_maps(cams, (8, 4), correction=ch.scaled(fc, 0.2 * (1.0 + 1e-9) / fc.fold_bound().max()))
  out, status = np.empty((1, 2)), np.empty(1, dtype=np.uint8)
  for over, message in ((dict(nx=0), "nx and ny must be at least 1"), (dict(ny=0), "nx and ny must be at least 1"),
                        (dict(nx=6, ny=4), "need 63 control points, more than 62")):
    s = f.struct()
    for k, v in over.items():
      setattr(s, k, v)
    with pytest.raises(McbaError, match=message):
      correction._entry("warp_points")(C.byref(s), 1, None, 0, px.ctypes.data_as(C.POINTER(C.c_double)),
                                       out.ctypes.data_as(C.POINTER(C.c_double)), status.ctypes.data_as(C.POINTER(C.c_uint8)))
  assert np.isfinite(f.correct(px)[0]).all()                                              # the family still works
