"""The projection difference of two calibrations: the g++ build of csrc/mcba_projdiff.h (projdiff_host_lib) against
an independent numpy / scipy restatement (projdiff_reference.py), the reader of exported calibrations, and a stand-alone sanitizer
program.  No GPU.  Measured values: profiles/projection_diff_parity.txt."""
import functools
import json

import numpy as np
import pytest

import host_build
from multical_amd import compare, export, import_calib, synthetic, uncertainty

import projdiff_host_lib as pl
import projdiff_reference as ref
from util import mirror

CAMERAS = list(range(9))
MODES = [(compare.NONE, 0), (compare.ROTATION, 3), (compare.RIGID, 6)]
PLANTED = np.array([3e-3, -2e-3, 1.5e-3, 2e-3, -1e-3, 1.5e-3])       # a few mrad, a few mm
FIT_PIXELS = pl.inner_pixels(48, 3)
QUERY_PIXELS = pl.inner_pixels(12, 4)


@functools.lru_cache(maxsize=None)
def rays0(b):
  """the restatement's rays of the shared fit pixels through camera b of calibration 0 (computed once, unchanged)"""
  Y, ok = ref.unit_rays(pl.rigs()[0].cameras[b], FIT_PIXELS)
  assert ok.all()
  return Y


def distance_of(rho):
  return np.inf if rho == 0 else 1.0 / rho


# ---- identical calibrations -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", CAMERAS)
def test_identical_calibrations(b):
  rig0 = pl.rigs()[0]
  jobs = [pl.fit_job(b, np.inf, compare.ROTATION), pl.fit_job(b, 2.0, compare.RIGID), compare.Job(b, b, 2.0, pixels=pl.spread_pixels(40, b))]
  r = pl.run(jobs, pair=(rig0, rig0))
  assert (r.fit_info[:, 4] == compare.FIT_OK).all()
  assert np.abs(r.transform).max() < 1e-12
  n = jobs[0].n + jobs[1].n
  ok = r.status[:n] == compare.OK
  assert ok.any() and np.abs(r.diff[:n][ok]).max() <= 1e-9 and r.magnitude[:n][ok].max() <= 1e-9
  same = r.status[n:] == compare.OK
  assert same.any() and (r.diff[n:][same] == 0).all() and (r.magnitude[n:][same] == 0).all()
  assert np.array_equal(r.landing[n:][same], jobs[2].pixels[same])
  assert np.isnan(r.diff[n:][~same]).all()


# ---- the header's fit function on a planted transform ------------------------------------------------------------------------
@pytest.mark.parametrize("b", CAMERAS)
def test_planted_transform_is_recovered(b):
  worst = 0.0
  for mode, rho in ((compare.ROTATION, 0.0), (compare.RIGID, 0.5), (compare.RIGID, 2.0)):
    K = 3 if mode == compare.ROTATION else 6
    planted = np.where(np.arange(6) < K, PLANTED, 0.0)
    fit, valid = pl.fit_planted(pl.fit_job(b, distance_of(rho), mode, fit_pixels=pl.inner_pixels(200, b)), planted)
    assert fit[10] == compare.FIT_OK and valid.all() and fit[6] == 200
    err = np.abs(fit[:6] - planted).max()
    worst = max(worst, err)
    print(f"camera {b} mode {mode} rho {rho}: |transform - planted| {err:.3g} after {int(fit[7])} linearisations, rms {fit[8]:.3g} -> {fit[9]:.3g}")
    assert err <= 1e-11 and fit[9] <= 1e-9
  print(f"camera {b}: worst {worst:.3g}")


# ---- against the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", CAMERAS)
def test_fit_and_map_against_the_restatement(b):
  rig0, rig1 = pl.rigs()
  cam0, cam1 = rig0.cameras[b], rig1.cameras[b]
  Y = rays0(b)
  worst_t = worst_d = 0.0
  for rho in (0.0, 0.5, 2.0):
    for mode, K in MODES:
      if mode == compare.RIGID and rho == 0.0:
        continue
      r = pl.run([pl.fit_job(b, distance_of(rho), mode, fit_pixels=FIT_PIXELS, pixels=QUERY_PIXELS)])
      assert r.fit_info[0, 4] == compare.FIT_OK and (r.status == compare.OK).all()
      assert mode == compare.NONE or r.fit_info[0, 0] == len(FIT_PIXELS)
      want = ref.fit_transform(cam1, Y, FIT_PIXELS, rho, K, "trf")
      other = ref.fit_transform(cam1, Y, FIT_PIXELS, rho, K, "lm")
      spread = ref.displacement(cam1, Y, rho, want, other)
      got = ref.displacement(cam1, Y, rho, r.transform[0], want)
      bound = max(1e-9, 100.0 * spread)
      d = np.abs(ref.intrinsic_diff(cam0, cam1, r.transform[0], rho, QUERY_PIXELS) - r.diff).max()
      worst_t, worst_d = max(worst_t, got / bound), max(worst_d, d)
      print(f"camera {b} rho {rho} mode {mode}: transform displacement {got:.3g} px (restatement's spread {spread:.3g}), "
            f"diff given the transform {d:.3g} px, rms {r.fit_info[0, 2]:.4f} -> {r.fit_info[0, 3]:.4f}")
      assert got <= bound
      assert d <= 1e-9
      assert np.array_equal(r.magnitude, np.sqrt(r.diff[:, 0] * r.diff[:, 0] + r.diff[:, 1] * r.diff[:, 1]))
      if mode != compare.NONE:
        rms = np.sqrt((ref.intrinsic_diff(cam0, cam1, r.transform[0], rho, FIT_PIXELS) ** 2).sum() / len(FIT_PIXELS))
        assert abs(rms - r.fit_info[0, 3]) <= 1e-9
  print(f"camera {b}: worst transform displacement / bound {worst_t:.3g}, worst diff {worst_d:.3g} px")


def test_cross_family_eight_coefficients_for_five():
  """calibration 1 is the restatement's own 8-coefficient least-squares fit of the 5-coefficient camera 0 (to its pixels displaced by
  a smooth 0.3 px pattern, so that the fit has something to absorb)"""
  from types import SimpleNamespace
  rig0 = pl.rigs()[0]
  grid = compare.Job._grid_array(uncertainty.grid_of(pl.IMAGE_SIZE, (12, 9)))
  K, dist = ref.fit_camera(rig0.cameras[0], 8, grid, grid + 0.3 * np.sin(grid / 40.0))
  cam1 = SimpleNamespace(intrinsic=K, dist=dist, image_size=pl.IMAGE_SIZE, fix_aspect=False)
  rig1 = uncertainty.RigModel([cam1], rig0.poses[:1])
  first = uncertainty.RigModel([pl.ul.source_cameras()[0]], rig0.poses[:1])
  assert rig1.n_dist == [8] and first.n_dist == [5]
  for mode, K_, rho in ((compare.ROTATION, 3, 0.0), (compare.RIGID, 6, 0.5)):
    r = pl.run([pl.fit_job(0, distance_of(rho), mode, fit_pixels=FIT_PIXELS, pixels=QUERY_PIXELS)], pair=(first, rig1))
    assert r.fit_info[0, 4] == compare.FIT_OK and (r.status == compare.OK).all()
    want = ref.fit_transform(rig1.cameras[0], rays0(0), FIT_PIXELS, rho, K_, "trf")
    other = ref.fit_transform(rig1.cameras[0], rays0(0), FIT_PIXELS, rho, K_, "lm")
    bound = max(1e-9, 100.0 * ref.displacement(rig1.cameras[0], rays0(0), rho, want, other))
    got = ref.displacement(rig1.cameras[0], rays0(0), rho, r.transform[0], want)
    d = np.abs(ref.intrinsic_diff(first.cameras[0], rig1.cameras[0], r.transform[0], rho, QUERY_PIXELS) - r.diff).max()
    print(f"8 for 5, mode {mode}: displacement {got:.3g} px (bound {bound:.3g}), diff {d:.3g} px, |diff| up to {r.magnitude.max():.3f} px")
    assert got <= bound and d <= 1e-9 and r.magnitude.max() > 1e-3


# ---- the focus disc ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,distance", [(compare.ROTATION, np.inf), (compare.RIGID, 2.0)])
def test_focus_disc_is_the_list_of_the_pixels_inside(mode, distance):
  focus = (110.0, 70.0, 42.5)
  disc = pl.fit_job(4, distance, mode, focus=focus)
  px = disc.fit_pixel_array()
  inside = ((px - focus[:2]) ** 2).sum(axis=1) <= focus[2] ** 2
  assert 100 < inside.sum() < len(px)
  listed = pl.fit_job(4, distance, mode, fit_pixels=px[inside])
  whole = pl.fit_job(4, distance, mode)
  r = pl.run([disc, listed, whole])
  assert (r.fit_info[:, 4] == compare.FIT_OK).all() and r.fit_info[0, 0] == r.fit_info[1, 0] == inside.sum()
  assert np.abs(r.transform[0] - r.transform[1]).max() <= 1e-12 and np.abs(r.fit_info[0, 2:4] - r.fit_info[1, 2:4]).max() <= 1e-12
  n = disc.n
  assert np.abs(r.diff[:n] - r.diff[n:2 * n]).max() <= 1e-12
  assert np.abs(r.transform[0] - r.transform[2]).max() > 1e-6          # (the disc matters)
  again = pl.run([pl.fit_job(4, distance, mode, focus=(0.0, 0.0, -1.0))])
  assert again.transform.tobytes() == r.transform[2:].tobytes()        # (a radius <= 0: the whole image)


# ---- statuses --------------------------------------------------------------------------------------------------------------------
def test_too_few_fit_pixels_and_queries_of_a_failed_fit():
  px = pl.inner_pixels(3, 1)
  far = np.array([[5000.0, 4000.0]])
  jobs = [pl.fit_job(1, np.inf, compare.ROTATION, fit_pixels=px[:1], pixels=px),
          pl.fit_job(1, np.inf, compare.ROTATION, fit_pixels=px[:2], pixels=px),
          pl.fit_job(1, 2.0, compare.RIGID, fit_pixels=px[:2], pixels=px),
          pl.fit_job(1, 2.0, compare.RIGID, fit_pixels=px[:3], pixels=px),
          pl.fit_job(5, np.inf, compare.ROTATION, fit_pixels=np.concatenate([px[:1], far, far]), pixels=px),
          pl.fit_job(1, np.inf, compare.ROTATION, fit_pixels=np.zeros((0, 2)), pixels=px)]
  r = pl.run(jobs)
  assert r.fit_info[:, 4].tolist() == [compare.FIT_TOO_FEW, compare.FIT_OK, compare.FIT_TOO_FEW, compare.FIT_OK, compare.FIT_TOO_FEW,
                                       compare.FIT_TOO_FEW]
  assert r.fit_info[:, 0].tolist() == [1, 2, 2, 3, 1, 0]
  status = r.status.reshape(6, 3)
  for j in (0, 2, 4, 5):
    assert (status[j] == compare.NO_FIT).all() and np.isnan(r.diff[3 * j:3 * j + 3]).all() and np.isnan(r.magnitude[3 * j:3 * j + 3]).all()
    assert np.isnan(r.transform[j]).all() and np.isnan(r.fit_info[j, 3])
  for j in (1, 3):
    assert (status[j] == compare.OK).all() and np.isfinite(r.diff[3 * j:3 * j + 3]).all() and np.isfinite(r.transform[j]).all()
  assert np.isnan(r.landing).all()                                       # (no transfer job)


def test_fit_pixels_outside_the_fisheye_range_are_left_out():
  """pixels no fisheye camera has produced (the inverse does not converge) do not change the fit of the rest"""
  px = pl.inner_pixels(40, 2)
  far = np.array([[5000.0, 4000.0], [-3000.0, 9000.0], [np.nan, 3.0]])
  mixed = np.concatenate([px[:20], far, px[20:]])
  r = pl.run([pl.fit_job(5, np.inf, compare.ROTATION, fit_pixels=px), pl.fit_job(5, np.inf, compare.ROTATION, fit_pixels=mixed),
              pl.fit_job(5, 2.0, compare.RIGID, fit_pixels=px), pl.fit_job(5, 2.0, compare.RIGID, fit_pixels=mixed)])
  assert (r.fit_info[:, 4] == compare.FIT_OK).all() and (r.fit_info[:, 0] == 40).all()
  assert r.transform[0].tobytes() == r.transform[1].tobytes() and r.transform[2].tobytes() == r.transform[3].tobytes()
  fit, valid = pl.fit_planted(pl.fit_job(5, np.inf, compare.ROTATION, fit_pixels=mixed), PLANTED * [1, 1, 1, 0, 0, 0])
  assert valid.tolist() == [True] * 20 + [False] * 3 + [True] * 20


def test_behind_and_not_converged_in_transfer_jobs():
  rig0, rig1 = pl.rigs()
  turned = rig1.poses.copy()
  turned[2] = np.diag([-1.0, 1.0, -1.0, 1.0]) @ turned[2]               # camera 2 looks the other way under calibration 1
  pair = (rig0, uncertainty.RigModel(pl._rigs[2], turned))
  px = np.array([[99.5, 74.5], [5000.0, 4000.0], [np.nan, 10.0]])
  r = pl.run([compare.Job(2, 0, 1.0, pixels=px), compare.Job(0, 5, 1.0, pixels=px), compare.Job(1, 0, 1.0, pixels=px)], pair=pair)
  s = r.status.reshape(3, 3)
  assert s[0, 0] == compare.BEHIND and s[1, 1] == compare.NOT_CONVERGED and s[2, 0] == compare.OK and (s[:, 2] == compare.NOT_CONVERGED).all()
  bad = r.status != compare.OK
  assert np.isnan(r.diff[bad]).all() and np.isnan(r.landing[bad]).all() and np.isnan(r.magnitude[bad]).all()
  assert np.isfinite(r.diff[~bad]).all() and np.isfinite(r.landing[~bad]).all()


def test_refused_calls_name_the_argument():
  px = pl.inner_pixels(4, 1)
  with pytest.raises(RuntimeError, match="mcba_projection_diff: job 0: a rigid fit needs a finite distance"):
    pl.run([pl.fit_job(0, np.inf, compare.RIGID, fit_pixels=px, pixels=px)])
  with pytest.raises(RuntimeError, match="mcba_projection_diff: job 1: inv_distance must be finite and >= 0"):
    pl.run([pl.fit_job(0, 2.0, compare.RIGID), pl.fit_job(0, -2.0, compare.ROTATION)])
  with pytest.raises(RuntimeError, match="fit grid of 65792 pixels, at most 65536 are served"):
    pl.run([compare.Job(0, None, np.inf, compare.ROTATION, fit_grid=uncertainty.grid_of(pl.IMAGE_SIZE, (257, 256)), pixels=px)])
  with pytest.raises(RuntimeError, match="reference 9 of 9"):
    pl.run([compare.Job(0, 9, 1.0, pixels=px)])
  with pytest.raises(RuntimeError, match="fit mode 7"):
    pl.run([compare.Job(0, None, 1.0, 7, fit_pixels=px, pixels=px)])
  with pytest.raises(ValueError, match="a rigid fit needs a finite distance"):
    rig0, rig1 = pl.rigs()
    pl.on_host(compare.projection_diff, pl.ul.source_cameras(), rig0.poses, pl._rigs[2], rig1.poses, fit="rigid")
  empty = pl.run([pl.fit_job(0, np.inf, compare.ROTATION, pixels=np.zeros((0, 2)))])     # no query: nothing runs
  assert empty.diff.shape == (0, 2) and (empty.transform == 0).all() and empty.fit_info[0, 0] == 0


# ---- transfer mode ---------------------------------------------------------------------------------------------------------------
def test_transfer_against_the_restatement():
  rig0, rig1 = pl.rigs()
  cams = (0, 4, 5)                                                       # 5 coefficients, tilted 14, fisheye
  worst = 0.0
  for rho in (0.0, 0.5):
    pairs = [(b, a) for b in cams for a in cams if a != b]
    r = pl.run([compare.Job(b, a, distance_of(rho), pixels=QUERY_PIXELS) for b, a in pairs])
    for k, (b, a) in enumerate(pairs):
      sl = slice(k * len(QUERY_PIXELS), (k + 1) * len(QUERY_PIXELS))
      ok = r.status[sl] == compare.OK
      assert ok.any(), (b, a)
      diff, landing = ref.transfer_diff(rig0, rig1, b, a, rho, QUERY_PIXELS)
      e = max(np.abs(diff[ok] - r.diff[sl][ok]).max(), np.abs(landing[ok] - r.landing[sl][ok]).max())
      worst = max(worst, e)
      assert e <= 1e-9, (b, a, rho, e)
  print(f"transfer, every ordered pair of cameras {cams}: worst |diff|, |landing| error {worst:.3g} px")


def test_functional_entry_shapes_and_defaults():
  rig0, rig1 = pl.rigs()
  cams0, cams1 = pl.ul.source_cameras(), pl._rigs[2]
  r = pl.on_host(compare.projection_diff, cams0, rig0.poses, cams1, rig1.poses, query_cameras=[1, 4], grid=(5, 4))
  assert r.diff.shape == (2, 4, 5, 2) and r.magnitude.shape == (2, 4, 5) and r.landing.shape == (2, 4, 5, 2) and r.transform.shape == (2, 6)
  assert (r.transform[:, 3:] == 0).all() and (r.fit.n_fit == 2400).all() and (r.fit.status == compare.FIT_OK).all()   # auto: rotation
  near = pl.on_host(compare.projection_diff, cams0, rig0.poses, cams1, rig1.poses, query_cameras=[1], distance=2.0, pixels=QUERY_PIXELS)
  assert near.diff.shape == (12, 2) and (near.transform[0, 3:] != 0).all()                                           # auto: rigid
  t = pl.on_host(compare.projection_diff, cams0, rig0.poses, cams1, rig1.poses, reference=0, grid=(3, 2))
  assert t.landing.shape == (9, 2, 3, 2) and (t.diff[0] == 0).all() and (t.fit.n_fit == 0).all()
  d = compare.significance(np.array([[3.0, 4.0]]), np.array([[[2.0, 0.0], [0.0, 8.0]]]), np.array([[[2.0, 0.0], [0.0, 8.0]]]))
  assert abs(d[0] - np.sqrt(9.0 / 4.0 + 16.0 / 16.0)) < 1e-15


# ---- import_calib ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "tiny_fisheye"])
@pytest.mark.parametrize("master", [None, "cam1"])
def test_export_then_load_round_trip(tmp_path, name, master):
  c = mirror(synthetic.make_rig(name))
  names = dict(camera=list(c.camera_poses.names))
  path = str(tmp_path / "calibration.json")
  export.export(path, c, names, [], master=master)
  fisheye = names["camera"] if name == "tiny_fisheye" else None
  got = import_calib.load_calibration(path, fisheye=fisheye)
  want = c if master is None else c.with_master(master)
  poses = np.asarray(want.camera_poses.poses)
  assert got.names == names["camera"]
  for i, cam in enumerate(got.cameras):
    src = want.cameras[i]
    assert np.asarray(cam.intrinsic).tobytes() == np.asarray(src.intrinsic, dtype=np.float64).tobytes()
    assert np.asarray(cam.dist).tobytes() == np.asarray(src.dist, dtype=np.float64).tobytes()
    assert tuple(cam.image_size) == tuple(src.image_size) and cam.model == src.model
    assert type(cam).__name__ == type(src).__name__
  if master is None:
    assert got.camera_poses.tobytes() == poses.tobytes()
  else:
    m = names["camera"].index(master)
    assert got.camera_poses[m].tobytes() == poses[m].tobytes()
    for i in range(len(poses)):                     # the file states T_i T_m^-1 beside T_m: T_i is their product, formed once
      want_i = poses[i] if i == m or np.array_equal(poses[m], np.eye(4)) else poses[i] @ poses[m]
      assert got.camera_poses[i].tobytes() == want_i.tobytes()
      assert np.abs(got.camera_poses[i] - poses[i]).max() <= 4 * np.finfo(np.float64).eps * max(1.0, np.abs(poses[i]).max())
  with open(path) as f:
    data = json.load(f)
  assert all(("_to_" in k) == (master is not None and k != master) for k in data["camera_poses"])


def test_a_missing_pose_and_an_inconsistent_loop_raise():
  c = mirror(synthetic.make_rig("tiny"))
  names = list(c.camera_poses.names)
  data = export.export_json(c, dict(camera=names), [])
  lost = json.loads(json.dumps(data))
  del lost["camera_poses"][names[1]]
  with pytest.raises(ValueError, match="no camera pose for"):
    import_calib.import_cameras(lost)
  chained = json.loads(json.dumps(data))                                  # cam1 by a relative entry only: found through the graph
  P = np.asarray(c.camera_poses.poses)
  M = P[1] @ np.linalg.inv(P[0])
  del chained["camera_poses"][names[1]]
  chained["camera_poses"][f"{names[1]}_to_{names[0]}"] = dict(R=M[:3, :3].tolist(), T=M[:3, 3].tolist())
  assert np.abs(import_calib.import_cameras(chained).camera_poses[1] - P[1]).max() < 1e-14
  looped = json.loads(json.dumps(data))                                   # an absolute pose AND a relative entry that disagrees
  M[:3, 3] += 1e-3
  looped["camera_poses"][f"{names[1]}_to_{names[0]}"] = dict(R=M[:3, :3].tolist(), T=M[:3, 3].tolist())
  with pytest.raises(ValueError, match="inconsistent camera poses"):
    import_calib.import_cameras(looped)
  stray = json.loads(json.dumps(data))
  stray["camera_poses"]["nobody_to_cam0"] = stray["camera_poses"][names[0]]
  with pytest.raises(ValueError, match="names no camera"):
    import_calib.import_cameras(stray)


# ---- sanitizer ---------------------------------------------------------------------------------------------------------------------
def test_sanitized_program(tmp_path):
  """the smallest, odd and failing cases once more in a stand-alone program under AddressSanitizer + UBSan (CPU only, nothing loaded
  into Python)"""
  r = host_build.sanitized_program("projdiff_host", "projdiff_sanitize_main.cpp", tmp_path)
  assert r.returncode == 0 and "projdiff sanitize run: ok" in r.stdout, r.stdout + r.stderr
