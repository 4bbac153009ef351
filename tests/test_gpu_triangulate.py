"""mcba_triangulate on the device (k_triangulate) against the g++ build of the same header (triangulate_host_lib): equal statuses and
view counts, points within 1e-8 px of whitened distance (100 x the stop rule: the device contracts to FMAs, the host build does
not), covariances to 1e-6 relative, sse and per-view errors to 1e-8 px, NaN and 0 at the same slots."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from multical_amd import _lib, triangulate

import triangulate_host_lib as th

pytestmark = pytest.mark.gpu

M_EDGES = [1, 63, 64, 65, 255, 256, 257]      # lane, wave and workgroup edges
M_MAX = max(M_EDGES)


def first_points(rig, M):
  """the first M points of every frame of a rig (the rigs are generated once, at M_MAX)"""
  Cn, F, _ = rig.shape
  return SimpleNamespace(cameras=rig.cameras, camera_poses=rig.camera_poses, rig_poses=rig.rig_poses, rig_poses_end=rig.rig_poses_end,
                         views=rig.views, views_end=rig.views_end, truth=rig.truth[:, :M], points=np.ascontiguousarray(rig.points[:, :, :M]),
                         clean=rig.clean[:, :, :M], valid=np.ascontiguousarray(rig.valid[:, :, :M]), shape=(Cn, F, M))


@functools.lru_cache(maxsize=None)
def host_result(Cn, F, rolling):
  """the host build once per rig, at M_MAX and sigma = 1 (so that inv(cov) is H): a point does not depend on its neighbours, the
  first M points of the result are the result of the first M points"""
  rig = th.make_rig(Cn, F, M_MAX, rolling)
  return rig, th.run(rig, sigma=1.0)


def compare(got, want, M, label):
  want = SimpleNamespace(points=want.points[:, :M], cov=want.cov[:, :M], sse=want.sse[:, :M], error=want.error[:, :, :M],
                         n_views=want.n_views[:, :M], status=want.status[:, :M])
  assert got.points.shape == want.points.shape and got.error.shape == want.error.shape
  assert np.array_equal(got.status, want.status) and np.array_equal(got.n_views, want.n_views), label
  ok = got.status == triangulate.OK
  assert np.array_equal(np.isnan(got.points), np.isnan(want.points)) and np.array_equal(np.isnan(got.cov), np.isnan(want.cov)), label
  assert np.array_equal(got.error == 0, want.error == 0) and np.array_equal(got.sse == 0, want.sse == 0), label
  assert not np.isnan(got.points[ok]).any()
  if not ok.any():
    return 0.0
  H = np.linalg.inv(want.cov[ok])
  d = got.points[ok] - want.points[ok]
  dist = np.sqrt(np.maximum(np.einsum('ni,nij,nj->n', d, H, d), 0.0)).max()
  cov = (np.abs(got.cov[ok] - want.cov[ok]).max(axis=(1, 2)) / np.abs(want.cov[ok]).max(axis=(1, 2))).max()
  sse, err = np.abs(got.sse - want.sse).max(), np.abs(got.error - want.error).max()
  print(f"{label}: {int(ok.sum())} of {ok.size} points; whitened distance {dist:.2e} px, cov {cov:.2e} relative, sse {sse:.2e} px^2, "
        f"err {err:.2e} px")
  assert dist <= 1e-8 and cov <= 1e-6 and sse <= 1e-8 and err <= 1e-8, label
  return dist


@pytest.mark.parametrize("M", M_EDGES)
def test_device_matches_host_build(M):
  """C in {2, 3, 8}, F in {1, 3}, static and rolling shutter at every edge of M"""
  n_ok = 0
  for Cn in (2, 3, 8):
    for F in (1, 3):
      for rolling in (False, True):
        rig, want = host_result(Cn, F, rolling)
        got = th.run(first_points(rig, M), backend="device", sigma=1.0)
        compare(got, want, M, f"C={Cn} F={F} M={M}{' rolling' if rolling else ''}")
        n_ok += int((got.status == triangulate.OK).sum())
        ms, count = triangulate.last_call_ms()
        assert count == F * M and ms["kernel"] > 0.0 and ms["call"] >= ms["kernel"]
  assert n_ok > 0


def test_sixteen_cameras_and_automatic_sigma():
  rig = th.make_rig(16, 1, 65)
  got, want = th.run(rig, backend="device"), th.run(rig)
  assert np.array_equal(got.status, want.status) and (got.status == triangulate.OK).all()
  ok = got.status == triangulate.OK
  assert (np.abs(got.cov[ok] - want.cov[ok]).max(axis=(1, 2)) / np.abs(want.cov[ok]).max(axis=(1, 2))).max() <= 1e-6
  compare(th.run(rig, backend="device", sigma=1.0), th.run(rig, sigma=1.0), 65, "C=16 F=1 M=65")
  # the statuses that end without a point, and the cap, are the host build's too
  one = th.run(rig, backend="device", max_iterations=1)
  assert (one.status == triangulate.NOT_CONVERGED).all() and np.abs(one.points - th.run(rig, max_iterations=1).points).max() <= 1e-9
  same = np.repeat(rig.views[:1], 16, axis=0)
  deg = triangulate.triangulate([rig.cameras[0]] * 16, same, np.repeat(rig.clean[:1], 16, axis=0), np.ones((16, 1, 65), dtype=bool))
  seen = rig.valid[0, 0]
  assert seen.sum() > 10 and (deg.status[0, seen] == triangulate.DEGENERATE).all() and np.isnan(deg.points[0, seen]).all()


def test_repeatable_and_scaffold():
  rig = th.make_rig(8, 3, M_MAX, True)
  a, b = th.run(rig, backend="device"), th.run(rig, backend="device")
  for k in ("points", "cov", "sse", "error", "n_views", "status"):
    assert a[k].tobytes() == b[k].tobytes(), k
  ms, count = triangulate.last_call_ms()
  assert count == 3 * M_MAX and ms["kernel"] > 0.0
  # F * M == 0 launches nothing
  empty = triangulate.triangulate(rig.cameras, rig.views, np.zeros((8, 3, 0, 2)), np.zeros((8, 3, 0), dtype=bool), views_end=rig.views_end)
  assert empty.points.shape == (3, 0, 3)
  ms, count = triangulate.last_call_ms()
  assert count == 0 and ms["kernel"] == 0.0
  # a refused call leaves its message and nothing else behind
  lib = _lib.load()
  small = th.make_rig(2, 1, 65)
  for label, change, text in (("cameras", None, b"at most 64"), ("views", "views", b"null argument"), ("heights", "views_end", b"image_heights")):
    p, out, keep = th.raw_problem(small, n_cameras=triangulate.MAX_CAMERAS + 1 if change is None else None)
    if change == "views":
      p.views = None
    if change == "views_end":
      p.views_end = p.views
    assert th.raw_call(lib.mcba_triangulate, p, out) == 1 and text in lib.mcba_last_error(), label
    c = th.run(rig, backend="device")
    assert c.points.tobytes() == a.points.tobytes() and c.cov.tobytes() == a.cov.tobytes() and c.status.tobytes() == a.status.tobytes(), label
  # NULL outputs are neither allocated nor copied: X and status alone are the full call's
  p, out, keep = th.raw_problem(small)
  assert th.raw_call(lib.mcba_triangulate, p, out) == 0
  full = th.run(small, backend="device")
  assert out["X"].tobytes() == full.points.tobytes() and out["status"].tobytes() == full.status.tobytes()


@pytest.mark.parametrize("name", ["tiny", "tiny_rolling"])
def test_reconstruction_error_on_the_device(name):
  """Calibration.reconstruction_error of the golden detections at the truth parameters: the device's equals the host build's"""
  calib = th.truth_calibration(name, noise_free=False)
  got = calib.reconstruction_error()
  with th.host_backend():
    want = calib.reconstruction_error()
  assert np.array_equal(got.valid, want.valid) and got.valid.sum() > 100
  d = np.abs(got.error - want.error).max()
  print(f"{name}: {int(got.valid.sum())} corners, median {1e3 * got.overall.quantiles[2]:.3f} mm, device - host build {d:.2e} m")
  assert d <= 1e-9
