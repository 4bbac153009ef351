"""mcba_calibrate_intrinsics / k_calibrate_camera on the MI355X: against the host build of the same header (tests/intrinsic_host) run
in the device's summation order, bit-reproducibility, the warm start, the call that has nothing to do, and -- end to end -- a
bundle adjustment started from nothing but detections.

Shapes: 16-frame rigs give 6 .. 22 views per camera (above, below and not a multiple of the four waves of a workgroup), their
81-corner boards are one full 64-corner chunk plus a partial one; tiny_mixed and tiny_fishmix launch once per (coefficients,
fisheye) family; tiny_bigboard has 816 corners (13 chunks) next to an 81-corner board; masks leave a camera with 3 views (idle
waves), one with a single view and one with none."""

import numpy as np
import pytest

import intrinsic_host_lib as L
from multical_amd import _lib, tables

pytestmark = pytest.mark.gpu

RIGS = [("tiny", 16), ("tiny_pin4", 16), ("tiny_fisheye", 16), ("tiny_mixed", 16), ("tiny_fishmix", 16), ("tiny_bigboard", 8)]
HIGH_ORDER = ("rational", "thin_prism", "tilted")
_cache = {}


def view_mask_of(r):
  """Every view, except: the last camera keeps 3 views (idle waves in its workgroup).  tiny_fisheye keeps all: three views do not
  determine a Kannala-Brandt camera of that ring rig (the host build ends NOT_CONVERGED), and it is compared on parameters."""
  mask = np.ones(r.valid.shape[:3], dtype=bool)
  if r.name != "tiny_fisheye":
    seen = np.argwhere(r.valid[-1].sum(axis=2) >= 4)
    mask[-1] = False
    for f, b in seen[:3]:
      mask[-1, f, b] = True
  return mask


def solved(name, frames):
  """(rig, device result, host build in table order, host build in the device's order), computed once."""
  if name not in _cache:
    r = L.rig(name, frames=frames)
    args = (L.table_of(r), r.board_points, r.image_sizes)
    kw = dict(model=r.models, view_mask=view_mask_of(r))
    _cache[name] = (r, tables.calibrate_intrinsics(*args, **kw), L.calibrate_intrinsics(*args, **kw),
                    L.calibrate_intrinsics(*args, device_order=True, **kw))
  return _cache[name]


def tolerance(a, b):
  """max(1e-10, 100 x the host build's own difference between its two summation orders)."""
  return max(1e-10, 100 * float(np.abs(np.asarray(a) - np.asarray(b)).max()))


@pytest.mark.parametrize("name,frames", RIGS)
def test_device_equals_host_build(name, frames):
  r, dev, serial, host = solved(name, frames)
  assert np.array_equal(dev.n_used, host.n_used) and np.array_equal(dev.view_status, host.view_status)
  assert np.array_equal(dev.camera_status, host.camera_status)
  for c, model in enumerate(r.models):
    views = int((dev.view_status[c] == tables.VIEW_OK).sum())
    cost = [float(x.sse[c].sum()) for x in (dev, host, serial)]
    print(f"{name} camera {c} ({model}, {views} views): status {dev.camera_status[c]} / {host.camera_status[c]}, passes "
          f"{dev.lm_iterations[c]} / {host.lm_iterations[c]}, cost device {cost[0]:.12g} host {cost[1]:.12g} (table order {cost[2]:.12g}), "
          f"|K - K_host| {np.abs(dev.cameras[c, :4] - host.cameras[c, :4]).max():.3g} px, host orders differ by "
          f"{np.abs(host.cameras[c, :4] - serial.cameras[c, :4]).max():.3g} px")
    if model in HIGH_ORDER:
      # flat valleys: compared on cost, by the rule of the host test -- not above the lower of the yardstick's two end costs
      assert dev.camera_status[c] in (tables.CAMERA_OK, tables.CAMERA_NOT_CONVERGED)
      low = min(cost[1], cost[2])
      assert cost[0] <= low + max(1e-9 * low, 100 * abs(cost[1] - cost[2]))
      continue
    assert dev.camera_status[c] == host.camera_status[c] == tables.CAMERA_OK
    for key in ("cameras", "poses", "sse"):
      assert np.abs(dev[key][c] - host[key][c]).max() <= tolerance(host[key][c], serial[key][c]), key


def test_two_calls_return_the_same_bits():
  r, dev, _, _ = solved("tiny_mixed", 16)
  again = tables.calibrate_intrinsics(L.table_of(r), r.board_points, r.image_sizes, model=r.models, view_mask=view_mask_of(r))
  for key in ("cameras", "poses", "sse", "n_used", "view_status", "camera_status", "lm_iterations"):
    assert np.array_equal(dev[key], again[key]), key


def test_warm_start_at_the_optimum():
  r, dev, serial, host = solved("tiny", 16)
  warm = tables.calibrate_intrinsics(L.table_of(r), r.board_points, r.image_sizes, model=r.models, view_mask=view_mask_of(r),
                                     init=(dev.cameras, dev.poses))
  print("passes of the warm start", warm.lm_iterations, "cold", dev.lm_iterations)
  assert np.all(warm.camera_status == tables.CAMERA_OK) and np.all(warm.lm_iterations <= 3)
  for key in ("cameras", "poses", "sse"):
    assert np.abs(warm[key] - dev[key]).max() <= tolerance(host[key], serial[key]), key


def call_times():
  ms, n = _lib.call_ms("calibrate_intrinsics", range(4))
  return list(ms.values()), n


def test_nothing_active_touches_nothing():
  r = L.rig("tiny")
  mask = np.zeros(r.valid.shape[:3], dtype=bool)
  one = np.argwhere(r.valid[1].sum(axis=2) >= 4)[0]
  mask[1, one[0], one[1]] = True                    # camera 0: every view masked; camera 1: a single view
  out = tables.calibrate_intrinsics(L.table_of(r), r.board_points, r.image_sizes, view_mask=mask)
  assert list(out.camera_status) == [tables.CAMERA_MASKED, tables.CAMERA_TOO_FEW_VIEWS]
  assert np.all(out.view_status == tables.VIEW_MASKED) and np.all(out.cameras == 0.0) and np.all(out.n_used == 0)
  ms, n = call_times()
  assert n == 0 and ms[1] == 0.0 and ms[2] == 0.0 and ms[3] == 0.0     # no upload, no kernel, no download


def test_detections_to_bundle_adjustment_without_cameras():
  """cfg1 from nothing but detections: calibrate_single -> initialise_poses -> enable(cameras=True) -> bundle_adjust reaches the RMS
  the same bundle adjustment reaches from the fixture's own cameras and x0, within 1e-9 px (the project's residual-parity unit):
  the optimum does not depend on the start."""
  from multical_amd import calibration
  from multical_amd.workspace import Workspace
  rig = L.pnp_host_lib.golden_rig("cfg1")
  own = calibration.from_rig(rig)
  enable = dict(rig.optimize, cameras=True)
  tight = dict(tolerance=1e-15, xtol=1e-15, gtol=1e-15, max_iterations=300, solver="native")
  want = own.enable(**enable).bundle_adjust(**tight)
  ws = Workspace()
  cameras = ws.calibrate_single(own.point_table, list(own.boards), [c.image_size for c in own.cameras], camera_model='standard')
  assert ws.cameras is cameras and len(cameras) == len(own.cameras)
  # (every converged view stays: cfg1's 315-corner views nearly all hold a gross outlier corner, as in test_gpu_pose_table)
  init = ws.initialise_poses(own.point_table, list(own.boards), exclude_bad_poses=False)
  got = init.enable(**enable).bundle_adjust(**tight)
  rms = lambda c: float(np.sqrt(np.mean(np.square(c.reprojection_error))))
  print(f"cfg1: rms from detections alone {rms(got):.12f} px, from the fixture's cameras and x0 {rms(want):.12f} px, at the "
        f"initialisation {rms(init):.3f} px; intrinsic errors {ws.intrinsic_errors}")
  assert abs(rms(got) - rms(want)) <= 1e-9
