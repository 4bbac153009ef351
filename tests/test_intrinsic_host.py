"""Intrinsic calibration (tables.calibrate_intrinsics / mcba_calibrate_intrinsics): the mathematics of
multical_amd/csrc/mcba_intrinsic.h built for the host (tests/intrinsic_host) against an independent numpy / scipy restatement
(tests/intrinsic_reference.py), and the Python mirrors of the reference's entry points (camera.calibrate_cameras' rejection loop,
top_detection_coverage).  No GPU.

Tolerances come from the restatement itself: a quantity is compared within max(floor, 100 x what the restatement's own two end
points -- started at the truth and at the truth with focal + 1 %, poses perturbed by 1e-3 -- differ by)."""
import os

import numpy as np
import pytest

import intrinsic_host_lib as L
import intrinsic_reference as R
from multical_amd import camera as camera_mod
from multical_amd import tables
from multical_amd.structs import struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ref = {}
_parity_lines = []


def restated(key, r, c, model, points=None, valid=None, fix_aspect=False, free=None, max_nfev=400):
  """The restatement's two end points of camera c (cached): struct(slots, a, b) -- a started at the truth, b at the perturbed truth."""
  if key not in _ref:
    slots, views = L.camera_views(r, c, points, valid)
    prob = R.Problem(views, model, fix_aspect=fix_aspect, free=free)
    blk = L.truth_block(r.truth.cameras[c], fix_aspect)[:5 + prob.nd]
    if free is not None:
      blk[5:][~np.asarray(free, dtype=bool)[:prob.nd]] = 0.0
    poses = L.truth_poses(r, c, slots)
    a = prob.solve(blk, poses, max_nfev)
    b = prob.solve(*L.perturbed(blk, poses), max_nfev)
    _ref[key] = struct(slots=slots, prob=prob, a=a, b=b, truth_block=blk, truth_poses=poses)
  return _ref[key]


def gaps(block_a, poses_a, block_b, poses_b):
  """(K [px], dist, rotation [rad], translation) distances between two solutions."""
  ang, tr = L.pose_gap(poses_a, poses_b)
  return (float(np.abs(block_a[:4] - block_b[:4]).max()), float(np.abs(block_a[5:] - block_b[5:]).max()), ang, tr)


# ---- 1. noise-free recovery ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,model,fix_aspect", [("tiny", "standard", False), ("tiny_pin4", "pin4", False),
                                                   ("tiny_fisheye", "fisheye", False), ("tiny", "standard", True)])
def test_noise_free_recovery(name, model, fix_aspect):
  r = L.rig(name)
  if fix_aspect:   # (a truth with one focal length)
    from types import SimpleNamespace
    cams = [SimpleNamespace(**{**vars(c), "intrinsic": np.array([[c.intrinsic[0, 0], 0, c.intrinsic[0, 2]],
                                                                  [0, c.intrinsic[0, 0], c.intrinsic[1, 2]], [0, 0, 1.0]])})
            for c in r.truth.cameras]
    r = SimpleNamespace(**{**vars(r), "truth": SimpleNamespace(**{**vars(r.truth), "cameras": cams})})
  points, ok = L.pnp_host_lib.noise_free_points(r)
  out = L.calibrate_intrinsics(L.table_of(r, points, ok), r.board_points, r.image_sizes, model=model, fix_aspect=fix_aspect)
  for c in range(len(r.image_sizes)):
    ref = restated(("free", name, model, fix_aspect, c), r, c, model, points, ok, fix_aspect)
    assert out.camera_status[c] == tables.CAMERA_OK
    assert [(f, b) for f, b in ref.slots] == [tuple(s) for s in np.argwhere(out.view_status[c] == tables.VIEW_OK)]
    own = gaps(ref.b.block, ref.b.poses, ref.truth_block, ref.truth_poses)     # the restatement's own recovery error
    got = gaps(out.cameras[c, :len(ref.truth_block)], L.host_poses(out, c, ref.slots), ref.truth_block, ref.truth_poses)
    print(f"{name} {model} fix_aspect={fix_aspect} camera {c}: (K px, dist, rot, trans) host {got} restatement {own}")
    for g, o in zip(got, own):
      assert g <= max(1e-10, 100 * o), (got, own)
    assert out.sse[c].sum() <= max(1e-16, 100 * ref.b.cost)


# ---- 2. noisy optimum ------------------------------------------------------------------------------------------------------------
NOISY = [("tiny", "standard", 0.0), ("tiny_pin4", "pin4", 0.0), ("tiny_fisheye", "fisheye", 0.0), ("tiny", "standard", 0.01)]


@pytest.mark.parametrize("name,model,outliers", NOISY)
def test_noisy_optimum(name, model, outliers):
  r = L.rig(name, outlier_frac=outliers)
  out = L.calibrate_intrinsics(L.table_of(r), r.board_points, r.image_sizes, model=model)
  for c in range(len(r.image_sizes)):
    ref = restated(("noisy", name, model, outliers, c), r, c, model)
    spread = gaps(ref.a.block, ref.a.poses, ref.b.block, ref.b.poses)
    cost_spread = abs(ref.a.cost - ref.b.cost)
    # a condition of the test: the yardstick has to be defined to 1e-7 px, else the test is mis-specified (no wider tolerance)
    assert spread[0] <= 1e-7, f"restatement's end points differ by {spread[0]:.3g} px in K on {name} camera {c}"
    assert out.camera_status[c] == tables.CAMERA_OK
    n = len(ref.truth_block)
    got = gaps(out.cameras[c, :n], L.host_poses(out, c, ref.slots), ref.a.block, ref.a.poses)
    sse = np.array([out.sse[c, f, b] for f, b in ref.slots])
    line = (f"{name:13s} {model:9s} outliers {outliers:4.2f} camera {c}: views {len(ref.slots):2d}  host - restatement  K {got[0]:.2e} px  "
            f"dist {got[1]:.2e}  rot {got[2]:.2e} rad  trans {got[3]:.2e}  cost {abs(sse.sum() - ref.a.cost):.2e} of {ref.a.cost:.6f}"
            f"   restatement's two end points  K {spread[0]:.2e}  dist {spread[1]:.2e}  rot {spread[2]:.2e}  trans {spread[3]:.2e}  "
            f"cost {cost_spread:.2e}   LM passes {int(out.lm_iterations[c])}")
    print(line)
    _parity_lines.append(line)
    for g, s in zip(got, spread):
      assert g <= max(1e-9, 100 * s), (got, spread)
    assert abs(sse.sum() - ref.a.cost) <= max(1e-9, 100 * cost_spread)
    assert np.abs(sse - ref.a.sse).max() <= max(1e-9, 100 * np.abs(ref.a.sse - ref.b.sse).max())   # (the same rule per view)
    assert [int(out.n_used[c, f, b]) for f, b in ref.slots] == [len(o) for o, _ in ref.prob.views]
  if os.environ.get("MCBA_WRITE_PROFILES") == "1" and (name, model, outliers) == NOISY[-1]:
    with open(os.path.join(ROOT, "profiles", "intrinsic_parity.txt"), "w") as fh:
      fh.write("# tests/test_intrinsic_host.py::test_noisy_optimum: the g++ build of csrc/mcba_intrinsic.h (table order) against the numpy / scipy\n"
               "# restatement (complex-step Jacobian, least_squares trf, x_scale='jac', ftol = xtol = gtol = 1e-15, then exact Gauss-Newton steps)\n"
               "# on 16-frame rigs with 0.2 px noise; the restatement's two end points: started at the truth and at the truth with focal + 1 %, poses + 1e-3\n")
      fh.write("\n".join(_parity_lines) + "\n")


# ---- 3. high-order models: flat valleys, compared on cost only ----------------------------------------------------------------------
@pytest.mark.parametrize("name,rig_model,model", [("tiny_rational", None, "rational"), ("tiny_rational", "thin_prism", "thin_prism"),
                                                  ("tiny_tilted", None, "tilted")])
def test_high_order_models_reach_the_cost(name, rig_model, model):
  r = L.rig(name, model=rig_model)
  # (2000 passes: along these valleys the damped steps are short -- the thin-prism camera 0 is 2e-5 above the restatement's cost
  #  after the default 100 passes, 3e-10 after 1000)
  out = L.calibrate_intrinsics(L.table_of(r), r.board_points, r.image_sizes, model=model, max_iterations=2000)
  nd, _, default_free = tables.INTRINSIC_MODELS[model]
  for c in range(len(r.image_sizes)):
    ref = restated(("high", name, model, c), r, c, model, free=default_free, max_nfev=200)
    assert out.camera_status[c] in (tables.CAMERA_OK, tables.CAMERA_NOT_CONVERGED)
    cost = float(sum(out.sse[c, f, b] for f, b in ref.slots))
    low = min(ref.a.cost, ref.b.cost)
    print(f"{name} {model} camera {c}: host cost {cost:.9f} ({int(out.lm_iterations[c])} passes, status {out.camera_status[c]}), "
          f"restatement {ref.a.cost:.9f} / {ref.b.cost:.9f}")
    assert cost <= low + max(1e-9 * low, 100 * abs(ref.a.cost - ref.b.cost))
    held = ~np.asarray(default_free, dtype=bool)
    assert np.all(out.cameras[c, 5:5 + nd][held] == 0.0)            # exactly their start values


# ---- 4. free_dist ------------------------------------------------------------------------------------------------------------------
def test_free_dist_holds_k3():
  r = L.rig("tiny")
  free = [1, 1, 1, 1, 0]
  out = L.calibrate_intrinsics(L.table_of(r), r.board_points, r.image_sizes, model="standard", free_dist=free)
  for c in range(len(r.image_sizes)):
    ref = restated(("k3", c), r, c, "standard", free=free)
    spread = gaps(ref.a.block, ref.a.poses, ref.b.block, ref.b.poses)
    assert spread[0] <= 1e-7
    got = gaps(out.cameras[c, :10], L.host_poses(out, c, ref.slots), ref.a.block, ref.a.poses)
    print(f"k3 held, camera {c}: host - restatement {got}, restatement's spread {spread}")
    assert out.cameras[c, 9] == 0.0
    for g, s in zip(got, spread):
      assert g <= max(1e-9, 100 * s), (got, spread)
    full = restated(("noisy", "tiny", "standard", 0.0, c), r, c, "standard")
    assert ref.a.cost > full.a.cost                                  # (a different optimum from the unconstrained one)


# ---- 5. statuses -----------------------------------------------------------------------------------------------------------------
def test_two_views_are_too_few():
  r = L.rig("tiny")
  mask = np.asarray(r.valid).sum(axis=3) >= 4
  keep = np.argwhere(mask[0])[:2]
  mask[0] = False
  for f, b in keep:
    mask[0, f, b] = True
  out = L.calibrate_intrinsics(L.table_of(r), r.board_points, r.image_sizes, view_mask=mask)
  assert out.camera_status[0] == tables.CAMERA_TOO_FEW_VIEWS and out.camera_status[1] == tables.CAMERA_OK
  assert np.all(out.view_status[0] == tables.VIEW_MASKED) and np.all(out.cameras[0] == 0.0)


def test_fronto_parallel_copies_are_not_ok():
  r = L.rig("tiny")
  cam = r.truth.cameras[0]
  X = np.asarray(r.board_points[0], dtype=np.float64)
  pose = np.array([0.0, 0.0, 0.0, -0.2, -0.2, 1.0])                  # the board square to the optical axis
  uv = R.project(cam.intrinsic[[0, 1], [0, 1]], cam.intrinsic[:2, 2], np.asarray(cam.dist), False, X + pose[3:])
  V = 5
  points, valid = np.zeros((1, V, 1, len(X), 2)), np.ones((1, V, 1, len(X)), dtype=bool)
  points[0, :, 0] = uv
  out = L.calibrate_intrinsics(struct(points=points, valid=valid), r.board_points, r.image_sizes[:1])
  assert out.camera_status[0] in (tables.CAMERA_DEGENERATE, tables.CAMERA_NOT_CONVERGED)
  # ... and the restatement's rank test says the same of this data: focal length and distance are one direction
  prob = R.Problem([(uv, X)] * V, "standard")
  s = prob.scaled_singular_values(prob.pack(L.truth_block(cam), np.tile(pose, (V, 1))))
  assert s[-1] < 1e-10 * s[0]


def test_masked_camera_leaves_its_neighbour_bit_identical():
  r = L.rig("tiny")
  both = L.calibrate_intrinsics(L.table_of(r), r.board_points, r.image_sizes)
  mask = np.ones(r.valid.shape[:3], dtype=bool)
  mask[0] = False
  one = L.calibrate_intrinsics(L.table_of(r), r.board_points, r.image_sizes, view_mask=mask)
  assert one.camera_status[0] == tables.CAMERA_MASKED and one.camera_status[1] == tables.CAMERA_OK
  for k in ("cameras", "poses", "sse", "n_used", "view_status"):
    assert np.array_equal(one[k][1], both[k][1]), k
  assert one.lm_iterations[1] == both.lm_iterations[1]


# ---- 6. the rejection loop of calibrate_cameras, with a scripted solver in place of the device call -----------------------------------
class Board(object):
  def __init__(self, n=16):
    self.points = np.stack([np.arange(n) % 4, np.arange(n) // 4, np.zeros(n)], axis=1) * 0.1
    self.num_points = n


def detections(n_frames, missing=()):
  """One board, every corner seen in every frame but `missing`: [frame][board] of struct(ids, corners)."""
  ids = np.arange(16)
  return [[struct(ids=ids if f not in missing else ids[:0], corners=np.full((16 if f not in missing else 0, 2), float(f)))]
          for f in range(n_frames)]


class Script(object):
  """Stands in for tables.calibrate_intrinsics: per-view errors are a function of (camera, frame); err of a camera = a scripted value
  per round.  Records the view sets it was called with."""

  def __init__(self, per_view, errs):
    self.per_view, self.errs, self.calls = per_view, errs, []

  def __call__(self, table, boards, image_sizes, model, fix_aspect, view_mask, init=None, free_dist=None):
    C_, F, B = view_mask.shape
    k = len(self.calls)
    self.calls.append(dict(views=[sorted(int(f) for f in np.flatnonzero(view_mask[c, :, 0])) for c in range(C_)], warm=init is not None))
    assert np.array_equal(view_mask, np.asarray(table.valid).any(axis=3) & view_mask)
    assert init is None or (init[0].shape[0] == C_ and init[1].shape == (C_, F, B, 4, 4))   # the warm start fits this round's table
    epv = np.zeros((C_, F, B))
    for c in range(C_):
      for f in range(F):
        epv[c, f, 0] = self.per_view(c, f)
    cams = np.zeros((C_, 10))
    cams[:, :4] = [[100.0 + k, 101.0 + k, 50.0, 40.0]] * C_
    status = np.where(view_mask.any(axis=(1, 2)), tables.CAMERA_OK, tables.CAMERA_MASKED)
    return struct(cameras=cams, camera_n_dist=np.full(C_, 5), poses=np.tile(np.eye(4), (C_, F, B, 1, 1)),
                  error=np.array([self.errs[c][min(k, len(self.errs[c]) - 1)] for c in range(C_)]), error_perview=epv,
                  camera_status=status, view_status=np.where(view_mask, tables.VIEW_OK, tables.VIEW_MASKED))


def test_rejection_loop_quantile_rounds(monkeypatch):
  # 20 views: err 1.234 -> rounded 1.23 >= 1.0: the views below the 0.95 quantile stay (19); err 0.996 -> 1.00 still >= 1.0 -> 18;
  # err 0.994 -> 0.99: finished -- and the views are cut once more after the last solve, as in the reference
  script = Script(lambda c, f: 0.1 * (f + 1), [[1.234, 0.996, 0.994]])
  monkeypatch.setattr(camera_mod, "_solve", script)
  cams, errs = camera_mod.calibrate_cameras([Board()], [detections(20)], [(640, 480)], 1.0)
  assert [c["views"][0] for c in script.calls] == [list(range(20)), list(range(19)), list(range(18))]
  assert [c["warm"] for c in script.calls] == [False, True, True]
  assert errs == [0.99] and cams[0].intrinsic[0, 0] == 102.0
  assert len(cams[0].error_perview) == 18 and cams[0].intrinsic_dataset["image_ids"] == list(range(17))
  assert cams[0].intrinsic_dataset["board_ids"] == [0.0] * 17


def test_rejection_loop_few_views_raise_the_limit(monkeypatch):
  script = Script(lambda c, f: 1.0, [[1.25]])
  monkeypatch.setattr(camera_mod, "_solve", script)
  cams, errs = camera_mod.calibrate_cameras([Board()], [detections(10)], [(640, 480)], 1.0)
  assert len(script.calls) == 1                                      # no second solve on unchanged data
  assert errs == [1.25] and len(cams[0].error_perview) == 10         # (not rounded: fewer than 15 views)
  cam, err = camera_mod.Camera.calibrate([Board()], 1.0, detections(10), (640, 480))
  assert err == 1.25 and cam.image_size == (640, 480) and "error_perview" not in cam.__getstate__()


def test_rejection_loop_batch_finishes_cameras_apart(monkeypatch):
  # camera 0 is done after the first round, camera 1 needs a second one: camera 0 is masked out of it
  script = Script(lambda c, f: 0.1 * (f + 1), [[0.5], [1.5, 0.7]])
  monkeypatch.setattr(camera_mod, "_solve", script)
  cams, errs = camera_mod.calibrate_cameras([Board()], [detections(16), detections(16, missing=(3,))], [(640, 480)] * 2, 1.0)
  assert script.calls[0]["views"] == [list(range(16)), [f for f in range(16) if f != 3]]
  assert script.calls[1]["views"] == [[], [f for f in range(15) if f != 3]]
  assert len(script.calls) == 2 and errs == [0.5, 0.7]
  assert cams[0].intrinsic[0, 0] == 100.0 and cams[1].intrinsic[0, 0] == 101.0


def test_rejection_rounds_with_the_real_solver_drop_the_last_frame(monkeypatch):
  """calibrate_single over the host build: several warm-started rejection rounds in which the LAST frame is among the dropped
  views (the table keeps its number of frames), beside a view of collinear corners that never gets a start pose."""
  from multical_amd.workspace import Workspace
  r = L.rig("tiny", frames=48)
  points, valid = r.points.copy(), r.valid.copy()
  last = valid.shape[1] - 1
  seen = np.argwhere(valid[0, :, 0].sum(axis=1) >= 4).ravel()
  src = seen[0]
  noise = np.random.default_rng(7).normal(0, 3.0, points[0, src].shape)           # (a constant offset would go into the pose)
  points[0, last], valid[0, last] = points[0, src] + noise, valid[0, src]         # camera 0: its last frame is 3 px noisier
  row = np.flatnonzero(valid[1, src, 0])
  row = row[row < 9]                                                              # camera 1, frame `src`: one row of the board
  assert len(row) >= 4
  valid[1, src, 0] = False
  valid[1, src, 0, row] = True
  calls = []

  def solver(table, boards, image_sizes, **kw):
    out = L.calibrate_intrinsics(table, boards, image_sizes, **kw)
    calls.append((kw["view_mask"].copy(), kw.get("init") is not None, out, table))
    return out

  monkeypatch.setattr(camera_mod, "_solve", solver)
  ws = Workspace()
  boards = [Board.__new__(Board) for _ in r.board_points]
  for b, pts in zip(boards, r.board_points):
    b.points, b.num_points = np.asarray(pts), len(pts)
  cams = ws.calibrate_single(struct(points=points, valid=valid), boards, r.image_sizes, intrinsic_error_limit=0.1)
  assert len(calls) >= 3 and [w for _, w, _, _ in calls] == [False] + [True] * (len(calls) - 1)
  assert all(m.shape == valid.shape[:3] for m, _, _, _ in calls)
  assert calls[0][0][0, last, 0] and not calls[1][0][0, last, 0]                  # the last frame went in the first cut
  assert calls[0][2].view_status[1, src, 0] == tables.VIEW_DEGENERATE and not calls[1][0][1, src, 0]
  assert last not in cams[0].intrinsic_dataset["image_ids"] and src not in cams[1].intrinsic_dataset["image_ids"]
  # the warm-started rounds end where a cold solve of the same views ends
  for c, cam in enumerate(cams):
    k = max(i for i, (m, _, _, _) in enumerate(calls) if m[c].any())
    cold = L.calibrate_intrinsics(calls[k][3], boards, r.image_sizes, view_mask=calls[k][0])   # (the round's table: float32 corners)
    got = np.array([cam.intrinsic[0, 0], cam.intrinsic[1, 1], cam.intrinsic[0, 2], cam.intrinsic[1, 2]])
    print(f"camera {c}: {len(calls)} rounds, {int(calls[k][0][c].sum())} views in its last, warm - cold {np.abs(got - cold.cameras[c, :4]).max():.2e} px")
    assert np.abs(got - cold.cameras[c, :4]).max() <= 1e-9 and np.abs(cam.dist - cold.cameras[c, 5:10]).max() <= 1e-9


# ---- 7. top_detection_coverage -------------------------------------------------------------------------------------------------------
def test_top_detection_coverage_is_deterministic_bin_coverage():
  size = (100, 80)
  corners = [np.array([[5.0, 5.0], [6.0, 6.0]]),                                  # one bin
             np.array([[5.0, 5.0], [55.0, 5.0], [95.0, 75.0]]),                   # three
             np.array([[5.0, 5.0], [55.0, 45.0]]),                                # two
             np.array([[15.0, 5.0], [55.0, 45.0], [95.0, 5.0]])]                  # three (ties keep their order)
  views = struct(corners=corners, ids=[np.arange(len(c)) for c in corners], object_points=[None] * 4, board_offset=[0.0] * 4,
                 image_ids=[0, 1, 2, 3])
  bins = camera_mod.image_bins(size)
  assert [len(b) for b in bins] == [12, 10]                            # bin size 8: linspace(0, 100, 12), linspace(0, 80, 10)
  direct = []
  for c in corners:
    ix = np.searchsorted(bins[0], c[:, 0], side='right') - 1
    iy = np.searchsorted(bins[1], c[:, 1], side='right') - 1
    direct.append(len(set(zip(ix.tolist(), iy.tolist()))))
  assert direct == [1, 3, 2, 3] and [camera_mod.coverage(c, bins) for c in corners] == direct
  top = camera_mod.top_detection_coverage(views, 3, size)
  assert top.image_ids == [1, 3, 2] and camera_mod.top_detection_coverage(views, 3, size).image_ids == top.image_ids
  assert all(a is b for a, b in zip(top.corners, [corners[1], corners[3], corners[2]]))
  jittered = camera_mod.top_detection_coverage(views, 4, size, rng=np.random.default_rng(0))
  assert sorted(jittered.image_ids) == [0, 1, 2, 3]
