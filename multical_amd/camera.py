"""Cameras as parameter blocks (multical/camera.py:27-171, multical/camera_fisheye.py:28-160).

The bundle-adjustment face of the reference classes: intrinsic matrix + distortion <-> parameter vector [fx fy | cx cy | skew |
dist].  The projection lives in the HIP kernels (csrc/mcba_math.h: project_point) -- there is no OpenCV in this package; `project`,
`undistort_points`, `undistort_map` and `undistort_images` (camera.py:113-128, 244-258) are calls into them (undistort.py).  Intrinsic calibration (Camera.calibrate, CameraFisheye.calibrate, calibrate_cameras: camera.py:69-105,
229-241, camera_fisheye.py:71-94) runs on the device: tables.calibrate_intrinsics solves all cameras of a round in one call.
"""
from functools import cached_property
import numpy as np
from .parameters import Parameters
from .structs import struct

DIST_SIZES = dict(standard=(4, 5), rational=(8,), thin_prism=(12,), tilted=(14,))


class Camera(Parameters):
  model_names = ("standard", "rational", "tilted", "thin_prism")

  def __init__(self, image_size, intrinsic, dist, model='standard', fix_aspect=False, has_skew=False, error_perview=None,
               intrinsic_dataset=None):
    assert model in self.model_names, f"unknown camera model {model} options are {list(self.model_names)}"
    self.model = model
    self.error_perview = error_perview                                               # (optional: outside __getstate__,
    self.intrinsic_dataset = {} if intrinsic_dataset is None else intrinsic_dataset  #  as in the reference)
    self.image_size = tuple(image_size)
    self.intrinsic = np.asarray(intrinsic, dtype=np.float64)
    self.dist = np.zeros(5) if dist is None else np.asarray(dist, dtype=np.float64)
    self.fix_aspect = fix_aspect
    self.has_skew = has_skew

  @property
  def focal_length(self):
    return np.array([self.intrinsic[0, 0], self.intrinsic[1, 1]])

  @property
  def principle_point(self):
    return np.array([self.intrinsic[0, 2], self.intrinsic[1, 2]])

  @property
  def skew(self):
    return self.intrinsic[0, 1] if self.has_skew else 0.0

  @cached_property
  def params(self):
    f = self.focal_length
    if self.fix_aspect:
      f = np.array([f.mean(), f.mean()])
    return struct(focal_length=f, principle_point=self.principle_point, skew=np.array([self.skew]),
                  dist=np.asarray(self.dist))

  def with_params(self, params):
    f = params.focal_length
    fx, fy = f if not self.fix_aspect else (f[0], f[0])
    px, py = params.principle_point
    skew, = params.skew
    intrinsic = np.array([[fx, skew, px], [0, fy, py], [0, 0, 1]])
    return self.copy(intrinsic=intrinsic, dist=params.dist)

  def scale_image(self, factor):
    intrinsic = self.intrinsic.copy()
    intrinsic[:2] *= factor
    return self.copy(intrinsic=intrinsic)

  def project(self, points):
    """camera.py:124-128: pixels [..., 2] of camera-frame points [..., 3] (on the device: undistort.project_points)."""
    from . import undistort
    points = np.asarray(points, dtype=np.float64)
    return undistort.project_points([self], points.reshape(-1, 3)).reshape(*points.shape[:-1], 2)

  def undistort_points(self, points):
    """camera.py:119-122 (cv2.undistortPoints(points, K, dist, P=K)): pixels [..., 2] -> the pixels of the distortion-free camera
    with the same matrix.  The exact inverse of `project`; a pixel outside the model's range comes back NaN."""
    from . import undistort
    points = np.asarray(points, dtype=np.float64)
    out, _ = undistort.undistort_points([self], points.reshape(-1, 2), P=self.intrinsic)
    return out.reshape(*points.shape[:-1], 2)

  @cached_property
  def undistort_map(self):
    """camera.py:113-117 (cv2.initUndistortRectifyMap(K, dist, None, K, image_size, CV_32FC2)): [H, W, 2] float32.  Cached on the
    instance, not part of its state."""
    from . import undistort
    return undistort.undistort_maps([self], self.image_size)[0]

  def __getstate__(self):
    return dict(image_size=self.image_size, intrinsic=self.intrinsic, dist=self.dist, fix_aspect=self.fix_aspect,
                has_skew=self.has_skew, model=self.model)

  def __setstate__(self, d):
    self.__dict__.update(d)

  def copy(self, **k):
    d = self.__getstate__()
    d.update(k)
    return self.__class__(**d)

  @staticmethod
  def calibrate(boards, intrinsic_error_limit, detections, image_size, max_iter=10, eps=1e-3, model='standard', fix_aspect=False,
                has_skew=False, flags=0, max_images=None):
    """camera.py:69-105 for one camera: (camera, err).  See calibrate_cameras for what differs from the reference."""
    cams, errs = calibrate_cameras(boards, [detections], [image_size], intrinsic_error_limit, max_iter=max_iter, eps=eps,
                                   model=model, fix_aspect=fix_aspect, has_skew=has_skew, flags=flags, max_images=max_images)
    return cams[0], errs[0]

  def __repr__(self):
    return f"{type(self).__name__}(image_size={self.image_size}, intrinsic={self.intrinsic.tolist()}, dist={self.dist.tolist()})"


class CameraFisheye(Camera):
  """Kannala-Brandt fisheye (camera_fisheye.py:28): same parameter block, cv2.fisheye.projectPoints forward model."""
  model_names = ("standard", "fix_k1", "fix_k2", "fix_k3", "fix_k4")

  @staticmethod
  def calibrate(boards, detections, image_size, max_iter=10, eps=1e-3, model='standard', fix_aspect=False, has_skew=False, flags=0,
                max_images=None):
    """camera_fisheye.py:71-94 for one camera: (camera, err).  See calibrate_cameras_fisheye."""
    cams, errs = calibrate_cameras_fisheye(boards, [detections], [image_size], max_iter=max_iter, eps=eps, model=model,
                                           fix_aspect=fix_aspect, has_skew=has_skew, flags=flags, max_images=max_images)
    return cams[0], errs[0]


def undistort_images(images, cameras, j=None, chunksize=None):
  """camera.py:249-258: images[c] = the images of cameras[c]; returns the undistorted images, one list per camera.

  The reference maps cv2.remap(image, camera.undistort_map, None, INTER_CUBIC) over a thread pool; here every group of cameras that
  share an image format goes to the device in ONE fused call (undistort.undistort_images: no map is materialised).  j and chunksize
  are accepted and unused."""
  from . import undistort
  out = [[None] * len(cam_images) for cam_images in images]
  groups = {}
  for c, (camera, cam_images) in enumerate(zip(cameras, images)):
    for i, image in enumerate(cam_images):
      image = np.asarray(image)
      groups.setdefault((tuple(camera.image_size), image.shape, image.dtype.str), []).append((c, i, image))
  for (size, _, _), items in groups.items():
    members = sorted({c for c, _, _ in items})
    result = undistort.undistort_images([cameras[c] for c in members], np.stack([image for _, _, image in items]),
                                        camera_of_image=[members.index(c) for c, _, _ in items], image_size=size)
    for (c, i, _), r in zip(items, result):
      out[c][i] = r
  return out


# ---- intrinsic calibration from detections (camera.py:184-241) ---------------------------------------------------------------
# detections: per frame a list with one struct(ids, corners) per board, as the reference's detect step returns them
def _has_min_detections(board, detection):
  if hasattr(board, "has_min_detections"):
    return board.has_min_detections(detection)
  from . import tables
  ids = np.asarray(detection.ids, dtype=np.int64).ravel()
  n = int(getattr(board, "num_points", len(np.asarray(board.points))))
  valid = np.zeros((1, 1, 1, n), dtype=bool)
  valid[0, 0, 0, ids] = True
  return len(ids) >= 4 and bool(tables.min_detections_mask(valid, [board])[0, 0, 0])


def board_correspondences(board_id, board, detections):
  """The views of one board (camera.py:184-195): detections = that board's struct(ids, corners) of every frame."""
  kept = [(i, d) for i, d in enumerate(detections) if _has_min_detections(board, d)]
  pts = np.asarray(board.points)
  return struct(corners=[np.asarray(d.corners, dtype=np.float32).reshape(-1, 2) for _, d in kept],
                ids=[np.asarray(d.ids).ravel() for _, d in kept],
                object_points=[pts[np.asarray(d.ids).ravel()].astype(np.float32) for _, d in kept],
                board_offset=[float(board_id)] * len(kept), image_ids=[i for i, _ in kept])


def calibration_points(boards, detections):
  """All views of one camera, board by board (camera.py:229-235): struct of parallel lists corners, ids, object_points,
  board_offset, image_ids."""
  per_board = [board_correspondences(b, board, [frame[b] for frame in detections]) for b, board in enumerate(boards)]
  return struct(**{k: [x for pb in per_board for x in pb[k]] for k in ("corners", "ids", "object_points", "board_offset", "image_ids")})


def coverage(corners, bins):
  """Number of image bins that hold a corner (camera.py:206-210)."""
  corners = np.asarray(corners).reshape(-1, 2)
  hist, _, _ = np.histogram2d(corners[:, 0], corners[:, 1], bins)
  return int(np.count_nonzero(hist))


def image_bins(image_size, approx_bins=10):
  bin_size = min(image_size[0] / approx_bins, image_size[1] / approx_bins)
  return [np.linspace(0, image_size[axis], int(image_size[axis] / bin_size)) for axis in (0, 1)]


def top_detection_coverage(detections, k, image_size, approx_bins=10, jitter=0.1, rng=None):
  """The k views that cover the most image bins (camera.py:219-227).

  DEVIATION from the reference: it adds np.random.normal(0, jitter * approx_bins**2) -- a standard deviation of 10 bins, unseeded --
  to every view's bin count before sorting, so its choice differs from run to run.  Here rng=None means NO jitter and a stable
  order (ties keep their order in the list); passing a numpy Generator draws the reference's jitter from it."""
  bins = image_bins(image_size, approx_bins=10)
  sizes = np.array([-float(coverage(c, bins)) for c in detections.corners])
  if rng is not None:
    sizes = sizes + rng.normal(0, jitter * (approx_bins * approx_bins), len(sizes))
  order = np.argsort(sizes, kind='stable')[:k]
  return detections._map(lambda xs: [xs[i] for i in order])


def _solve(*args, **kwargs):
  """The device call of a round (tables.calibrate_intrinsics); the tests of the rejection loop replace it."""
  from . import tables
  return tables.calibrate_intrinsics(*args, **kwargs)


def _dense_views(boards, points_per_camera, n_frames):
  """Detection table [C,F,B,P] of the listed views and the mask [C,F,B] of the slots they fill.  F is the number of frames of the
  detections in every round, whatever views are left: the warm start of a round is the pose table of the round before."""
  from .structs import Table
  C_, B, F = len(points_per_camera), len(boards), int(n_frames)
  P = max(len(np.asarray(b.points)) for b in boards)
  pts, valid, mask = np.zeros((C_, F, B, P, 2)), np.zeros((C_, F, B, P), dtype=bool), np.zeros((C_, F, B), dtype=bool)
  for c, p in enumerate(points_per_camera):
    for corners, ids, b, f in zip(p.corners, p.ids, p.board_offset, p.image_ids):
      pts[c, f, int(b), ids] = corners
      valid[c, f, int(b), ids] = True
      mask[c, f, int(b)] = True
  return Table.create(points=pts, valid=valid), mask


def _solved_views(res, c, points):
  """The views of camera c that entered the solution: a view without a start pose (collinear corners: VIEW_DEGENERATE) has no
  error and no pose, so it leaves the list -- it is neither counted in the quantile nor warm-started at the identity."""
  from . import tables
  keep = [i for i, (b, f) in enumerate(zip(points.board_offset, points.image_ids)) if res.view_status[c, f, int(b)] == tables.VIEW_OK]
  return points if len(keep) == len(points.image_ids) else points._map(lambda xs: [xs[i] for i in keep])


def _require_result(res, c):
  from . import tables
  if res.camera_status[c] not in (tables.CAMERA_OK, tables.CAMERA_NOT_CONVERGED):
    names = {tables.CAMERA_TOO_FEW_VIEWS: "fewer than 3 usable views", tables.CAMERA_DEGENERATE: "degenerate views (no focal start)",
             tables.CAMERA_MASKED: "no views"}
    raise RuntimeError(f"intrinsic calibration of camera {c} failed: {names.get(int(res.camera_status[c]), res.camera_status[c])}")


def _camera_of(res, c, cls, image_size, model, fix_aspect, has_skew, points):
  blk, nd = res.cameras[c], int(res.camera_n_dist[c])
  K = np.array([[blk[0], 0.0, blk[2]], [0.0, blk[1], blk[3]], [0.0, 0.0, 1.0]])
  per_view = np.array([res.error_perview[c, f, int(b)] for b, f in zip(points.board_offset, points.image_ids)])
  return cls(image_size=image_size, intrinsic=K, dist=blk[5:5 + nd].copy(), model=model, fix_aspect=fix_aspect, has_skew=has_skew,
             error_perview=per_view, intrinsic_dataset={'board_ids': list(points.board_offset), 'image_ids': list(points.image_ids)})


def calibrate_cameras(boards, points, image_sizes, intrinsic_error_limit, max_iter=10, eps=1e-3, model='standard', fix_aspect=False,
                      has_skew=False, flags=0, max_images=None):
  """camera.py:237-241 + the loop of Camera.calibrate (camera.py:84-99): (cameras, errs).  points: the detections of every camera.

  A round solves ALL cameras that are not finished in one device call (tables.calibrate_intrinsics); err = sqrt(sum sse / sum n),
  per-view error = sqrt(sse_v / n_v).  While |err| >= its limit a camera with 15 views or more rounds err to two decimals and
  keeps the views below the 0.95 quantile of the per-view errors; one with fewer raises its limit by 0.1.  Differences from the
  reference: a view whose corners give no start pose (collinear) leaves the list; finished cameras are masked out of later rounds; a round starts from the previous solution; the reference's repeat
  solve on unchanged data (fewer than 15 views) is skipped -- its result is the same.  max_iter, eps and flags are accepted and
  UNUSED: the solve goes to the optimum of the reprojection cost, not to cv2's (max_iter, eps) stop.  Skew is not estimated."""
  assert model in Camera.model_names, f"unknown camera model {model} options are {list(Camera.model_names)}"
  n = len(points)
  n_frames = max(len(d) for d in points)
  views = [calibration_points(boards, d) for d in points]
  if max_images is not None:
    views = [top_detection_coverage(v, max_images, size) for v, size in zip(views, image_sizes)]
  limits, errs = [float(intrinsic_error_limit)] * n, [float(intrinsic_error_limit)] * n
  cameras, init = [None] * n, None
  active = [c for c in range(n) if abs(errs[c]) >= limits[c]]
  while active:
    table, mask = _dense_views(boards, views, n_frames)
    mask[[c for c in range(n) if c not in active]] = False
    res = _solve(table, boards, image_sizes, model=model, fix_aspect=fix_aspect, view_mask=mask, init=init)
    init = (res.cameras, res.poses)
    for c in active:
      _require_result(res, c)
      v = views[c] = _solved_views(res, c, views[c])
      cameras[c] = _camera_of(res, c, Camera, image_sizes[c], model, fix_aspect, has_skew, v)
      per_view, errs[c] = cameras[c].error_perview, float(res.error[c])
      if len(per_view) >= 15:
        errs[c] = float("{:.2f}".format(errs[c]))
        threshold = np.quantile(per_view, 0.95)
        keep = [i for i, e in enumerate(per_view) if e < threshold]
        views[c] = v._map(lambda xs: [xs[i] for i in keep])
        cameras[c].intrinsic_dataset = {'board_ids': list(views[c].board_offset), 'image_ids': list(views[c].image_ids)}
      else:
        while abs(errs[c]) >= limits[c]:     # (the reference solves the same views again after every step of the limit)
          limits[c] += 0.1
    active = [c for c in active if abs(errs[c]) >= limits[c]]
  return cameras, errs


def calibrate_cameras_fisheye(boards, points, image_sizes, max_iter=10, eps=1e-3, model='standard', fix_aspect=False, has_skew=False,
                              flags=0, max_images=None):
  """camera_fisheye.py:71-94 for every camera, all of them in ONE device call: (cameras, errs).  One solve over every view that
  passes has_min_detections, no rejection rounds (the reference has none for fisheye cameras).  `fix_kN` holds that coefficient at
  0 (cv2.fisheye.CALIB_FIX_KN); skew is never estimated (the reference passes CALIB_FIX_SKEW).  max_iter, eps and flags are
  accepted and unused: the solution is the optimum of the reprojection cost."""
  assert model in CameraFisheye.model_names, f"unknown camera model {model} options are {list(CameraFisheye.model_names)}"
  views = [calibration_points(boards, d) for d in points]
  if max_images is not None:
    views = [top_detection_coverage(v, max_images, size) for v, size in zip(views, image_sizes)]
  free = [0 if model == f"fix_k{i + 1}" else 1 for i in range(4)]
  table, mask = _dense_views(boards, views, max(len(d) for d in points))
  res = _solve(table, boards, image_sizes, model='fisheye', fix_aspect=fix_aspect, view_mask=mask, free_dist=[free] * len(views))
  cameras = []
  for c, v in enumerate(views):
    _require_result(res, c)
    cameras.append(_camera_of(res, c, CameraFisheye, image_sizes[c], model, fix_aspect, has_skew, _solved_views(res, c, v)))
  return cameras, [float(e) for e in res.error]


# ---- stereo calibration of a pair with the cameras held (camera.py:261-286, camera_fisheye.py:180-200) -------------------------
def _start_poses(points, valid, board_points, cameras):
  """The device call behind the start poses of the matched views (tables.view_poses); the host tests replace it."""
  from . import tables
  return tables.view_poses(points, valid, board_points, cameras)


def _stereo_calibrate(cameras, matches, fix_intrinsic, who):
  from . import stereo
  if not fix_intrinsic:
    raise NotImplementedError(f"{who}(fix_intrinsic=False): the pair model holds the cameras (cv2.CALIB_FIX_INTRINSIC); intrinsics and "
                              "extrinsics are refined together by Calibration.bundle_adjust")
  left, right = cameras
  views = list(zip(matches.object_points, matches.points1, matches.points2))
  n = len(views)
  if n == 0:
    raise RuntimeError(f"{who}: no matched views")
  P = max(max(len(np.asarray(x)) for x, _, _ in views), 1)
  # every matched view is a board of its own in a table of one frame: [2, 1, n, P]
  points, valid, boards = np.zeros((2, 1, n, P, 2)), np.zeros((2, 1, n, P), dtype=bool), []
  for b, (X, p1, p2) in enumerate(views):
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    points[0, 0, b, :len(X)] = np.asarray(p1, dtype=np.float64).reshape(-1, 2)
    points[1, 0, b, :len(X)] = np.asarray(p2, dtype=np.float64).reshape(-1, 2)
    valid[:, 0, b, :len(X)] = True
    boards.append(X)
  poses, _, _, status, _ = _start_poses(points, valid, boards, [left, right])
  res = stereo.calibrate_pairs([left, right], boards, points, valid, poses, status == 0, [(0, 1)])
  if res.status[0] not in (stereo.OK, stereo.NOT_CONVERGED):
    raise RuntimeError(f"{who} failed: {stereo.STATUS_NAMES.get(int(res.status[0]), res.status[0])}")
  return left.copy(), right.copy(), res.T[0], float(res.rms[0])


def stereo_calibrate(cameras, matches, max_iter=60, eps=1e-6, fix_aspect=False, fix_intrinsic=True):
  """camera.py:261-286 (cv2.stereoCalibrate with CALIB_USE_INTRINSIC_GUESS | CALIB_FIX_INTRINSIC): (left, right, pose, err) with
  pose = matrix.join(R, T), left-camera frame -> right-camera frame.  matches: tables.matching_points' struct of parallel lists
  object_points, points1, points2 -- one entry per view.

  One device call (stereo.calibrate_pairs); the views start from their PnP pose in the left camera.  err = sqrt(sse / (2 n)) over the
  pair's 2 n image points, believed to be cv2's return value (no cv2 binary was at hand to confirm it).  max_iter and eps are
  accepted and UNUSED, as in Camera.calibrate here: the solve goes to the optimum of the reprojection cost, not to cv2's stop;
  fix_aspect has nothing to act on while the intrinsics are held.  fix_intrinsic=False raises: Calibration.bundle_adjust refines
  intrinsics and extrinsics together.  The two cameras need not share a model or an image size."""
  return _stereo_calibrate(cameras, matches, fix_intrinsic, "stereo_calibrate")


def stereo_calibrate_fisheye(cameras, matches, max_iter=60, eps=1e-6, fix_aspect=False, fix_intrinsic=True):
  """camera_fisheye.py:180-200 (cv2.fisheye.stereoCalibrate): the same call as stereo_calibrate -- the projection of every camera
  is switched at run time by its own family, so the two functions differ in name only."""
  return _stereo_calibrate(cameras, matches, fix_intrinsic, "stereo_calibrate_fisheye")
