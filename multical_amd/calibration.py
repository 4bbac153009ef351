"""Host mirror of multical.optimization.calibration.Calibration (optimization/calibration.py:43-310) whose numerical
work runs on the MI355X back-end.

Same constructor, same immutable-copy style, same parameter ordering and the same public methods as the reference
class, so that callers written against the reference (Workspace.calibrate, workspace.py:228-247) work unchanged:

    bundle_adjust(tolerance, f_scale, max_iterations, loss)   calibration.py:199-212   -> mcba_solve
    reprojected / reprojection_error / reprojection_inliers    calibration.py:124-141   -> mcba_project / _error
    reject_outliers / adjust_outliers / report                 calibration.py:234-300
    enable / copy / params / with_params / param_vec           calibration.py:144-171,214-232

Objects hold no device state: like the reference only the 8 constructor fields are pickled (calibration.py:222-226);
device handles live in a small module-level cache keyed on the observation table.
"""
import contextlib
import logging
import os
from functools import cached_property

import numpy as np

from . import distributed, parameters
from .backend import Handle, lower
from .structs import Struct, Table, struct, choose, subset

logger = logging.getLogger("calibration")   # same logger name as multical/io/logging.py:11


def info(msg):
  logger.info(msg)


class LogWriter(object):
  """io/logging.py:53-68: file-like object that forwards what scipy prints with verbose=2 to the "calibration" logger."""

  def __init__(self, level=logging.INFO, ignore_newline=True):
    self.level, self.ignore_newline = level, ignore_newline

  def write(self, message, *args, **kwargs):
    if message != '\n' or not self.ignore_newline:
      logger._log(self.level, message, args, **kwargs)

  def flush(self):
    pass

  @staticmethod
  def info(ignore_newline=True):
    return LogWriter(logging.INFO, ignore_newline)


# Which solver `Calibration.bundle_adjust` uses (all run residuals and Jacobian on the MI355X):
#   "lsmr"    DEFAULT.  mcba_solve with scipy's OWN trust-region step on the device (tr_solver = lsmr): gn_h = lsmr(J_h, f, damp) with
#             the two Jacobian products as HIP kernels and scipy's driver restated line by line -- the reference's trajectory and
#             END POINT (within max(1e-6 px, the reference's own reproducibility), identical nfev / status), without the
#             host-side LSMR (an hour of one core at the north-star rig).
#   "native"  mcba_solve: trust-region driver with exact Schur / Cholesky steps, everything on the device, ~100 x faster than
#             "lsmr".  Ends at the CONVERGED optimum (at or below the reference's cost) -- NOT at the reference's end point: on
#             weakly determined rigs the principal point ends tens of pixels away from the reference's (profiles/parity_table.md).
#   "scipy"   the reference's own call scipy.optimize.least_squares(method='trf', x_scale='jac', ...) on mcba_residuals +
#             mcba_jacobian (Handle.solve_scipy): the reference's end point as well, at the price of scipy's host-side LSMR.
SOLVERS = ("lsmr", "native", "scipy")
_default_solver = [os.environ.get("MULTICAL_AMD_SOLVER", "lsmr").lower()]


def set_solver(name):
  """Select the solver of every following `bundle_adjust` / `adjust_outliers` / `Workspace.calibrate`; returns the previous one."""
  if name not in SOLVERS:
    raise ValueError(f"unknown solver {name!r}, options are {SOLVERS}")
  prev, _default_solver[0] = _default_solver[0], name
  if prev != name:
    import logging
    logging.getLogger("calibration").info("multical_amd: bundle adjustment solver '%s' -> '%s'", prev, name)
  return prev


def get_solver():
  return _default_solver[0]


_scipy_unsharded_noted = [False]


def _note_scipy_unsharded():
  if distributed.sharding_enabled() and not _scipy_unsharded_noted[0]:
    _scipy_unsharded_noted[0] = True
    logger.info("multical_amd: solver 'scipy' is not frame-sharded: every rank solves the whole rig")


def fused_outlier_loop_off():
  """MULTICAL_AMD_FUSED_LOOP=0: adjust_outliers as a Python loop over report / reject_outliers / bundle_adjust on new Calibration
  objects (the reference's structure, step by step) instead of one mcba_adjust_outliers call."""
  return os.environ.get("MULTICAL_AMD_FUSED_LOOP", "1") == "0"


default_optimize = struct(cameras=False, boards=False, camera_poses=True, board_poses=True, motion=True)


def select_threshold(quantile=0.75, factor=5.0):
  """calibration.py:37-40.  The returned callable still works on an error array like the reference's; it is tagged with
  its parameters so that adjust_outliers can evaluate the quantile on the device without downloading the errors."""
  def f(reprojection_error):
    return np.quantile(reprojection_error, quantile) * factor
  f.quantile, f.factor = quantile, factor
  return f


def error_stats(errors):
  """calibration.py:304-310."""
  if len(errors) == 0:
    errors = np.zeros((1, 1), np.float32)
  mse = np.square(errors).mean()
  quantiles = np.array([np.quantile(errors, n) for n in [0, 0.25, 0.5, 0.75, 1]])
  return struct(mse=mse, rms=np.sqrt(mse), quantiles=quantiles, n=errors.size)


# ---------------------------------------------------------------------------------------------------------------
# device-handle cache (never pickled, never part of a Calibration)
# ---------------------------------------------------------------------------------------------------------------
class _HandleCache(object):
  def __init__(self, capacity=2):
    self.capacity = capacity
    # entries: dict(key, points, valid, x_full, handle, mask).  `points` / `valid` are the ORIGINAL arrays of the point
    # table the handle was built from, held strongly: identity (`is`) is the fast test, and holding the reference keeps
    # an id from being recycled by a later table of the same shape (float32 detections are widened into a copy, so the
    # handle itself would not keep the original alive).  A table with equal content but another identity (e.g.
    # `point_table._extend(valid=...)` keeps `points`, replaces `valid`) is compared by value.  The inlier mask OBJECT is
    # a token compared with `is` first: hashing 2.6 MB of mask bytes on every lookup cost 0.6 ms x 16 lookups per
    # Workspace.calibrate.
    self.entries = []
    # frame-sharded handles (multical_amd.distributed.sharding) live in a list of their own, keyed additionally by group, world size
    # and shard plan.  Their inputs are replicated, so hits, misses and evictions are the same on every rank -- creation is collective.
    self.sharded = []

  @staticmethod
  def _same_array(a, b):
    return a is b or (a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b))

  def get(self, calib, sharded=False):
    """(handle, lowered problem) of `calib`; sharded=True: a frame-sharded handle while multical_amd.distributed.sharding is on with
    more than one rank (otherwise the plain one)."""
    prob = getattr(calib, "_mcba_problem", None)     # Calibration objects are immutable: lower once per object
    if prob is None:
      prob = lower(calib)
      try:
        calib._mcba_problem = prob                   # (not part of __getstate__: never pickled)
      except AttributeError:
        pass
    key = (prob.shape, prob.optimize, prob.motion, prob.camera_model, prob.n_dist,
           None if prob.camera_n_dist is None else prob.camera_n_dist.tobytes(),
           None if prob.camera_fisheye is None else prob.camera_fisheye.tobytes(), prob.fix_aspect.tobytes(),
           prob.camera_valid.tobytes(), prob.frame_valid.tobytes(), prob.board_valid.tobytes(),
           prob.board_sizes.tobytes(), prob.image_heights.tobytes())
    cfg = distributed.shard_config() if sharded else None
    entries = self.entries
    if cfg is not None:
      group, world, native, balance = cfg
      plan = distributed.shard_plan(calib, world, balance)
      key = key + ("sharded", id(group), world, tuple(plan))
      entries = self.sharded
    points, valid = calib.point_table.points, calib.point_table.valid
    for i, e in enumerate(entries):
      h = e["handle"]
      if e["key"] == key and h.h and self._same_array(e["points"], points) and self._same_array(e["valid"], valid) \
          and np.array_equal(self._constants(calib, prob, e["x_full"]), self._constants(calib, prob, prob.x_full)) \
          and (prob.base_wrt_gripper is None or np.array_equal(prob.base_wrt_gripper, h.problem.base_wrt_gripper)):
        mask, tok = calib.inlier_mask, e["mask"]
        if mask is not tok:
          if mask is None or tok is None or not np.array_equal(mask, tok):
            h.set_inliers(mask)
          e["mask"] = mask
        return h, prob
    if cfg is None:
      h = Handle(prob)
    else:
      distributed.agree_on_plan(plan, group)        # once per handle, before the collective creation
      h = distributed.sharded_handle(calib, group=group, native=native, shards=plan, problem=prob)
      h.shard_group = group
    entries.append(dict(key=key, points=points, valid=valid, x_full=prob.x_full, handle=h, mask=calib.inlier_mask))
    while len(entries) > self.capacity:
      entries.pop(0)["handle"].close()
    return h, prob

  @staticmethod
  def _constants(calib, prob, x_full):
    """values of the DISABLED blocks (the only part of x_full the device keeps)."""
    out, pos = [], 0
    for k, n in zip(parameters_order(), prob.block_sizes):
      if calib.optimize[k] is not True:
        out.append(x_full[pos:pos + n])
      pos += n
    return np.concatenate(out) if out else np.zeros(0)

  def note_inliers(self, handle, mask):
    """the device already holds `mask` (set by reject_outliers): remember its token so it is not uploaded again."""
    for e in self.entries + self.sharded:
      if e["handle"] is handle:
        e["mask"] = mask

  def invalidate_inliers(self, handle):
    """a library call that rewrites the device mask (mcba_reject_outliers, mcba_adjust_outliers) FAILED part-way: the
    device mask is unknown, so the next lookup must upload its own (a fresh token never compares equal)."""
    self.note_inliers(handle, _UNKNOWN_MASK)

  def close_sharded(self, group=None):
    """close the sharded handles of `group` (leaving multical_amd.distributed.sharding)"""
    keep = []
    for e in self.sharded:
      if getattr(e["handle"], "shard_group", None) is group:
        e["handle"].close()
      else:
        keep.append(e)
    self.sharded = keep

  def clear(self):
    for e in self.entries + self.sharded:
      e["handle"].close()
    self.entries = []
    self.sharded = []


def parameters_order():
  return ["camera_poses", "board_poses", "motion", "cameras", "boards"]


_UNKNOWN_MASK = np.zeros(0, dtype=np.uint8)   # token of "the device mask is in an unknown state"
handle_cache = _HandleCache()


class Calibration(parameters.Parameters):
  correction = None          # a correction.FieldCorrection and the table it was applied to: with_corrected_observations
  raw_point_table = None

  def __init__(self, cameras, boards, point_table, camera_poses, board_poses, motion, inlier_mask=None,
               optimize=default_optimize, correction=None, raw_point_table=None):
    # (correction, raw_point_table: set by with_corrected_observations alone -- point_table is then the warped raw table)
    assert (correction is None) == (raw_point_table is None), "a corrected calibration carries its raw table"
    if correction is not None:            # (class attributes else: the state of an uncorrected calibration is what it was)
      self.correction = correction
      self.raw_point_table = raw_point_table
    self.cameras = cameras
    self.boards = boards
    self.point_table = point_table
    self.camera_poses = camera_poses
    self.board_poses = board_poses
    self.motion = motion
    self.optimize = optimize
    self.inlier_mask = inlier_mask

    assert len(self.cameras) == self.size.cameras
    assert camera_poses.size == self.size.cameras
    assert board_poses.size == self.size.boards

  # --- shapes and masks (calibration.py:63-81) --------------------------------------------------------------
  @cached_property
  def size(self):
    cameras, rig_poses, boards, points = self.point_table.valid.shape
    return struct(cameras=cameras, rig_poses=rig_poses, boards=boards, points=points)

  @cached_property
  def valid(self):
    valid = (np.expand_dims(self.camera_poses.valid, [1, 2]) & np.expand_dims(self.motion.valid, [0, 2]) &
             np.expand_dims(self.board_poses.valid, [0, 1]))
    return self.point_table.valid & np.expand_dims(valid, valid.ndim)

  @cached_property
  def inliers(self):
    return choose(self.inlier_mask, self.valid)

  # --- parameters (calibration.py:144-171) ------------------------------------------------------------------
  @cached_property
  def param_objects(self):
    return struct(camera_poses=self.camera_poses, board_poses=self.board_poses, motion=self.motion,
                  cameras=self.cameras, boards=self.boards)

  @cached_property
  def params(self):
    all_params = self.param_objects._map(lambda p: p.param_vec)
    return all_params._filterWithKey(lambda k: self.optimize[k] is True)

  def with_params(self, params):
    updated = {k: self.param_objects[k].with_param_vec(param_vec) for k, param_vec in params.items()}
    return self.copy(**updated)

  def enable(self, **flags):
    for k in flags.keys():
      assert k in self.optimize, f"unknown option {k}, options are {list(self.optimize.keys())}"
    return self.copy(optimize=self.optimize._extend(**flags))

  def __getstate__(self):
    attrs = ['cameras', 'boards', 'point_table', 'camera_poses', 'board_poses', 'motion', 'inlier_mask', 'optimize']
    if self.correction is not None:
      attrs = attrs + ['correction', 'raw_point_table']
    return subset(self.__dict__, attrs)

  def __setstate__(self, d):
    self.__dict__.update(d)

  def copy(self, **k):
    d = self.__getstate__()
    d.update(k)
    return Calibration(**d)

  def with_master(self, camera):
    """calibration.py:99-104: re-gauge so that `camera` (name or index) sits at the origin."""
    if isinstance(camera, str):
      camera = self.camera_poses.names.index(camera)
    return self.transform_views(self.camera_poses.poses[int(camera)])

  def transform_views(self, t):
    """calibration.py:107-112: cameras by t^-1, time poses by t -- the reprojections do not change."""
    return self.copy(camera_poses=self.camera_poses.post_transform(np.linalg.inv(t)),
                     motion=self.motion.pre_transform(t))

  # --- device evaluation ------------------------------------------------------------------------------------
  def _handle(self, sharded=False):
    """the cached device handle; sharded=True: frame-sharded while multical_amd.distributed.sharding is on (solves, outlier loop and
    statistics).  The accessors that return per-point arrays always use the plain handle."""
    return handle_cache.get(self, sharded)[0]

  @cached_property
  def reprojected(self):
    """calibration.py:124-130 (rolling-shutter scan time from the measured points).  Per-point: always the plain (unsharded) handle."""
    h = self._handle()
    points = h.project(self.param_vec)
    _, valid = h.reprojection_error(self.param_vec)
    # reprojected.valid of the reference = pose validity & board-point validity (no detection mask)
    C, F, B, P = self.point_table.valid.shape
    pose_valid = (np.expand_dims(self.camera_poses.valid, [1, 2, 3]) & np.expand_dims(self.motion.valid, [0, 2, 3]) &
                  np.expand_dims(self.board_poses.valid, [0, 1, 3]))
    sizes = np.array([b.num_points for b in self.boards])
    board_valid = np.arange(P)[None, :] < sizes[:, None]
    return Table.create(points=points, valid=pose_valid & board_valid[None, None])

  @cached_property
  def projected(self):
    """calibration.py:113-119: projected points to each image WITHOUT the measured points (rolling shutter: the scan
    time is iterated from the projected row, RollingFrames.max_iterations passes) -- the table the GUI draws.  Per-point: always the
    plain (unsharded) handle."""
    h = self._handle()
    points = h.project_model(self.param_vec, getattr(self.motion, "max_iterations", 4))
    return Table.create(points=points, valid=self.reprojected.valid)

  def _errors(self):
    """tables.reprojection_error (tables.py:244-249) of (reprojected, point_table) on the device."""
    return self._handle().reprojection_error(self.param_vec)

  @cached_property
  def reprojection_error(self):
    """per-point errors of the valid points; always the plain (unsharded) handle"""
    err, mask = self._errors()
    return err[mask]

  @cached_property
  def reprojection_inliers(self):
    """per-point errors of the inliers; always the plain (unsharded) handle"""
    err, mask = self._errors()
    # calibration.py:138-141: point_table with valid := inliers, masked with reprojected.valid
    return err[self.reprojected.valid & choose(self.inliers, self.valid)]

  def residuals(self, param_vec=None):
    """`evaluate` of calibration.py:204-206; always the plain (unsharded) handle."""
    return self._handle().residuals(self.param_vec if param_vec is None else param_vec)

  def jacobian(self, param_vec=None):
    """always the plain (unsharded) handle"""
    return self._handle().jacobian(self.param_vec if param_vec is None else param_vec)

  # --- solve (calibration.py:199-212) -----------------------------------------------------------------------
  def bundle_adjust(self, tolerance=1e-4, f_scale=1.0, max_iterations=100, loss='linear', return_result=False,
                    xtol=1e-8, gtol=1e-8, solver=None):
    """Non-linear least squares on point reprojection error, solved on the GPU.

    Keeps the reference's signature and semantics.  solver = "lsmr" (default, see `set_solver`) / "native" (mcba_solve): the iteration
    table scipy prints with verbose=2 is emitted in the same format through the "calibration" logger (calibration.py:208,
    io/logging.py:53-68).  solver = "scipy": the reference's own `least_squares` call on the device residuals + analytic
    Jacobian (`Handle.solve_scipy`), scipy's own table redirected to the logger exactly as calibration.py:208 does.
    Under multical_amd.distributed.sharding the "lsmr" / "native" solves run on frame-sharded handles (every rank returns the same
    parameter vector); "scipy" stays unsharded."""
    solver = get_solver() if solver is None else solver
    if solver not in SOLVERS:
      raise ValueError(f"unknown solver {solver!r}, options are {SOLVERS}")
    if solver == "scipy":
      _note_scipy_unsharded()
      h = self._handle()
      with contextlib.redirect_stdout(LogWriter.info()):
        res = h.solve_scipy(self.param_vec, tolerance=tolerance, f_scale=f_scale, max_iterations=max_iterations, loss=loss,
                            verbose=2)
      out = self.with_param_vec(res.x)
      return (out, res) if return_result else out
    h = self._handle(sharded=True)
    rows = []

    def log_row(it, nfev, cost, red, step, opt):
      red_s = " " * 15 if np.isnan(red) else f"{red:^15.2e}"
      step_s = " " * 15 if np.isnan(step) else f"{step:^15.2e}"
      rows.append(f"{it:^15}{nfev:^15}{cost:^15.4e}{red_s}{step_s}{opt:^15.2e}")

    h.set_log(log_row)
    info("{:^15}{:^15}{:^15}{:^15}{:^15}{:^15}".format("Iteration", "Total nfev", "Cost", "Cost reduction",
                                                       "Step norm", "Optimality"))
    try:
      res = h.solve(self.param_vec, tolerance=tolerance, f_scale=f_scale, max_iterations=max_iterations, loss=loss,
                    xtol=xtol, gtol=gtol, verbose=2, tr_solver="lsmr" if solver == "lsmr" else "exact")
    finally:
      h.set_log(None)        # cached handles outlive the call: do not keep the closure over `rows` installed
    for r in rows:
      info(r)
    info(res.message)
    info(f"Function evaluations {res.nfev}, initial cost {res.initial_cost:.4e}, final cost {res.cost:.4e}, "
         f"first-order optimality {res.optimality:.2e}.")
    out = self.with_param_vec(res.x)
    return (out, res) if return_result else out

  # --- outliers (calibration.py:234-268) --------------------------------------------------------------------
  def reject_outliers_quantile(self, quantile=0.95, factor=1.0):
    threshold = np.quantile(self.reprojection_error, quantile)
    return self.reject_outliers(threshold=threshold * factor)

  def _select(self, selector):
    """selector(self.reprojection_error); tagged select_threshold closures are evaluated on the device
    (exact numpy 'linear' quantile from radix-selected order statistics), anything else gets the error array."""
    if hasattr(selector, "quantile") and hasattr(selector, "factor"):
      # report() has usually just selected this very quantile (0.75 is one of its five): same object, same errors
      stats = self.__dict__.get("_overall_stats")
      if stats is not None:
        hit = [v for qq, v in zip(stats[0], stats[1].quantiles) if qq == selector.quantile]
        if hit:
          return float(hit[0]) * selector.factor
      _, _, q, _ = self._handle(sharded=True).error_stats(self.param_vec, quantiles=[selector.quantile])
      return float(q[0]) * selector.factor
    return selector(self.reprojection_error)

  def reject_outliers(self, threshold):
    """calibration.py:240-252, evaluated on the device; only the new mask (uint8) comes back (complete on every rank when sharded)."""
    h = self._handle(sharded=True)
    try:
      n_in, n_valid = h.reject_outliers(self.param_vec, threshold)
      inliers = h.gather_inliers()
    except BaseException:
      handle_cache.invalidate_inliers(h)
      raise
    num_outliers = n_valid - n_in
    inlier_percent = 100.0 * n_in / max(n_valid, 1)
    info(f"Rejecting {num_outliers} outliers with error > {threshold:.2f} pixels, "
         f"keeping {n_in} / {n_valid} inliers, ({inlier_percent:.2f}%)")
    out = self.copy(inlier_mask=inliers)
    handle_cache.note_inliers(h, inliers)
    return out

  def _adjust_outliers_in_one_call(self, num_adjustments, select_scale, select_outliers, kwargs):
    """The whole loop inside the library (mcba_adjust_outliers): no Calibration objects, no re-lowering and no rotation-vector <->
    matrix round trips between the rounds.  The log lines are the reference's, emitted afterwards in the reference's order."""
    h = self._handle(sharded=True)
    rows = []

    def log_row(it, nfev, cost, red, step, opt):
      red_s = " " * 15 if np.isnan(red) else f"{red:^15.2e}"
      step_s = " " * 15 if np.isnan(step) else f"{step:^15.2e}"
      rows.append((it, f"{it:^15}{nfev:^15}{cost:^15.4e}{red_s}{step_s}{opt:^15.2e}"))

    h.set_log(log_row)
    try:
      x, rounds, mask = h.adjust_outliers(
        self.param_vec, num_adjustments,
        outlier=None if select_outliers is None else (select_outliers.quantile, select_outliers.factor),
        scale=None if select_scale is None else (select_scale.quantile, select_scale.factor),
        tr_solver="lsmr" if get_solver() == "lsmr" else "exact", **kwargs)
    except BaseException:
      handle_cache.invalidate_inliers(h)   # a rejection may already have rewritten the device mask
      raise
    finally:
      h.set_log(None)
    tables, cur = [], None                      # the iteration rows of every solve (a solve starts with iteration 0)
    for it, line in rows:
      if it == 0:
        cur = []
        tables.append(cur)
      cur.append(line)
    has_mask = self.inlier_mask is not None

    def report_line(stage, r, with_inliers):
      n_all = max(r.n, 1)                       # (the reference substitutes a single zero for an empty error set)
      if with_inliers:
        info(f"{stage} reprojection RMS={r.rms_inliers:.3f} ({r.rms:.3f}), n={r.n_inliers} ({n_all}), quantiles={r.quantiles}")
      else:
        info(f"{stage} reprojection RMS={r.rms:.3f}, n={n_all}, quantiles={r.quantiles}")

    for i, r in enumerate(rounds[:-1]):
      report_line(f"Adjust_outliers {i}:", r, has_mask)
      if select_scale is not None:
        info(f"Auto scaling for outliers influence at {r.f_scale:.2f} pixels")
      if select_outliers is not None:
        num_outliers = r.n_valid - r.n_kept
        info(f"Rejecting {num_outliers} outliers with error > {r.threshold:.2f} pixels, "
             f"keeping {r.n_kept} / {r.n_valid} inliers, ({100.0 * r.n_kept / max(r.n_valid, 1):.2f}%)")
        has_mask = True
      info("{:^15}{:^15}{:^15}{:^15}{:^15}{:^15}".format("Iteration", "Total nfev", "Cost", "Cost reduction", "Step norm",
                                                         "Optimality"))
      for line in (tables[i] if i < len(tables) else []):
        info(line)
      info(r.solve.message)
      info(f"Function evaluations {r.solve.nfev}, initial cost {r.solve.initial_cost:.4e}, final cost {r.solve.cost:.4e}, "
           f"first-order optimality {r.solve.optimality:.2e}.")
    report_line("Adjust_outliers end:", rounds[-1], has_mask)
    out = self.with_param_vec(x)
    if select_outliers is not None and num_adjustments > 0:
      out = out.copy(inlier_mask=mask)
      handle_cache.note_inliers(h, mask)
    final = rounds[-1]
    out.__dict__["_overall_stats"] = ((0.0, 0.25, 0.5, 0.75, 1.0),
                                      struct(mse=final.rms ** 2, rms=final.rms, quantiles=final.quantiles, n=max(final.n, 1)))
    return out

  def adjust_outliers(self, num_adjustments=3, select_scale=None, select_outliers=None, **kwargs):
    info(f"Beginning adjustments ({num_adjustments}) enabled: {dict(self.optimize)}, options: {kwargs}")
    tagged = lambda f: f is None or (hasattr(f, "quantile") and hasattr(f, "factor"))
    if (get_solver() in ("native", "lsmr") and tagged(select_scale) and tagged(select_outliers) and not fused_outlier_loop_off()
        and set(kwargs) <= {"loss", "tolerance", "f_scale", "max_iterations", "xtol", "gtol"}):
      return self._adjust_outliers_in_one_call(num_adjustments, select_scale, select_outliers, kwargs)
    for i in range(num_adjustments):
      self.report(f"Adjust_outliers {i}:")
      f_scale = (None if select_scale is None else self._select(select_scale)) or 1.0
      if select_scale is not None:
        info(f"Auto scaling for outliers influence at {f_scale:.2f} pixels")
      if select_outliers is not None:
        self = self.reject_outliers(self._select(select_outliers))
      self = self.bundle_adjust(f_scale=f_scale, **kwargs)
    self.report("Adjust_outliers end:")
    return self

  def error_statistics(self, inliers_only=False, quantiles=(0, 0.25, 0.5, 0.75, 1)):
    """error_stats(self.reprojection_error / reprojection_inliers) without downloading the error table.  (A Calibration is
    immutable: the statistics over all valid points are kept on the object, like the reference's cached properties.)"""
    key = tuple(float(q) for q in quantiles)
    if not inliers_only:
      kept = self.__dict__.get("_overall_stats")
      if kept is not None and kept[0] == key:
        return kept[1]
    mse, rms, q, n = self._handle(sharded=True).error_stats(self.param_vec, quantiles=quantiles, inliers_only=inliers_only)
    out = struct(mse=mse, rms=rms, quantiles=q, n=n)
    if not inliers_only:
      self.__dict__["_overall_stats"] = (key, out)
    return out

  def report(self, stage=""):
    overall = self.error_statistics(False)
    # (the reference's report prints RMS and n of the inliers, never their quantiles: calibration.py:296-300)
    inliers = self.error_statistics(True, quantiles=()) if self.inlier_mask is not None else overall
    if self.inlier_mask is not None:
      info(f"{stage} reprojection RMS={inliers.rms:.3f} ({overall.rms:.3f}), "
           f"n={inliers.n} ({overall.n}), quantiles={overall.quantiles}")
    else:
      info(f"{stage} reprojection RMS={overall.rms:.3f}, n={overall.n}, quantiles={overall.quantiles}")

  # --- parameter uncertainty ---------------------------------------------------------------------
  def covariance(self, hold=None, sigma2=None, cross=False):
    """Gauss-Newton covariance sigma2 (J^T J)^-1 of param_vec at the current parameters: linear loss over the current inliers
    (compute it after outlier rejection).  hold: mask over param_vec of the parameters held fixed (default:
    gauge.default_hold); sigma2: known residual variance (None: |r|^2 / (m - p_free)).  Returns struct(shared,
    shared_index, frames [F, DF, DF], frame_index [F, DF], frame_shared [F, DF, n_shared] (cross=True), std, sigma2, dof,
    held).  Always the plain (unsharded) handle: under sharding() every rank computes the same result."""
    from . import gauge
    held = gauge.default_hold(self) if hold is None else np.asarray(hold).astype(bool)
    cov = self._handle().covariance(self.param_vec, hold=held, sigma2=sigma2, frames=True, cross=cross)
    return cov._extend(held=held)

  def parameter_std(self, hold=None, sigma2=None):
    """Standard deviations of the parameters split like `params` (parameters.split): camera_poses [C, 6], board_poses
    [B, 6], motion (shaped as its params), cameras (one array per camera), boards -- the enabled blocks only.  0 where held,
    NaN where no residual depends on the parameter."""
    from . import gauge
    held = gauge.default_hold(self) if hold is None else np.asarray(hold).astype(bool)
    cov = self._handle().covariance(self.param_vec, hold=held, sigma2=sigma2, frames=False)
    return split_std(self, cov.std)

  def report_uncertainty(self, stage="", hold=None):
    """One line per camera through the "calibration" logger: standard deviations of fx, fy, cx, cy (px) and of the camera
    pose (rotation in degrees, translation in board units) in the gauge of `hold` (default: gauge.default_hold)."""
    std = self.parameter_std(hold=hold)
    names = getattr(self.camera_poses, "names", None) or [f"cam{i}" for i in range(self.size.cameras)]
    for c in range(self.size.cameras):
      parts = [f"{stage} {names[c]}:"]
      if "cameras" in std:
        k = np.asarray(std["cameras"][c]).ravel()
        parts.append(f"std fx={k[0]:.3f} fy={k[1]:.3f} cx={k[2]:.3f} cy={k[3]:.3f} px")
      if "camera_poses" in std:
        p = np.asarray(std["camera_poses"][c]).ravel()
        parts.append(f"pose std rotation={np.degrees(np.linalg.norm(p[:3])):.4f} deg translation={np.linalg.norm(p[3:]):.5f}")
      info(" ".join(parts))

  # --- prediction uncertainty per observation -----------------------------------------------------
  def _observation_covariance(self, hold, sigma2, cov, student):
    from . import gauge
    held = gauge.default_hold(self) if hold is None else np.asarray(hold).astype(bool)
    return self._handle().observation_covariance(self.param_vec, hold=held, sigma2=sigma2, cov=cov, student=student)

  def prediction_covariance(self, hold=None, sigma2=None):
    """Covariance of the predicted image point of every valid table slot, C_i = J_i Sigma J_i^T with Sigma of `covariance`
    (same hold / sigma2): struct(cov [C,F,B,P,2,2], valid, sigma2, dof).  NaN where the prediction is not constrained (a valid
    point whose frame, camera or board has no inlier).  Always the plain (unsharded) handle."""
    oc = self._observation_covariance(hold, sigma2, True, False)
    return struct(cov=oc.cov, valid=self.valid, sigma2=oc.sigma2, dof=oc.dof)

  def studentized_error(self, hold=None, sigma2=None):
    """Reprojection error of every valid point in units of its own standard deviation: d = sqrt(r^T Omega^-1 r) with Omega =
    sigma2 I - C_i for inliers (residual covariance) and sigma2 I + C_i for the other valid points (prediction-error
    covariance); d^2 is chi-square with 2 degrees of freedom under the model.  struct(error [C,F,B,P], valid)."""
    oc = self._observation_covariance(hold, sigma2, False, True)
    return struct(error=oc.student, valid=self.valid)

  def reject_outliers_studentized(self, threshold, hold=None):
    """The analogue of reject_outliers on the studentised error: inliers = valid points with d < threshold (NaN, an
    unconstrained prediction, is rejected)."""
    st = self.studentized_error(hold=hold)
    with np.errstate(invalid="ignore"):
      inliers = (st.error < threshold) & st.valid
    n_in, n_valid = int(inliers.sum()), int(st.valid.sum())
    info(f"Rejecting {n_valid - n_in} outliers with studentized error > {threshold:.2f}, "
         f"keeping {n_in} / {n_valid} inliers, ({100.0 * n_in / max(n_valid, 1):.2f}%)")
    return self.copy(inlier_mask=inliers)

  def report_prediction_uncertainty(self, stage="", hold=None):
    """One line per camera through the "calibration" logger: median and max standard deviation of the predicted points (px,
    sqrt of the larger eigenvalue of C_i over the camera's valid points) and the largest leverage tr(H_ii) of its inliers."""
    oc = self._observation_covariance(hold, None, True, False)
    uu, uv, vv = oc.cov[..., 0, 0], oc.cov[..., 0, 1], oc.cov[..., 1, 1]
    with np.errstate(invalid="ignore"):
      std = np.sqrt(np.maximum(0.5 * (uu + vv) + np.sqrt((0.5 * (uu - vv)) ** 2 + uv ** 2), 0.0))
    lev = (uu + vv) / oc.sigma2
    names = getattr(self.camera_poses, "names", None) or [f"cam{i}" for i in range(self.size.cameras)]
    for c in range(self.size.cameras):
      s = std[c][self.valid[c] & np.isfinite(std[c])]
      l = lev[c][self.inliers[c] & np.isfinite(lev[c])]
      med = float(np.median(s)) if s.size else float("nan")
      info(f"{stage} {names[c]}: predicted std median={med:.4f} max={float(oc.cam_max_std[c]):.4f} px, "
           f"max leverage={float(l.max()) if l.size else float('nan'):.4f}")

  # --- residual fields: the systematic part of the reprojection error ----------------------------
  def residual_field(self, nx=5, ny=4, n_folds=5, prior_px=1.0, sigma2=None, inliers_only=True, grid=(16, 12), pixels=None,
                     coverage=(16, 12), tau0=100.0):
    """Is what the bundle adjustment leaves behind noise?  Per camera a smooth vector field (uniform cubic B-spline, nx x ny
    intervals over the image) is fitted to the residuals projected - observed as a function of the observed pixel: one pass over the
    observation table on the device (mcba_residual_gram), the rest numpy on blocks of at most 62 x 62 (multical_amd.residual_field).
    Returns struct(field [C, gh, gw, 2] on the centres of `grid` (or [C, n, 2] at `pixels`), field_std (its posterior standard
    deviation), pixels, coefficients [C, K, 2], n, rms (all of the residual), systematic_rms (the fitted field at the observations),
    explained (in-sample), cv_gain (share of the squared error of held-out frames, fold = frame mod n_folds, that the field
    predicts; about 0 or negative for noise), z (energy of the fit against sigma2, in standard deviations), T, nu, count
    [C, n_folds], outside [C] (observed pixels outside the image), coverage [C, 2, h, w] (inliers | valid but rejected), sigma2).
    Modelling choices: prior_px = the second difference of neighbouring control values thought plausible (1 px); tau0 = 100 px only
    keeps the system positive definite where a camera never saw a board; sigma2 = the residual variance (None: the estimate
    `covariance` uses).  Always the plain (unsharded) handle."""
    from . import residual_field
    if sigma2 is None:
      sigma2 = self.covariance().sigma2
    sizes = [tuple(int(v) for v in cam.image_size) for cam in self.cameras]
    g = self._handle().residual_gram(self.param_vec, sizes, nx=nx, ny=ny, n_folds=n_folds, inliers_only=inliers_only,
                                     coverage=coverage)
    return residual_field.analyse(g.gram, g.count, g.outside, g.coverage, sizes, int(nx), int(ny), sigma2, prior_px=prior_px,
                                  tau0=tau0, grid=grid, pixels=pixels)

  def report_residual_field(self, stage="", **kwargs):
    """One line per camera through the "calibration" logger: n, rms, systematic_rms, cv_gain, z, the largest |field| on the grid and
    where it is.  A camera whose cv_gain exceeds 0.1 AND whose z exceeds 5 gets a warning instead: both thresholds are reporting
    conventions (residual_field.WARN_CV_GAIN, WARN_Z), not tests.  Returns the result of `residual_field(**kwargs)`."""
    from . import residual_field
    out = self.residual_field(**kwargs)
    names = getattr(self.camera_poses, "names", None) or [f"cam{i}" for i in range(self.size.cameras)]
    for line, warn in residual_field.report_lines(out, names, stage):
      (logger.warning if warn else info)(line)
    return out

  # --- applying the residual field -----------------------------------------------------------------
  def _image_sizes(self):
    return [tuple(int(v) for v in cam.image_size) for cam in self.cameras]

  def _uncorrected(self):
    """this calibration on its raw observation table, at the current parameters"""
    if self.correction is None:
      return self
    d = self.__getstate__()
    d.update(point_table=self.raw_point_table, correction=None, raw_point_table=None)
    return Calibration(**d)

  def residual_correction(self, **fit_kwargs):
    """The correction.FieldCorrection of `residual_field(**fit_kwargs).coefficients`: the fitted field as a warp of the image plane,
    w(p) = p + e(p), raw pixel -> the pixel the parametric model explains."""
    from .correction import FieldCorrection
    out = self.residual_field(**fit_kwargs)
    return FieldCorrection(out.coefficients, self._image_sizes(), out.nx, out.ny)

  def with_corrected_observations(self, correction):
    """A copy whose point_table is the RAW observation table warped by `correction` (one device call, mcba_warp_points); it carries
    `correction` and `raw_point_table`, and report, bundle_adjust, covariance, triangulate, localize and residual_field work on it
    unchanged.  On an already corrected calibration the raw table is warped again, never a warp of a warp.  (A later
    copy(point_table=...) keeps the attributes: replace the table through this method only.)"""
    raw = self.point_table if self.correction is None else self.raw_point_table
    return self.copy(point_table=correction.correct_table(raw), correction=correction, raw_point_table=raw)

  def refine_with_residual_field(self, rounds=3, sigma2=None, **kwargs):
    """Alternates, `rounds` times: (1) fit the field to the RAW residuals at the current parameters, (2) bundle_adjust on the raw
    table corrected by that field.  nx, ny, n_folds, prior_px and tau0 go to the fit, every other keyword to bundle_adjust.  sigma2
    is fixed at the first round (the caller's value or the `covariance()` estimate); the inlier mask, prior_px and tau0 are held.
    Returns (the corrected calibration, one record per round: struct(sse, penalty, joint = sse + c^T Pen c, rms, systematic_rms,
    cv_gain, z, param_vec)): sse of the corrected table's inliers after the round's adjustment, the per-camera figures of the
    round's fit, param_vec the parameters the round's field was fitted at.

    This is block coordinate descent on J(x, c) = |pi(x) - p - B c|^2 + c^T Pen c -- step (1) minimises over c exactly, step (2)
    over x -- so `joint` cannot rise from round to round, PROVIDED: linear loss, a fixed inlier set, no observation outside the
    image (there the field is the clamped extension, which the fit does not see) and a static motion model.  Under rolling shutter
    the scan time is read from the CORRECTED row, so the two steps minimise slightly different functions."""
    from . import residual_field as rf
    from .correction import FieldCorrection
    fit_kwargs = {k: kwargs.pop(k) for k in ("nx", "ny", "n_folds", "prior_px", "tau0") if k in kwargs}
    assert int(rounds) >= 1, "refine_with_residual_field: at least one round"
    if sigma2 is None:
      sigma2 = self.covariance().sigma2
    sigma2 = float(sigma2)
    current, records = self, []
    for _ in range(int(rounds)):
      raw = current._uncorrected()
      fit = raw.residual_field(sigma2=sigma2, **fit_kwargs)
      correction = FieldCorrection(fit.coefficients, self._image_sizes(), fit.nx, fit.ny)
      current = current.with_corrected_observations(correction).bundle_adjust(**kwargs)
      r = np.asarray(current.residuals(), dtype=np.float64)
      pen = rf.penalty(fit.nx, fit.ny, sigma2, fit.prior_px, fit.tau0)
      sse, penalty = float(r @ r), float(np.einsum("cki,kl,cli->", fit.coefficients, pen, fit.coefficients))
      records.append(struct(sse=sse, penalty=penalty, joint=sse + penalty, rms=fit.rms, systematic_rms=fit.systematic_rms,
                            cv_gain=fit.cv_gain, z=fit.z, param_vec=np.array(raw.param_vec, dtype=np.float64)))
    return current, records

  def report_residual_correction(self, stage=""):
    """One line per camera through the "calibration" logger: the fold bound of its field, the largest |e| on the default grid, the
    reprojection rms of the camera's inliers on the raw and on the corrected table (both at the current parameters)."""
    from . import correction
    assert self.correction is not None, "report_residual_correction: this calibration carries no correction"
    names = getattr(self.camera_poses, "names", None) or [f"cam{i}" for i in range(self.size.cameras)]
    before, after = self._uncorrected().residual_field(sigma2=1.0).rms, self.residual_field(sigma2=1.0).rms
    for line in correction.report_lines(self.correction, names, before, after, stage):
      info(line)

  # --- triangulation through the rig --------------------------------------------------------------
  @cached_property
  def world_points(self):
    """calibration.py:83-90: board points in the rig's world frame, board_pose[b] . X_board: Table(points [B, P, 3], valid [B, P])."""
    B, P = self.size.boards, self.size.points
    pts, valid = np.zeros((B, P, 3)), np.zeros((B, P), dtype=bool)
    for b, board in enumerate(self.boards):
      x = np.asarray(board.adjusted_points, dtype=np.float64)
      pts[b, :len(x)] = x
      valid[b, :len(x)] = True
    poses = np.asarray(self.board_poses.poses, dtype=np.float64)
    world = np.einsum('bij,bpj->bpi', poses[:, :3, :3], pts) + poses[:, None, :3, 3]
    return Table.create(points=world, valid=valid & np.asarray(self.board_poses.valid)[:, None])

  def _rig_poses(self):
    """(start [F, 4, 4], end [F, 4, 4] or None) of the motion model: static, rolling shutter, hand-eye through its pose table"""
    m = self.motion
    if hasattr(m, "pose_start"):
      return np.asarray(m.pose_start), np.asarray(m.pose_end)
    return np.asarray(m.frame_poses.poses), None

  def triangulate(self, inliers_only=True, sigma=None, max_iterations=20, calibration_cov=False, hold=None):
    """Every corner of the point table intersected from the cameras that saw it in its frame (multical_amd.triangulate, one launch,
    M = B * P): Table(points [F, B, P, 3], valid [F, B, P], n_views, cov [F, B, P, 3, 3], status, error [C, F, B, P]) in the frame
    of `world_points`.  The mask is `inliers` (inliers_only) or `valid`; a corner is valid where the triangulation converged, which
    takes two cameras at least.  `cov` is the pixel noise of the corner alone; calibration_cov=True adds cov_cal [F, B, P, 3, 3], the
    covariance of the same corner under `covariance(hold)` of the intrinsics and camera poses (multical_amd.reconstruction, one more
    launch over the valid corners, the views offered to each corner, in the frame of `cov`; NaN where the corner is not valid or its
    calibration part is not defined).  For corners with non-zero residuals cov_cal is the Gauss-Newton approximation at the
    model-projected pixels; it is common to all corners and does not average out."""
    from . import triangulate as tri
    C, F, B, P = self.point_table.valid.shape
    mask = self.inliers if inliers_only else self.valid
    start, end = self._rig_poses()
    view_valid = np.asarray(self.camera_poses.valid)[:, None] & np.asarray(self.motion.valid)[None, :]
    r = tri.triangulate_rig(self.cameras, self.camera_poses.poses, start, np.asarray(self.point_table.points).reshape(C, F, B * P, 2),
                            np.asarray(mask).reshape(C, F, B * P), rig_poses_end=end, view_valid=view_valid, sigma=sigma,
                            max_iterations=max_iterations)
    out = Table.create(points=r.points.reshape(F, B, P, 3), valid=(r.status == tri.OK).reshape(F, B, P),
                       n_views=r.n_views.reshape(F, B, P), cov=r.cov.reshape(F, B, P, 3, 3), status=r.status.reshape(F, B, P),
                       error=r.error.reshape(C, F, B, P))
    if not calibration_cov:
      return out
    offered = np.asarray(mask).reshape(C, F, B, P) & view_valid[:, :, None, None]
    return Table(out._extend(cov_cal=self._triangulated_cov_cal(out.points, out.valid, offered, start, hold)))

  def _triangulated_cov_cal(self, points, valid, offered, rig_poses, hold):
    """cov_cal [F, B, P, 3, 3] of the world points [F, B, P, 3] that are `valid`, seen through the cameras offered [C, F, B, P] in
    frames at rig_poses [F, 4, 4]: one job of all cameras over the valid corners in the rig frame of their frame, turned back"""
    from . import reconstruction
    C = offered.shape[0]
    if C > reconstruction.MAX_CAMERAS:
      raise ValueError(f"triangulate(calibration_cov=True): {C} cameras; a group has at most {reconstruction.MAX_CAMERAS}")
    f, b, p = np.nonzero(valid)
    R, t = np.asarray(rig_poses)[f, :3, :3], np.asarray(rig_poses)[f, :3, 3]
    X = np.einsum("nij,nj->ni", R, points[f, b, p]) + t
    masks = (offered[:, f, b, p].astype(np.uint64) << np.arange(C, dtype=np.uint64)[:, None]).sum(axis=0).astype(np.uint64)
    u = self._reconstruction_uncertainty(self.covariance(hold=hold), None, None, X, masks, margin=1e9)
    cal = np.full(valid.shape + (3, 3), np.nan)
    cal[f, b, p] = np.einsum("nji,njk,nkl->nil", R, u.cov_cal, R)
    return cal

  def reconstruction_error(self, inliers_only=True):
    """How good the calibration is in the units of the boards: the distance of every triangulated corner from where the rig chain
    puts it (world_points[b, p]).  struct(error [F, B, P] (0 where invalid), valid, n_views, overall, boards): `overall` and
    boards[b] are error_stats of the valid corners (mse, rms, quantiles 0 .25 .5 .75 1, n)."""
    t = self.triangulate(inliers_only=inliers_only)
    world = self.world_points
    valid = t.valid & world.valid[None]
    with np.errstate(invalid="ignore"):
      dist = np.linalg.norm(t.points - world.points[None], axis=-1)
    dist = np.where(valid, dist, 0.0)
    boards = [error_stats(dist[:, b][valid[:, b]]) for b in range(self.size.boards)]
    return struct(error=dist, valid=valid, n_views=t.n_views, overall=error_stats(dist[valid]), boards=boards)

  def report_reconstruction(self, stage="", inliers_only=True):
    """One line through the "calibration" logger: RMS, median and largest 3-D distance between triangulated and predicted corners in
    millimetres (boards in metres), and how many corners two cameras or more saw."""
    r = self.reconstruction_error(inliers_only=inliers_only)
    n = int(r.valid.sum())
    if n == 0:
      info(f"{stage} reconstruction: no corner was seen by 2 or more cameras")
      return
    q = r.overall.quantiles
    info(f"{stage} reconstruction RMS={1e3 * r.overall.rms:.3f} mm, median={1e3 * q[2]:.3f} mm, max={1e3 * q[4]:.3f} mm, "
         f"n={n} corners seen by >= 2 cameras")


  # --- localising the rig in other frames ---------------------------------------------------------
  def localize(self, point_table=None, inliers_only=True, init=None, sigma=None, max_iterations=20):
    """The rig pose of every frame of `point_table` from that frame's detections alone, cameras, camera poses, boards and board
    poses held (multical_amd.localize, one workgroup per frame).  Default table: the calibration's own, over its inliers
    (inliers_only) or valid points, started from the current poses of the motion model.  Another table is started from its own views
    unless init ([F, 4, 4], or (start, end) under rolling shutter) is given.  A RollingFrames motion gives start and end poses; a
    HandEye motion is localised as static frames.  Returns the struct of localize.localize_rig."""
    from . import localize as loc
    own = point_table is None
    table = self.point_table if own else point_table
    rolling = hasattr(self.motion, "pose_start")
    shared = np.asarray(self.camera_poses.valid)[:, None, None, None] & np.asarray(self.board_poses.valid)[None, None, :, None]
    mask = (self.inliers if inliers_only else self.valid) if own else (np.asarray(table.valid) & shared)
    start, end = (None, None)
    if init is not None:
      start, end = init if isinstance(init, (tuple, list)) else (init, None)
    elif own:
      start, end = self._rig_poses()
    return loc.localize_rig(self.cameras, self.camera_poses.poses, self.board_poses.poses,
                            [np.asarray(b.adjusted_points, dtype=np.float64) for b in self.boards], table.points, mask, init=start,
                            init_end=end if rolling else None, rolling=rolling, sigma=sigma, max_iterations=max_iterations)

  def with_localized_frames(self, point_table, names=None):
    """A new Calibration with the same cameras, camera poses, boards and board poses over the frames of `point_table`: the motion is
    StaticFrames / RollingFrames of the localised poses, valid where the localisation converged (a HandEye calibration yields
    StaticFrames).  report(), reprojection_error, reject_outliers, reconstruction_error() and bundle_adjust then work on the held-out
    table unchanged."""
    from . import localize as loc
    from .motion import RollingFrames, StaticFrames
    r = self.localize(point_table)
    ok = r.status == loc.OK
    names = list(names) if names is not None else [str(i) for i in range(len(ok))]
    if r.poses_end is not None:
      motion = RollingFrames(r.poses, r.poses_end, ok, names, getattr(self.motion, "max_iterations", 4))
    else:
      motion = StaticFrames(Table.create(poses=r.poses, valid=ok), names)
    return self.copy(point_table=point_table, motion=motion, inlier_mask=None)

  def report_holdout(self, point_table, stage=""):
    """One line through the "calibration" logger: frames localised / total, RMS and quantiles of the held-out reprojection error
    (pixels, over the observations of the localised frames) and the median standard deviation of the frames' translations (board
    units, sqrt of the trace of the translation block of each frame's covariance)."""
    from . import localize as loc
    r = self.localize(point_table)
    ok = r.status == loc.OK
    entered = (r.error > 0) & ok[None, :, None, None]
    stats = error_stats(r.error[entered])
    with np.errstate(invalid="ignore"):
      t_std = np.sqrt(np.trace(r.cov[:, 3:6, 3:6], axis1=1, axis2=2))[ok]
    med = float(np.median(t_std)) if t_std.size else float("nan")
    info(f"{stage} held-out: {int(ok.sum())} / {len(ok)} frames localised, reprojection RMS={stats.rms:.3f}, n={stats.n}, "
         f"quantiles={stats.quantiles}, median translation std={med:.6f}")
    return r

  # --- every camera pair on its own, beside the rig ------------------------------------------------
  PAIR_WARN_SCALE = 5.0      # reporting convention of report_pairwise_extrinsics: scaled difference above which a pair is pointed at

  def pairwise_extrinsics(self, min_views=3, inliers_only=True, min_common=4, sigma=None):
    """The relative pose of every camera pair from that pair's own common views (multical_amd.stereo: cameras held, one workgroup
    per pair, all pairs in one launch), set beside the rig's camera_poses[j] @ inv(camera_poses[i]).  It says WHICH pair disagrees
    with the joint bundle adjustment: a camera that was bumped, a wrong spanning-tree edge of the initialisation, a pair whose
    overlap is too thin to trust.  The views start from the calibration's own chain camera . rig . board (the start pose under rolling
    shutter), over its inliers (inliers_only) or valid points.

    Returns the struct of stereo.calibrate_pairs (pairs i < j of valid cameras with a common view) extended by
      T_rig [n, 4, 4]        the rig's relative pose of the pair
      rotation_mrad [n]      rotation angle between the pair's estimate and the rig's, milliradians
      translation_mm [n]     norm of the translation difference, in 1/1000 of the boards' unit (mm for boards in metres)
      rotation_scaled, translation_scaled [n]   the differences in units of the pair's own standard deviation:
                             sqrt(d^T C^-1 d) with C the rotation / translation block of the pair's covariance and d taken in the
                             covariance's own parameters (stereo.scaled_difference: difference of the global rotation vectors)
      scaled [n]             the larger of the two
      enough [n]             the pair has a result and at least min_views views
      ranking                indices of the pairs with `enough`, largest scaled difference first
    The scaled difference is a SCALE, not a test: the two estimates share their data (the rig's comes from the same detections and
    more), so it does not follow a chi distribution.  The pair model is static: under a rolling shutter it ignores the readout."""
    from . import stereo
    cam_ok, board_ok = np.asarray(self.camera_poses.valid).astype(bool), np.asarray(self.board_poses.valid).astype(bool)
    start, _ = self._rig_poses()
    chain = (np.asarray(self.camera_poses.poses)[:, None, None] @ np.asarray(start)[None, :, None] @
             np.asarray(self.board_poses.poses)[None, None, :])
    view_valid = cam_ok[:, None, None] & np.asarray(self.motion.valid).astype(bool)[None, :, None] & board_ok[None, None, :]
    mask = np.asarray(self.inliers if inliers_only else self.valid).astype(bool)
    board_points = [np.asarray(b.adjusted_points, dtype=np.float64) for b in self.boards]
    pairs = stereo.common_view_pairs(mask, view_valid, min_common, stereo.pad_boards(board_points, mask.shape[3])[0])
    r = stereo.calibrate_pairs(self.cameras, board_points, self.point_table.points, mask, chain, view_valid, pairs,
                               min_common=min_common, sigma=sigma)
    poses = np.asarray(self.camera_poses.poses)
    T_rig = poses[pairs[:, 1]] @ np.linalg.inv(poses[pairs[:, 0]]) if len(pairs) else np.zeros((0, 4, 4))
    have = (r.status == stereo.OK) | (r.status == stereo.NOT_CONVERGED)
    # (the covariance is over the global rotation vector and the translation of T: the differences are taken in those parameters)
    diff = stereo.scaled_difference(r.T, T_rig, r.cov)
    angle = np.zeros(0)
    if len(pairs):
      angle = np.linalg.norm(stereo.rotation_vectors(r.T[:, :3, :3] @ np.swapaxes(T_rig[:, :3, :3], -1, -2)).reshape(-1, 3), axis=1)
    d_t = diff.d_t
    rot_s, t_s = np.where(have, diff.rotation, np.nan), np.where(have, diff.translation, np.nan)
    both = np.fmax(rot_s, t_s)
    enough = have & (r.n_views >= min_views) & np.isfinite(both)
    idx = np.flatnonzero(enough)
    ranking = idx[np.argsort(-both[idx], kind="stable")]
    return r._extend(T_rig=T_rig, rotation_mrad=np.where(have, 1e3 * angle, np.nan),
                     translation_mm=np.where(have, 1e3 * np.linalg.norm(d_t, axis=1), np.nan), rotation_scaled=rot_s,
                     translation_scaled=t_s, scaled=both, enough=enough, ranking=ranking)

  def report_pairwise_extrinsics(self, stage="", min_views=3):
    """One line per camera pair through the "calibration" logger: views and points, the pair's RMS, the rotation (mrad) and
    translation (mm) between the pair's own estimate and the rig's, and both in units of the pair's own standard deviation; pairs with
    fewer than min_views views are listed as thin.  A warning goes to the pair with the largest scaled difference when it exceeds
    Calibration.PAIR_WARN_SCALE (5): a reporting convention, not a test -- see pairwise_extrinsics.  Returns its struct."""
    r = self.pairwise_extrinsics(min_views=min_views)
    names = list(getattr(self.cameras, "names", [str(c) for c in range(len(self.cameras))]))
    if hasattr(self.motion, "pose_start"):
      info(f"{stage} pairwise extrinsics: the pair model is static and ignores the rolling-shutter readout; differences of the size of "
           "the motion during a frame are expected")
    for k, (i, j) in enumerate(r.pairs):
      thin = "" if r.enough[k] else " (thin: not ranked)"
      info(f"{stage} pair {names[i]}-{names[j]}: views={int(r.n_views[k])}, points={int(r.n_points[k])}, rms={r.rms[k]:.3f}, "
           f"rotation={r.rotation_mrad[k]:.3f} mrad ({r.rotation_scaled[k]:.1f} sd), translation={r.translation_mm[k]:.3f} mm "
           f"({r.translation_scaled[k]:.1f} sd){thin}")
    if len(r.ranking) and r.scaled[r.ranking[0]] > self.PAIR_WARN_SCALE:
      i, j = r.pairs[r.ranking[0]]
      logger.warning(
          f"{stage} pair {names[i]}-{names[j]} disagrees with the rig by {r.scaled[r.ranking[0]]:.1f} of its own standard deviations "
          f"(reporting convention: above {self.PAIR_WARN_SCALE:g})")
    return r

  # --- projection uncertainty where no board was ----------------------------------------------------
  def _shared_layout(self):
    """(camera_index, pose_index): per camera, where its stored block (fx fy cx cy skew dist..) and its pose (rvec | tvec) sit in
    param_vec -- the layout split_std walks; None for a block that is not optimised"""
    pos, out = 0, dict(cameras=None, camera_poses=None)
    for k in ("camera_poses", "board_poses", "motion", "cameras", "boards"):
      if self.optimize[k] is not True:
        continue
      if k == "camera_poses":
        out[k] = [np.arange(pos + 6 * c, pos + 6 * c + 6) for c in range(self.size.cameras)]
      elif k == "cameras":
        at, out[k] = pos, []
        for c in self.cameras:
          n = np.asarray(c.param_vec).size
          out[k].append(np.arange(at, at + n))
          at += n
      pos += parameters.count(self.params[k])
    return out["cameras"], out["camera_poses"]

  def projection_uncertainty(self, cameras=None, reference=None, distance=np.inf, grid=(16, 12), pixels=None, hold=None, sigma2=None):
    """How far the calibration can be trusted anywhere in the image: the 2 x 2 covariance of where a point projects into each of
    `cameras` (indices; None: all) when intrinsics and camera poses vary with `covariance(hold, sigma2)` (multical_amd.uncertainty,
    one covariance and one device call).  reference=None: the point behind each pixel at `distance` is fixed in the rig frame -- with
    the default hold that is the frame of the held camera, whose own map is then intrinsics-only; reference=a: camera a sees the
    point at that pixel, the result is where each camera sees it (transfer / epipolar uncertainty, gauge-free; 0 for a itself).
    grid=(gw, gh): centres u_i = (i + 0.5) W / gw - 0.5 (grid=image_size: every pixel); pixels [n, 2] with one camera: a list.
    Returns struct(cov [C', gh, gw, 2, 2], std [C', gh, gw] (sqrt of the larger eigenvalue), pixels [C', gh, gw, 2], status
    (uncertainty.OK / NOT_CONVERGED / BEHIND / UNCONSTRAINED; NaN where not OK), sigma2, dof)."""
    from . import uncertainty
    if self.optimize["boards"] is True:
      raise ValueError("projection_uncertainty: not supported with the boards block optimised (the board points would join the "
                       "shared system, as for prediction_covariance)")
    return self._projection_uncertainty(self.covariance(hold=hold, sigma2=sigma2), cameras, reference, distance, grid, pixels)

  def _projection_uncertainty(self, cov, cameras, reference, distance, grid, pixels):
    from . import uncertainty
    camera_index, pose_index = self._shared_layout()
    rtvecs = np.asarray(self.camera_poses.params, dtype=np.float64).reshape(-1, 6)
    out = uncertainty.projection_uncertainty(list(self.cameras), np.asarray(self.camera_poses.poses), cov, camera_index, pose_index,
                                             query_cameras=cameras, reference=reference, distance=distance, grid=grid, pixels=pixels,
                                             rtvecs=rtvecs)
    return out._extend(sigma2=cov.sigma2, dof=cov.dof)

  def report_projection_uncertainty(self, stage="", reference=None, distance=np.inf):
    """One line per camera through the "calibration" logger: the standard deviation (px) of a projected point at the image centre,
    its median and its worst value over the default 16 x 12 grid with the pixel where that occurs, and the share of grid cells
    whose standard deviation is below the residual sigma."""
    if self.optimize["boards"] is True:
      raise ValueError("report_projection_uncertainty: not supported with the boards block optimised")
    cov = self.covariance()
    u = self._projection_uncertainty(cov, None, reference, distance, (16, 12), None)
    sigma = float(np.sqrt(u.sigma2))
    names = getattr(self.camera_poses, "names", None) or [f"cam{i}" for i in range(self.size.cameras)]
    for c in range(self.size.cameras):
      w, h = self.cameras[c].image_size
      mid = self._projection_uncertainty(cov, [c], reference, distance, None, [[0.5 * (w - 1), 0.5 * (h - 1)]]).std[0]
      std = u.std[c]
      ok = np.isfinite(std)
      if not ok.any():
        info(f"{stage} {names[c]}: projection uncertainty not defined (no grid cell is constrained)")
        continue
      worst = np.unravel_index(np.nanargmax(std), std.shape)
      at = u.pixels[c][worst]
      info(f"{stage} {names[c]}: projected std centre={float(mid):.4f} median={float(np.median(std[ok])):.4f} "
           f"max={float(std[worst]):.4f} px at ({at[0]:.0f}, {at[1]:.0f}), {100.0 * float((std[ok] < sigma).mean()):.0f}% of cells "
           f"below sigma={sigma:.3f} px")
    return u

  # --- 3-D uncertainty of triangulated points -----------------------------------------------------
  def _median_board_distance(self, a):
    """median distance of the board centres from camera a over the views of the point table in which a saw the board"""
    start, _ = self._rig_poses()
    seen = np.asarray(self.point_table.valid)[a].any(axis=-1) & np.asarray(self.motion.valid)[:, None] & \
        np.asarray(self.board_poses.valid)[None, :]
    f, b = np.nonzero(seen)
    if len(f) == 0:
      return float("nan")
    centres = np.array([np.asarray(bd.adjusted_points, dtype=np.float64).reshape(-1, 3).mean(axis=0) for bd in self.boards])
    T = np.asarray(self.camera_poses.poses)[a][None] @ np.asarray(start)[f] @ np.asarray(self.board_poses.poses)[b]
    at = np.einsum("nij,nj->ni", T[:, :3, :3], centres[b]) + T[:, :3, 3]
    return float(np.median(np.linalg.norm(at, axis=1)))

  def _reconstruction_uncertainty(self, cov, cameras, reference, points, masks=None, pixels=None, grid=(16, 12), distances=None,
                                  margin=0.0):
    from . import reconstruction
    camera_index, pose_index = self._shared_layout()
    rtvecs = np.asarray(self.camera_poses.params, dtype=np.float64).reshape(-1, 6)
    out = reconstruction.reconstruction_uncertainty(list(self.cameras), np.asarray(self.camera_poses.poses), cov, camera_index, pose_index,
                                                    group=cameras, reference=reference, points=points, pixels=pixels, grid=grid,
                                                    distances=distances, masks=masks, margin=margin, rtvecs=rtvecs)
    return out._extend(sigma2=cov.sigma2, dof=cov.dof)

  def reconstruction_uncertainty(self, cameras=None, reference=None, distances=None, grid=(16, 12), points=None, hold=None,
                                 sigma2=None):
    """How well the rig measures 3-D: the 3 x 3 covariance of the point that the group `cameras` (2 .. 8 indices; None: all)
    triangulates, under `covariance(hold, sigma2)` of the intrinsics and camera poses (cov_cal: systematic, the same for every point
    of a scene, growing with the square of the distance) beside the pixel noise of the point alone (cov_noise, what triangulate()
    reports) (multical_amd.reconstruction, one covariance and one device call).  reference=None: the point in the rig frame;
    reference=a: in the frame of camera a of the group, the gauge-free form.  points [n, 3] in the rig frame, or the centres of
    `grid` in the image of the reference camera (None: the first of the group) at every one of `distances` from it (None: 0.5, 1, 2,
    4, 8 x the median distance of the boards it saw).  A camera is a view of a point where the point projects into its image.
    Returns struct(cov_cal, cov_noise, cov_total [.., 3, 3], n_views, views, status (reconstruction.OK / TOO_FEW / DEGENERATE /
    UNCONSTRAINED; NaN where not OK), points, range_std_cal, lateral_std_cal, range_std_noise, lateral_std_noise (along / across the
    line from the reference origin), r, distances, sigma2, dof); leading shape [n] or [D, gh, gw].  Exact for the point triangulated
    from its noise-free pixels; the Gauss-Newton approximation at the model-projected pixels for a point with residuals.  The motion
    model plays no part; correlations between points are not returned here (differences of nearby points are better than cov_cal
    says): length_uncertainty / length_errors."""
    if self.optimize["boards"] is True:
      raise ValueError("reconstruction_uncertainty: not supported with the boards block optimised (the board points would join the "
                       "shared system, as for projection_uncertainty)")
    if points is None and distances is None:
      members = list(range(self.size.cameras)) if cameras is None else [int(c) for c in np.atleast_1d(cameras)]
      a = members[0] if reference is None else int(reference)
      distances = np.array([0.5, 1.0, 2.0, 4.0, 8.0]) * self._median_board_distance(a)
    u = self._reconstruction_uncertainty(self.covariance(hold=hold, sigma2=sigma2), cameras, reference, points, grid=grid,
                                         distances=distances)
    return u._extend(distances=None if distances is None else np.asarray(distances, dtype=np.float64))

  def report_reconstruction_uncertainty(self, stage="", reference=None):
    """One line per camera pair (reference, b) through the "calibration" logger: at 0.5, 1, 2, 4 and 8 x the median distance of the
    boards the reference camera saw, on the ray of its image centre, the range error of the pair's triangulated point from the
    calibration / from the pixel noise of one point, in millimetres (boards in metres), and the distance at which the calibration's
    part overtakes the noise (interpolated between the five on a logarithmic scale)."""
    if self.optimize["boards"] is True:
      raise ValueError("report_reconstruction_uncertainty: not supported with the boards block optimised")
    from . import reconstruction
    a = 0 if reference is None else int(reference)
    cov = self.covariance()
    names = getattr(self.camera_poses, "names", None) or [f"cam{i}" for i in range(self.size.cameras)]
    w, h = self.cameras[a].image_size
    d = np.array([0.5, 1.0, 2.0, 4.0, 8.0]) * self._median_board_distance(a)
    out = {}
    for b in range(self.size.cameras):
      if b == a:
        continue
      u = self._reconstruction_uncertainty(cov, [a, b], a, None, pixels=[[0.5 * (w - 1), 0.5 * (h - 1)]], distances=d)
      out[b] = u
      cal, noise, ok = u.range_std_cal[:, 0], u.range_std_noise[:, 0], u.status[:, 0] == reconstruction.OK
      if not ok.any():
        info(f"{stage} {names[a]}-{names[b]}: range uncertainty not defined (no distance is seen by both and constrained)")
        continue
      cells = " ".join(f"{1e3 * cal[i]:.3f}/{1e3 * noise[i]:.3f}@{d[i]:.2f}" if ok[i] else f"-@{d[i]:.2f}" for i in range(len(d)))
      with np.errstate(invalid="ignore", divide="ignore"):
        lr = np.where(ok, np.log(cal / noise), np.nan)
      cross = f"calibration {'above' if np.nanmin(lr) > 0 else 'below'} the noise of one point at every distance"
      for i in range(len(d) - 1):
        if np.isfinite(lr[i]) and np.isfinite(lr[i + 1]) and (lr[i] <= 0) != (lr[i + 1] <= 0):
          at = float(np.exp(np.log(d[i]) - lr[i] / (lr[i + 1] - lr[i]) * np.log(d[i + 1] / d[i])))
          cross = (f"calibration overtakes the noise of one point at {at:.2f}" if lr[i] <= 0 else
                   f"calibration above the noise of one point up to {at:.2f}")
          break
      info(f"{stage} {names[a]}-{names[b]}: range std calibration/noise mm@distance {cells}; {cross}")
    return out

  # --- uncertainty of measured lengths: covariance between triangulated points ----------------------
  def _pair_uncertainty(self, cov, cameras, reference, points, pairs, masks=None, margin=0.0):
    from . import reconstruction
    camera_index, pose_index = self._shared_layout()
    rtvecs = np.asarray(self.camera_poses.params, dtype=np.float64).reshape(-1, 6)
    out = reconstruction.pair_uncertainty(list(self.cameras), np.asarray(self.camera_poses.poses), cov, camera_index, pose_index,
                                          points=points, pairs=pairs, group=cameras, reference=reference, masks=masks, margin=margin,
                                          rtvecs=rtvecs)
    return out._extend(sigma2=cov.sigma2, dof=cov.dof)

  def length_uncertainty(self, points_a, points_b, cameras=None, reference=None, hold=None, sigma2=None):
    """How well the rig measures the LENGTH between points_a [K, 3] and points_b [K, 3] (rig frame, as reconstruction_uncertainty(
    points=..)) triangulated by the group `cameras` (2 .. 8 indices; None: all) under `covariance(hold, sigma2)`.  The calibration's
    error is common to both ends and largely cancels in their difference, so the result is far below sqrt(var_a + var_b) of the
    per-point cov_cal (multical_amd.reconstruction.pair_uncertainty, one covariance and one device call).
    Returns its struct: cov_diff_cal, cov_diff_noise, cov_diff_total, cross_cal [K, 3, 3], length, length_std_cal, length_std_noise,
    length_std [K], status, views_a, views_b, r; and sigma2, dof.  To first order the length's standard deviations do not depend on
    `reference` or on which camera pose is held."""
    if self.optimize["boards"] is True:
      raise ValueError("length_uncertainty: not supported with the boards block optimised (the board points would join the shared "
                       "system, as for reconstruction_uncertainty)")
    a, b = np.asarray(points_a, dtype=np.float64).reshape(-1, 3), np.asarray(points_b, dtype=np.float64).reshape(-1, 3)
    assert len(a) == len(b), "one b end per a end"
    pairs = np.stack([np.arange(len(a)), len(a) + np.arange(len(a))], axis=1)
    return self._pair_uncertainty(self.covariance(hold=hold, sigma2=sigma2), cameras, reference, np.concatenate([a, b]), pairs)

  def length_pairs(self, pairs=None):
    """(pairs [B, K, 2], defined [B, K]) of length_errors: `pairs` [K, 2] (corner indices, the same for every board) or [B, K, 2]; the
    default is one pair per corner p of each board: (p, the corner farthest from p in the board's own geometry, ties to the lowest
    index) -- deterministic, and independent of which corners were seen.  defined: both corners exist on the board."""
    from . import reconstruction
    B, P = self.size.boards, self.size.points
    n = [len(np.asarray(b.adjusted_points).reshape(-1, 3)) for b in self.boards]
    if pairs is None:
      out = np.zeros((B, P, 2), dtype=np.int64)
      for b, board in enumerate(self.boards):
        out[b, :n[b]] = reconstruction.farthest_corner_pairs(board.adjusted_points)
      defined = np.arange(P)[None, :] < np.array(n)[:, None]
      return out, defined
    out = np.asarray(pairs, dtype=np.int64)
    out = np.broadcast_to(out, (B,) + out.shape[-2:]).copy()
    assert out.ndim == 3 and out.shape[2] == 2, "pairs is [K, 2] or [B, K, 2]"
    defined = ((out >= 0) & (out < np.array(n)[:, None, None])).all(axis=2)
    return np.where(defined[:, :, None], out, 0), defined

  def length_errors(self, inliers_only=True, pairs=None, hold=None):
    """The boards as rulers: for every frame and board the distance between the triangulated corners (triangulate()) of each pair of
    `pairs` (length_pairs: [K, 2] corner indices per board; default: every corner with the corner farthest from it), against the
    board's own distance, in units of its predicted standard deviation under `covariance(hold)` -- the first check of the chain
    covariance -> rig factors -> reconstruction against real detections, in metres.  One device call over the pairs whose two corners
    are valid in the frame, each corner with the views the triangulation offered it, as triangulate(calibration_cov=True) does.
    Returns struct(length, board_length, error = length - board_length, std_cal, std_noise, studentized = error / sqrt(std_cal^2 +
    std_noise^2) [F, B, K] (0 / NaN where not valid), valid [F, B, K]: both corners are valid in the frame and the pair's status is
    OK, status [F, B, K] (reconstruction.OK ..; 255: not launched), pairs [B, K, 2], overall = error_stats(|error| of the valid
    pairs)).
    The corners are IN-SAMPLE: the frame poses and the calibration were fitted to the same detections, and the pixel noise of a corner
    is partly absorbed by them, so studentised errors below 1 are expected.  with_localized_frames(held_out_table).length_errors()
    is the honest form.  The covariance does not contain the frame poses (they move both ends rigidly) nor the boards."""
    if self.optimize["boards"] is True:
      raise ValueError("length_errors: not supported with the boards block optimised (the board points would join the shared system, "
                       "as for reconstruction_uncertainty)")
    from . import reconstruction
    C, F, B, P = self.point_table.valid.shape
    if C > reconstruction.MAX_CAMERAS:
      raise ValueError(f"length_errors: {C} cameras; a group has at most {reconstruction.MAX_CAMERAS}")
    pair_table, defined = self.length_pairs(pairs)
    K = pair_table.shape[1]
    t = self.triangulate(inliers_only=inliers_only)
    ia, ib = pair_table[None, :, :, 0], pair_table[None, :, :, 1]
    bi = np.arange(B)[None, :, None]
    fi = np.arange(F)[:, None, None]
    both = t.valid[fi, bi, ia] & t.valid[fi, bi, ib] & defined[None]
    board_xyz = np.zeros((B, P, 3))
    for b, board in enumerate(self.boards):
      x = np.asarray(board.adjusted_points, dtype=np.float64).reshape(-1, 3)
      board_xyz[b, :len(x)] = x
    board_length = np.broadcast_to(np.linalg.norm(board_xyz[bi, ia] - board_xyz[bi, ib], axis=-1), (F, B, K)).copy()
    shape = (F, B, K)
    length, std_cal, std_noise = np.zeros(shape), np.full(shape, np.nan), np.full(shape, np.nan)
    status = np.full(shape, 255, dtype=np.uint8)
    f, b, k = np.nonzero(both)
    if len(f):
      # the corners that occur in a launched pair, once each, in the rig frame of their frame
      used = np.zeros((F, B, P), dtype=bool)
      used[f, b, pair_table[b, k, 0]] = True
      used[f, b, pair_table[b, k, 1]] = True
      uf, ub, up = np.nonzero(used)
      index = np.full((F, B, P), -1, dtype=np.int64)
      index[uf, ub, up] = np.arange(len(uf))
      start, _ = self._rig_poses()
      R, tr = np.asarray(start)[uf, :3, :3], np.asarray(start)[uf, :3, 3]
      X = np.einsum("nij,nj->ni", R, t.points[uf, ub, up]) + tr
      mask = self.inliers if inliers_only else self.valid
      view_valid = np.asarray(self.camera_poses.valid)[:, None] & np.asarray(self.motion.valid)[None, :]
      offered = np.asarray(mask).reshape(C, F, B, P) & view_valid[:, :, None, None]
      masks = (offered[:, uf, ub, up].astype(np.uint64) << np.arange(C, dtype=np.uint64)[:, None]).sum(axis=0).astype(np.uint64)
      launched = np.stack([index[f, b, pair_table[b, k, 0]], index[f, b, pair_table[b, k, 1]]], axis=1)
      u = self._pair_uncertainty(self.covariance(hold=hold), None, None, X, launched, masks, margin=1e9)
      length[f, b, k], std_cal[f, b, k], std_noise[f, b, k], status[f, b, k] = u.length, u.length_std_cal, u.length_std_noise, u.status
    valid = both & (status == reconstruction.OK)
    error = np.where(both, length - board_length, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
      studentized = np.where(valid, error / np.sqrt(std_cal ** 2 + std_noise ** 2), np.nan)
    return struct(length=length, board_length=board_length, error=error, std_cal=std_cal, std_noise=std_noise, studentized=studentized,
                  valid=valid, status=status, pairs=pair_table, overall=error_stats(np.abs(error[valid])))

  def report_length_uncertainty(self, stage="", length=None, reference=None):
    """One line per camera pair (reference, b) through the "calibration" logger: a bar of `length` (default: the largest board's
    diagonal) centred on the ray of the reference camera's image centre at 0.5, 1, 2, 4 and 8 x the median distance of the boards it
    saw, across and along the line of sight: the standard deviation of its measured length from the calibration / from the pixel
    noise of its two ends, in millimetres (boards in metres), and beside them the naive sqrt(var_a + var_b) of the two ends'
    cov_cal along the bar, which ignores that the calibration's error is common to both.  One more line: RMS and median |.| of
    length_errors().studentized (in-sample, see there).  Returns {b: the struct of the pair's call}."""
    if self.optimize["boards"] is True:
      raise ValueError("report_length_uncertainty: not supported with the boards block optimised")
    from . import reconstruction
    a = 0 if reference is None else int(reference)
    cov = self.covariance()
    names = getattr(self.camera_poses, "names", None) or [f"cam{i}" for i in range(self.size.cameras)]
    if length is None:
      diagonals = [np.asarray(bd.adjusted_points, dtype=np.float64).reshape(-1, 3) for bd in self.boards]
      length = max(float(np.linalg.norm(x[:, None] - x[None], axis=-1).max()) for x in diagonals)
    length = float(length)
    w, h = self.cameras[a].image_size
    d = np.array([0.5, 1.0, 2.0, 4.0, 8.0]) * self._median_board_distance(a)
    poses = np.asarray(self.camera_poses.poses, dtype=np.float64)
    centre = reconstruction.grid_points(list(self.cameras), poses, a, np.array([[0.5 * (w - 1), 0.5 * (h - 1)]]), d)[:, 0]
    Ta = np.linalg.inv(poses[a])
    along = (centre - Ta[:3, 3]) / np.linalg.norm(centre - Ta[:3, 3], axis=1, keepdims=True)
    across = np.cross(along, Ta[:3, :3] @ np.array([0.0, 1.0, 0.0]))
    across /= np.linalg.norm(across, axis=1, keepdims=True)
    D = len(d)
    # points: [across | along] x [a end | b end] x D; pairs: the bar, and each end with itself (cross_cal of (p, p) is its cov_cal)
    ends = np.concatenate([centre - 0.5 * length * across, centre + 0.5 * length * across, centre - 0.5 * length * along,
                           centre + 0.5 * length * along])
    ea = np.concatenate([np.arange(D), 2 * D + np.arange(D)])
    eb = ea + D
    pairs = np.concatenate([np.stack([ea, eb], axis=1), np.stack([ea, ea], axis=1), np.stack([eb, eb], axis=1)])
    out = {}
    for b in range(self.size.cameras):
      if b == a:
        continue
      u = self._pair_uncertainty(cov, [a, b], a, ends, pairs)
      out[b] = u
      n = 2 * D
      ok = (u.status[:n] == reconstruction.OK) & (u.status[n:2 * n] == reconstruction.OK) & (u.status[2 * n:] == reconstruction.OK)
      if not ok.any():
        info(f"{stage} {names[a]}-{names[b]}: length uncertainty not defined (no bar is seen by both and constrained)")
        continue
      T = poses[a]
      unit = np.einsum("ij,nj->ni", T[:3, :3], (ends[eb] - ends[ea]) / length)
      with np.errstate(invalid="ignore"):
        naive = np.sqrt(np.einsum("ni,nij,nj->n", unit, u.cross_cal[n:2 * n] + u.cross_cal[2 * n:], unit))
      cell = lambda i: (f"{1e3 * u.length_std_cal[i]:.4f}/{1e3 * u.length_std_noise[i]:.4f}/{1e3 * naive[i]:.3f}@{d[i % D]:.2f}"
                        if ok[i] else f"-@{d[i % D]:.2f}")
      info(f"{stage} {names[a]}-{names[b]}: std of a {1e3 * length:.0f} mm length, calibration/noise/naive sqrt(var_a + var_b) "
           f"mm@distance, across {' '.join(cell(i) for i in range(D))}; along {' '.join(cell(D + i) for i in range(D))}")
    e = self.length_errors()
    s = e.studentized[e.valid]
    if s.size == 0:
      info(f"{stage} board lengths: no pair of corners was triangulated")
    else:
      info(f"{stage} board lengths (in-sample): studentised error RMS={float(np.sqrt(np.mean(s ** 2))):.3f}, "
           f"median |.|={float(np.median(np.abs(s))):.3f}, n={s.size} pairs; length error RMS={1e3 * e.overall.rms:.3f} mm")
    return out

  # --- comparing two calibrations -----------------------------------------------------------------
  def _other_rig(self, other):
    """(cameras, camera_poses [C, 4, 4]) of `other` in this calibration's camera order: a Calibration (same order), or what
    import_calib.load_calibration returns (matched by name)"""
    if isinstance(other, Calibration):
      if other.size.cameras != self.size.cameras:
        raise ValueError(f"projection_diff: {self.size.cameras} and {other.size.cameras} cameras")
      return list(other.cameras), np.asarray(other.camera_poses.poses)
    names, theirs = list(self.camera_poses.names), list(other.names)
    missing = [n for n in names if n not in theirs]
    if missing:
      raise ValueError(f"projection_diff: the other calibration has no camera {missing} (it has {theirs})")
    pick = [theirs.index(n) for n in names]
    return [other.cameras[i] for i in pick], np.asarray(other.camera_poses, dtype=np.float64)[pick]

  def projection_diff(self, other, cameras=None, reference=None, distance=np.inf, grid=(16, 12), pixels=None, fit="auto",
                      fit_grid=(60, 40), focus=None, sigmas=False):
    """Where `other` (calibration 1: a Calibration, or what import_calib.load_calibration returns, matched by camera name) projects
    what this calibration (0) sees at a pixel, as a map over the image of each of `cameras` (multical_amd.compare, one device call).
    reference=None: the intrinsics difference behind the implied transform fitted over `fit_grid` inside `focus` = (u, v, radius)
    (fit: "auto" = "rotation" at infinity, "rigid" at a finite distance; "none"); reference=a: the transfer difference against
    camera a -- has the camera moved against a? -- with `landing`, where the point is seen under this calibration.  Returns
    struct(diff, magnitude, landing, pixels, status, transform, fit) as compare.projection_diff does.
    sigmas=True (transfer mode only): adds d = sqrt(diff^T (C0 + C1)^-1 diff), C^k each calibration's own
    projection_uncertainty(reference=a) at the same pixels; both sides must be Calibrations with observations (ValueError
    otherwise).  d is calibrated -- chi-distributed with two degrees of freedom under agreement -- ONLY when the two calibrations
    come from independent data sets: two fits of the same detections share their noise, and d then overstates the agreement."""
    from . import compare
    cams1, poses1 = self._other_rig(other)
    out = compare.projection_diff(list(self.cameras), np.asarray(self.camera_poses.poses), cams1, poses1, query_cameras=cameras,
                                  reference=reference, distance=distance, grid=grid, pixels=pixels, fit=fit, fit_grid=fit_grid,
                                  focus=focus)
    if not sigmas:
      return out
    if reference is None:
      raise ValueError("projection_diff: sigmas=True needs a reference camera (the fit of the intrinsics mode absorbs part of the "
                       "difference, so C0 + C1 is not its covariance)")
    if not isinstance(other, Calibration) or not np.asarray(other.point_table.valid).any() or not np.asarray(self.point_table.valid).any():
      raise ValueError("projection_diff: sigmas=True needs two Calibrations with observations (each side's covariance comes from "
                       "its own data)")
    u0, u1 = (c.projection_uncertainty(cameras=cameras, reference=reference, distance=distance, grid=grid, pixels=pixels)
              for c in (self, other))
    return out._extend(d=compare.significance(out.diff, u0.cov, u1.cov), cov0=u0.cov, cov1=u1.cov)

  def report_projection_diff(self, other, stage="", reference=None, distance=np.inf):
    """One line per camera through the "calibration" logger: median and maximum |diff| (px) over the default 16 x 12 grid, the value
    at the image centre, the implied rotation in mrad (and the translation in mm -- board units x 1000 -- at a finite distance) and
    the RMS over the fit pixels before -> after the fit; in transfer mode the fit figures are left out."""
    from . import compare
    r = self.projection_diff(other, reference=reference, distance=distance)
    names = getattr(self.camera_poses, "names", None) or [f"cam{i}" for i in range(self.size.cameras)]
    for c in range(self.size.cameras):
      mag = r.magnitude[c]
      ok = r.status[c] == compare.OK
      if not ok.any():
        why = "the fit of the implied transform failed" if (r.status[c] == compare.NO_FIT).all() else "no grid cell is OK"
        info(f"{stage} {names[c]}: projection difference not defined ({why})")
        continue
      w, h = self.cameras[c].image_size
      mid = self.projection_diff(other, cameras=[c], reference=reference, distance=distance, pixels=[[0.5 * (w - 1), 0.5 * (h - 1)]],
                                 fit_grid=(60, 40)).magnitude[0]
      line = (f"{stage} {names[c]}: projection difference median={float(np.median(mag[ok])):.4f} max={float(mag[ok].max()):.4f} "
              f"centre={float(mid):.4f} px")
      if reference is None:
        t = r.transform[c]
        line += f", implied rotation={1e3 * float(np.linalg.norm(t[:3])):.4f} mrad"
        if not np.isinf(distance):
          line += f", translation={1e3 * float(np.linalg.norm(t[3:])):.4f} mm"
        line += f", fit RMS {float(r.fit.rms_before[c]):.4f} -> {float(r.fit.rms_after[c]):.4f} px over {int(r.fit.n_fit[c])} pixels"
      info(line)
    return r

  # --- planning the next captures -----------------------------------------------------------------
  def suggest_views(self, n=3, cameras=None, board=0, candidates=None, focus_grid=(16, 12), focus_distance=np.inf, criterion="focus",
                    hold=None, sigma2=None):
    """Where to hold board `board` next: per camera of `cameras` (indices; None: all) the n candidate views that, one after the
    other, reduce the RMS projection uncertainty over the focus grid most (criterion="focus"; after the implied rotation -- or, at
    a finite focus_distance, rigid motion -- is fitted out) or carry the most information on its intrinsics (criterion="gain"),
    under `covariance(hold, sigma2)` (multical_amd.guidance, one covariance and one device call).  A candidate is a static capture
    in a new frame with a free rig pose, seen by that camera alone; candidates: None (guidance.candidate_poses) or {camera: poses
    [m, 4, 4] board in camera}.  Returns struct(cameras, poses [C', n, 4, 4], candidate_index, gain [C', n] (nats, each conditional
    on the earlier picks), focus_rms_before [C'], focus_rms_after [C', n] (px), n_visible, status (guidance.OK / TOO_FEW /
    UNCONSTRAINED), candidates, scores, sigma2, dof)."""
    from . import guidance
    if self.optimize["boards"] is True:
      raise ValueError("suggest_views: not supported with the boards block optimised (the board points would join the shared "
                       "system, as for projection_uncertainty)")
    cov = self.covariance(hold=hold, sigma2=sigma2)
    camera_index, _ = self._shared_layout()
    out = guidance.suggest_views(list(self.cameras), cov, camera_index, list(self.boards), n=n, query_cameras=cameras, board=board,
                                 candidates=candidates, focus_grid=focus_grid, focus_distance=focus_distance, criterion=criterion)
    return out._extend(sigma2=cov.sigma2, dof=cov.dof)

  def report_view_suggestions(self, stage="", n=3, board=0, criterion="focus"):
    """One line per camera and pick through the "calibration" logger: the distance of the board's centre, the image region it
    lands in (a 3 x 3 naming of where its centre projects), its tilt against the optical axis, the information gain and the focus
    RMS before -> after the pick in px."""
    from . import guidance
    s = self.suggest_views(n=n, board=board, criterion=criterion)
    names = getattr(self.camera_poses, "names", None) or [f"cam{i}" for i in range(self.size.cameras)]
    pts = np.asarray(self.boards[board].adjusted_points, dtype=np.float64).reshape(-1, 3)
    centre = 0.5 * (pts.min(axis=0) + pts.max(axis=0))
    for i, c in enumerate(s.cameras):
      if s.status[i] != guidance.OK:
        why = "an intrinsic is unconstrained" if s.status[i] == guidance.UNCONSTRAINED else "no candidate is usable"
        info(f"{stage} {names[c]}: no view suggested ({why})")
        continue
      before = float(s.focus_rms_before[i])
      for k in range(n):
        if s.candidate_index[i, k] < 0:
          break
        T = s.poses[i, k]
        X = T[:3, :3] @ centre + T[:3, 3]
        w, h = self.cameras[c].image_size
        K = np.asarray(self.cameras[c].intrinsic, dtype=np.float64)
        u, v = K[0, 0] * X[0] / X[2] + K[0, 2], K[1, 1] * X[1] / X[2] + K[1, 2]
        col = ("left", "centre", "right")[int(np.clip(3.0 * u / w, 0, 2))]
        row = ("top", "middle", "bottom")[int(np.clip(3.0 * v / h, 0, 2))]
        tilt = float(np.degrees(np.arccos(np.clip(abs(T[2, 2]), 0.0, 1.0))))
        after = float(s.focus_rms_after[i, k])
        info(f"{stage} {names[c]} view {k + 1}: board at distance={float(np.linalg.norm(X)):.3f}, {row} {col}, tilt={tilt:.0f} deg, "
             f"{int(s.n_visible[i, k])} corners, gain={float(s.gain[i, k]):.3f} nats, focus RMS {before:.4f} -> {after:.4f} px")
        before = after
    return s

  # --- views that several cameras see --------------------------------------------------------------
  def suggest_rig_views(self, n=3, cameras=None, reference=None, board=0, candidates=None, focus_grid=(16, 12), focus_distance=None,
                        criterion="focus", min_cameras=2, hold=None, sigma2=None):
    """Where to hold board `board` next so that the RIG gets better: the n candidate views that, one after the other, reduce most
    the RMS transfer uncertainty from camera `reference` (None: the first of the group) into every other camera of the group
    `cameras` (indices; None: all) over the focus grid at `focus_distance` (criterion="focus"), or carry the most information on
    the group's intrinsics and camera poses together (criterion="gain"), under `covariance(hold, sigma2)` (multical_amd.guidance,
    one covariance and one device call).  A candidate is a static capture in a new frame with a free rig pose, seen by every camera
    of the group whose image it falls into, at least `min_cameras` of them; candidates: None (guidance.rig_candidate_poses) or poses
    [m, 4, 4] board in rig.  focus_distance=None: the median distance of the candidates' board centres from the reference camera
    (reported).  A group whose joint factor has more than guidance.RIG_MAX_R = 128 columns is refused: pass a smaller cameras=.
    Returns struct(cameras, reference, focus_distance, poses [n, 4, 4] board in rig, camera_poses_of_board [n, C', 4, 4] board in
    each camera of the group, candidate_index [n], gain [n] (nats, each conditional on the earlier picks), focus_rms_before,
    focus_rms_after [n] (px), n_cameras [n], n_visible [n, C'], status (guidance.OK / TOO_FEW / UNCONSTRAINED), candidates, scores,
    sigma2, dof)."""
    from . import guidance
    cov = self.covariance(hold=hold, sigma2=sigma2)
    camera_index, pose_index = self._shared_layout()
    rtvecs = np.asarray(self.camera_poses.params, dtype=np.float64).reshape(-1, 6)
    out = guidance.suggest_rig_views(list(self.cameras), np.asarray(self.camera_poses.poses), cov, camera_index, pose_index,
                                     list(self.boards), n=n, group=cameras, reference=reference, board=board, candidates=candidates,
                                     focus_grid=focus_grid, focus_distance=focus_distance, criterion=criterion, min_cameras=min_cameras,
                                     rtvecs=rtvecs, boards_free=self.optimize["boards"] is True)
    return out._extend(sigma2=cov.sigma2, dof=cov.dof)

  def report_rig_view_suggestions(self, stage="", n=3, board=0, criterion="focus", cameras=None, reference=None):
    """One line per pick through the "calibration" logger: which cameras see it (with their corner counts), the distance of the
    board's centre from the reference camera, its tilt against that camera's optical axis, the information gain and the focus RMS
    (transfer uncertainty from the reference camera) before -> after the pick in px."""
    from . import guidance
    s = self.suggest_rig_views(n=n, board=board, criterion=criterion, cameras=cameras, reference=reference)
    names = getattr(self.camera_poses, "names", None) or [f"cam{i}" for i in range(self.size.cameras)]
    if s.status != guidance.OK:
      why = "a parameter of the group is unconstrained" if s.status == guidance.UNCONSTRAINED else "no candidate is seen by enough cameras"
      info(f"{stage} rig view: none suggested ({why})")
      return s
    pts = np.asarray(self.boards[board].adjusted_points, dtype=np.float64).reshape(-1, 3)
    centre = 0.5 * (pts.min(axis=0) + pts.max(axis=0))
    ia = list(s.cameras).index(s.reference)
    before = float(s.focus_rms_before)
    for k in range(n):
      if s.candidate_index[k] < 0:
        break
      T = s.camera_poses_of_board[k, ia]
      X = T[:3, :3] @ centre + T[:3, 3]
      tilt = float(np.degrees(np.arccos(np.clip(abs(T[2, 2]), 0.0, 1.0))))
      seen = ", ".join(f"{names[c]} ({int(m)})" for c, m in zip(s.cameras, s.n_visible[k]) if m > 0)
      after = float(s.focus_rms_after[k])
      info(f"{stage} rig view {k + 1}: seen by {seen}; board at distance={float(np.linalg.norm(X)):.3f} from {names[s.reference]}, "
           f"tilt={tilt:.0f} deg, gain={float(s.gain[k]):.3f} nats, transfer RMS at {s.focus_distance:.3f} {before:.4f} -> {after:.4f} px")
      before = after
    return s


def split_std(calib, std):
  """A vector over calib.param_vec (standard deviations) split into the enabled blocks: camera_poses [C, 6], board_poses
  [B, 6], motion (static [F, 6]; rolling shutter [start [F, 6], end [F, 6]]; hand-eye struct(world_wrt_base [6],
  gripper_wrt_camera [6])), cameras (one array per camera: fx fy cx cy skew dist..), boards (one [P_b, 3] array per board)."""
  blocks = parameters.split(np.asarray(std, dtype=np.float64), calib.params)
  out = struct()
  for k, v in blocks.items():
    if k in ("camera_poses", "board_poses"):
      v = v.reshape(-1, 6)
    elif k == "motion":
      mp = calib.motion.params
      v = parameters.split(v, mp)
      if not isinstance(mp, Struct):
        v = v.reshape(-1, 6) if isinstance(v, np.ndarray) else [a.reshape(-1, 6) for a in v]
    elif k == "cameras":
      v = parameters.split(v, [np.asarray(c.param_vec) for c in calib.cameras])
    elif k == "boards":
      v = [a.reshape(-1, 3) for a in parameters.split(v, [np.asarray(b.param_vec) for b in calib.boards])]
    out[k] = v
  return out


# ---------------------------------------------------------------------------------------------------------------
# builder from a synthetic rig (multical_amd.synthetic.make_rig)
# ---------------------------------------------------------------------------------------------------------------
def from_rig(rig, which='init'):
  from .board import Board
  from .camera import Camera, CameraFisheye
  from .motion import StaticFrames, RollingFrames, HandEye
  from .parameters import ParamList
  from .pose_set import PoseSet

  src = getattr(rig, which)
  C, F, B, P = rig.valid.shape
  cam_names = [f"cam{i}" for i in range(C)]
  board_names = [f"board{i}" for i in range(B)]
  frame_names = [f"frame{i}" for i in range(F)]
  cameras = []
  for c in src.cameras:
    if c.model == 'fisheye':
      cameras.append(CameraFisheye(c.image_size, c.intrinsic, c.dist, fix_aspect=c.fix_aspect, has_skew=c.has_skew))
    else:
      cameras.append(Camera(c.image_size, c.intrinsic, c.dist, model=c.model, fix_aspect=c.fix_aspect,
                            has_skew=c.has_skew))
  boards = [Board(p, name=n) for p, n in zip(rig.board_points, board_names)]
  kind = rig.cfg["motion"]
  if kind == 'static':
    motion = StaticFrames(Table.create(poses=src.rig, valid=rig.frame_valid), frame_names)
  elif kind == 'rolling':
    motion = RollingFrames(src.rig, src.rig_end, rig.frame_valid, frame_names)
  else:
    he = src.hand_eye
    motion = HandEye(Table.create(poses=he.base_wrt_gripper, valid=rig.frame_valid), he.world_wrt_base,
                     he.gripper_wrt_camera, frame_names)
  calib = Calibration(ParamList(cameras, cam_names), ParamList(boards, board_names),
                      Table.create(points=rig.points, valid=rig.valid),
                      PoseSet(Table.create(poses=src.camera_poses, valid=rig.camera_valid), cam_names),
                      PoseSet(Table.create(poses=src.board_poses, valid=rig.board_valid), board_names), motion)
  return calib.enable(**rig.optimize)
