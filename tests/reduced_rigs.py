"""TEST INFRASTRUCTURE: synthetic rigs chosen by the SHAPE OF THEIR REDUCED SYSTEM -- the width ns of the Schur complement (shared
parameters: camera poses, board poses, intrinsics; for hand-eye motion all parameters), the size DF of an eliminated frame block (6 static,
12 rolling shutter, 0 hand-eye) and the number of frames F, so that K = DF F rows are eliminated -- for the kernels between the per-view
kernels and the Cholesky factorisation: k_schur_frame, k_schur_syrk<true|false>, k_schur_syrk3, k_schur_reduce, k_schur_backsub and the
covariance route k_cov_trinv / k_schur_syrk on L^-1 / k_cov_fold / k_cov_frame<DF>.

The rigs come from synthetic.make_rig unchanged, with 81-point charuco_10x10 boards and no gross outliers.  What a target fixes is
(ns, motion, F); the numbers of cameras and boards and the distortion model that give that ns are ENUMERATED below:

    ns = 6 C [camera poses] + 6 B [board poses] + C (5 + number of distortion coefficients)     static, rolling
    ns = n = 6 B + 12 [world_wrt_base, gripper_wrt_camera] + the same camera blocks             hand-eye

with the camera blocks absent when the intrinsics are fixed: 9 entries for pin4, 10 standard, 13 rational, 17 thin-prism, 19 tilted.
One width the targets need has no such rig: ns = 32.  (ns = 2 mod 6 asks for camera blocks that sum to 2 mod 6; the shortest
such list, of one model or mixed, is two `standard` cameras, 20 entries, and 6 (2 + B) + 20 = 32 or 6 B + 12 + 20 = 32 leaves
no board.)  There the enumeration falls back to the same kind of rig with its camera poses held fixed
(`optimize["camera_poses"] = False`, the block a hand-eye calibration holds fixed too): ns = 6 B + camera blocks.  Every other target
is met with the camera poses optimised.

For a target the helper walks the compositions in order of preference and, for each, the frame counts of the target and a short
list of seeds in turn, and takes the first rig in which every frame, every camera and every board has a view; it asserts what it
found.  The results are cached and their tables are read-only.  The conditions a rig has to meet beyond that (condition numbers,
pivots, share of unobserved parameters) need the normal equations: tests/test_reduced_rigs_host.py checks them on the CPU."""
import functools
import itertools
from collections import namedtuple

from multical_amd import synthetic

BOARD = "charuco_10x10"
# entries of an optimised camera block: 5 (fx fy cx cy skew) + distortion coefficients
BLOCK = {model: 5 + synthetic.DIST_SIZE[model] for model in ("pin4", "standard", "rational", "thin_prism", "tilted")}
DF = dict(static=6, rolling=12, hand_eye=0)
SEEDS = range(71, 83)
MAX_CAMERAS, MAX_BOARDS = 10, 8
TILE = 16

Target = namedtuple("Target", "name ns motion frames step cov cross layout cameras boards model fixed")


def target(ns, motion, frames, step=False, cov=False, cross=False, layout="stereo", cameras=None, boards=None, model=None, fixed=False):
  """frames: a number, or a tuple of frame counts tried in turn; cameras / boards / model: given counts and ONE distortion model for all
  cameras (the two large rigs), else enumerated; fixed: intrinsics not optimised"""
  frames = tuple(frames) if isinstance(frames, (tuple, list, range)) else (int(frames),)
  tag = "F%d" % frames[0] if len(frames) == 1 else "F%d+" % frames[0]
  return Target(f"ns{ns}-{motion}-{tag}", ns, motion, frames, step, cov, cross, layout, cameras, boards, model, fixed)


# ---- the targets --------------------------------------------------------------------------------------------------------------------
# Step route: ncol = ns + 1 columns of W' = [W | y], ntile = ceil(ncol / 16), K = DF F.  ksplit doubles while K / (2 ksplit) >= 32 under
# k_schur_syrk (K >= 64: 2, K >= 128: 4) and while K / (8 ksplit) >= 16 under k_schur_syrk3 (K >= 128: 2).
# Covariance route: tiles of ns itself, nsp = 16 ceil(ns / 16).  Rolling-shutter rigs with free intrinsics do not meet the condition
# number the covariance route asks for (1e7 where 1e6 is the limit, whatever the composition), so the rolling covariance rigs have
# fixed intrinsics, ns = 6 (C + B); ns = 60 is there for them (an even number of column tiles, which 12 and 48 do not give).
TARGETS = [
  #      ns   motion      F                                      ncol  ntile  K    what the rig is there for
  target(12, "static", 1, step=True, cov=True, cross=True),    # 13    1     6    the smallest rig, one frame; nsp/16 = 1
  target(30, "rolling", 1, step=True),                         # 31    2     12
  target(31, "hand_eye", 8, step=True, cov=True),              # 32    2     0    no frame blocks, ncol on a tile edge; DF = 0 covariance
  target(32, "static", 5, step=True),                          # 33    3     30   K below one 32-row MFMA batch (camera poses fixed, see above)
  target(62, "static", 10, step=True),                         # 63    4     60   ksplit 1, the last K before the first doubling
  target(63, "static", 11, step=True, cov=True),               # 64    4     66   ksplit 2, per = 36 rows (not the split length 33)
  target(64, "rolling", 5, step=True),                         # 65    5     60
  target(126, "static", 21, step=True),                        # 127   8     126  ksplit 2, the last K before the second doubling
  target(127, "static", 22, step=True),                        # 128   8     132  ksplit 4; ntile 8: the last size on k_schur_syrk
  target(128, "static", 2, step=True),                         # 129   9     12   the first size on k_schur_syrk3; a wavefront without rows
  target(158, "static", 3, step=True),                         # 159   10    18   ntile % 3 = 1: the last 48-column block holds one tile; lone tail batches
  target(159, "rolling", 3, step=True),                        # 160   10    36   the last size on the LDS Cholesky; 12 rows per wavefront: a half-masked batch
  target(160, "rolling", 11, step=True),                       # 161   11    132  the first size on the panel Cholesky; syrk3 ksplit 2
  target(174, "static", 1, step=True),                         # 175   11    6    ntile % 3 = 2; six rows: 4 + 2, two wavefronts without rows
  target(175, "static", 6, step=True),                         # 176   11    36
  target(176, "rolling", 6, step=True),                        # 177   12    72   ntile % 3 = 0
  #                                                              nsp/16
  target(31, "static", 6, cov=True, cross=True),               # 2     fewer column tiles than k_cov_frame has wavefronts
  target(32, "static", 3, cov=True, cross=True),               # 2     ns on a tile edge (camera poses fixed, see above)
  target(33, "static", 6, cov=True),                           # 3     one column in the last tile
  target(47, "static", 8, cov=True, cross=True),               # 3     an odd number of column tiles
  target(48, "rolling", 1, cov=True, cross=True, fixed=True),  # 3     DF = 12, one frame
  target(49, "static", 9, cov=True),                           # 4     as many column tiles as wavefronts
  target(60, "rolling", 5, cov=True, cross=True, fixed=True),  # 4     DF = 12, an even number of column tiles
  target(64, "static", 7, cov=True, cross=True),               # 4
  target(65, "static", 8, cov=True),                           # 5     more column tiles than wavefronts
  target(79, "hand_eye", 10, cov=True),                        # 5     DF = 0, one column short of a tile edge
  target(80, "static", 10, cov=True, cross=True),              # 5     ns on a tile edge
  target(81, "static", 12, cov=True, cross=True),              # 6
  # the documented limit of the covariance, ns + 1 <= 1024: 39 / 40 `tilted` cameras (6 + 19 entries each) in a ring around 5 boards.
  # (`standard` cameras would leave their skew entries, 6 % of the shared parameters, unobserved; with three frames the condition
  #  number of such a rig is 1e9, with eight it meets the limit of 1e6 -- about 23 000 residuals.)
  target(6 * 44 + 19 * 39, "static", 8, cov=True, layout="ring", cameras=39, boards=5, model="tilted"),     # ns = 1005
  target(6 * 45 + 19 * 40, "static", 3, layout="ring", cameras=40, boards=5, model="tilted"),               # ns = 1030: refused
]
NAMES = [t.name for t in TARGETS]
assert len(set(NAMES)) == len(NAMES)
BY_NAME = dict(zip(NAMES, TARGETS))
STEP = [t.name for t in TARGETS if t.step]
COVARIANCE = [t.name for t in TARGETS if t.cov]
LARGE, REFUSED = NAMES[-2], NAMES[-1]
assert 1000 <= BY_NAME[LARGE].ns <= 1023 and BY_NAME[REFUSED].ns >= 1024


def expected_ns(motion, cameras, boards, models, camera_poses):
  """the formula of the module docstring (the lowering: n_params - n_motion, n_motion = DF F)"""
  intrinsics = 0 if models is None else sum(BLOCK[m] for m in models)
  if motion == "hand_eye":
    return 6 * boards + 12 + intrinsics
  return (6 * cameras if camera_poses else 0) + 6 * boards + intrinsics


def compositions(t):
  """(C, B, models or None, camera_poses) with expected_ns == t.ns, most preferred first: camera poses optimised (hand-eye never
  optimises them), then few boards beyond four (a fifth board of a flat grid is rarely in view), the shorter distortion model (the
  oracle's 3-point differences, the reference of the host test, are too noisy in the columns of k3 .. k6 and the tilt where a single frame
  observes them), few cameras, few boards.  Covariance rigs take few cameras first: every camera block has one entry no observation
  moves, the skew, and the share of such parameters is bounded there; then the models whose last coefficient can stay free in the
  covariance (covariance_hold).  All cameras of a rig have the same model: the reference's own sparsity_matrix reshapes the cameras block
  to [C, -1], so only rigs with camera blocks of one size can be pinned to it."""
  found = []
  for C in ([t.cameras] if t.cameras else range(1, MAX_CAMERAS + 1)):
    for B in ([t.boards] if t.boards else range(1, MAX_BOARDS + 1)):
      for camera_poses in ([False] if t.motion == "hand_eye" else [True, False]):
        rest = t.ns - expected_ns(t.motion, C, B, None, camera_poses)
        if rest == 0 and t.model is None:
          found.append((C, B, None, camera_poses))
        elif rest >= C * min(BLOCK.values()) and not t.fixed:
          for models in ([(t.model,) * C] if t.model else [(m,) * C for m in BLOCK]):
            if sum(BLOCK[m] for m in models) == rest:
              found.append((C, B, models, camera_poses))
  order = list(BLOCK)
  model = lambda c: -1 if c[2] is None else order.index(c[2][0])
  held = lambda c: c[2] is not None and c[2][0] not in ("rational", "thin_prism")      # (see covariance_hold)
  key = lambda c: (not c[3] and t.motion != "hand_eye", max(0, c[1] - 4)) + ((c[0], held(c), c[1], model(c)) if t.cov else (model(c), c[0], c[1]))
  return sorted(found, key=key)


def config(t, comp, frames, seed):
  C, B, models, camera_poses = comp
  cfg = dict(cameras=C, frames=frames, boards=[BOARD] * B, motion=t.motion, model="standard" if models is None else list(models),
             optimize_cameras=models is not None, layout=t.layout, seed=seed)
  if t.layout != "ring" and B > 1:       # boards on a flat grid seen from further away, as in the many-pairs fixture
    cfg.update(board_grid=2 if B <= 4 else 3, distance=1.6 if B <= 4 else 2.2)
  return cfg


def _freeze(rig):
  """the rigs are cached and shared by every test of a process: an accidental write is an error, not a dependency between tests"""
  rig.valid.flags.writeable = False
  rig.points.flags.writeable = False
  return rig


def _covered(rig):
  """every frame, every camera and every board has at least one view"""
  views = rig.valid.any(axis=-1)        # [C, F, B]
  return bool(views.any(axis=(0, 2)).all() and views.any(axis=(1, 2)).all() and views.any(axis=(0, 1)).all())


@functools.lru_cache(maxsize=None)
def reduced_rig(name):
  """The rig of a target (by name): the first of (one of the four preferred compositions) x (frame count) x (seed) whose rig has a
  view in every frame, on every camera and of every board.  rig.target is the target, rig.composition = (C, B, models, camera
  poses optimised), rig.shape = (ns, DF, F, K)."""
  t = BY_NAME[name]
  comps = compositions(t)[:4]
  assert comps, f"{name}: no rig of at most {MAX_CAMERAS} cameras and {MAX_BOARDS} boards has ns = {t.ns}"
  rig = None
  for comp, frames, seed in itertools.product(comps, t.frames, SEEDS):
    cand = synthetic.make_rig(config(t, comp, frames, seed), outlier_frac=0.0)
    if _covered(cand):
      rig = cand
      break
  assert rig is not None, f"{name}: none of {comps} has a view in every frame, on every camera and of every board at seeds {SEEDS}"
  C, B, models, camera_poses = comp
  if not camera_poses:
    rig.optimize = dict(rig.optimize, camera_poses=False)
  assert expected_ns(t.motion, C, B, models, camera_poses) == t.ns
  assert rig.valid.shape[:3] == (C, frames, B) and frames in t.frames
  assert rig.optimize["cameras"] is (models is not None) and rig.cfg["motion"] == t.motion
  if models is not None:
    assert [c.dist.size for c in rig.init.cameras] == [synthetic.DIST_SIZE[m] for m in models]
  rig.name = "reduced_" + name
  rig.target = t
  rig.composition = comp
  rig.shape = (t.ns, DF[t.motion], frames, DF[t.motion] * frames)
  return _freeze(rig)


# ---- the damped steps and the covariance holds of a rig, from the host build's H ---------------------------------------------------
REG_LADDER = (1e-3, 1e-2, 1e-1, 1.0)
STEP_CONDITION = 1e-10      # cond(D H D + reg I) 2^-52 n: a hundredth of the step's tolerance, so the reference alone stays inside it
COV_CONDITION, COV_PIVOT2 = 1e6, 1e-8     # (the pivot: 100 times COV_PIVOT_MIN, no rig sits on the refusal threshold)
UNOBSERVED_SHARE = 0.05


def jacobi(H):
  """(D H D, D) with D = diag(H)^-1/2, 1 where the diagonal is zero"""
  import numpy as np
  s = np.sqrt(np.diag(H))
  s[s == 0] = 1
  d = 1 / s
  return H * d[:, None] * d[None, :], d


def step_regs(H):
  """[(reg, cond(D H D + reg I) 2^-52 n)]: the two smallest dampings of REG_LADDER that meet STEP_CONDITION"""
  import numpy as np
  ev = np.linalg.eigvalsh(jacobi(H)[0])
  lo, hi, n = max(float(ev[0]), 0.0), float(ev[-1]), H.shape[0]
  found = [(reg, (hi + reg) / (lo + reg) * 2.0 ** -52 * n) for reg in REG_LADDER]
  found = [f for f in found if f[1] <= STEP_CONDITION][:2]
  assert len(found) == 2, (H.shape, found)
  return found


def covariance_conditions(H, hold):
  """(condition number, smallest squared Cholesky pivot, number of free parameters) of the Jacobi-scaled free Hessian"""
  import numpy as np
  diag = np.diag(H)
  free = np.flatnonzero(~hold & (diag > 0))
  Hf = jacobi(H[np.ix_(free, free)])[0]
  try:
    pivot2 = float((np.diag(np.linalg.cholesky(Hf)) ** 2).min())
  except np.linalg.LinAlgError:
    pivot2 = 0.0
  return float(np.linalg.cond(Hf)), pivot2, free.size


def covariance_hold(rig, c, H):
  """gauge.default_hold, plus -- where the intrinsics are optimised -- the distortion coefficients as far as needed (c: the mirror
  Calibration, H: the host build's at x0).  With all of them free no rig meets COV_CONDITION (1e14 .. 1e17).  Held parameters are unit
  rows of the reduced system, and the cameras block is the END of the shared vector: with every coefficient held the last columns of
  the last tile carry nothing, and a kernel that mistreats them goes unnoticed.  So the LAST coefficient of every camera stays free
  where the rig still meets COV_CONDITION and COV_PIVOT2 then (k6 of the rational and s4 of the thin-prism model do; the tilt and p2
  of a 4-coefficient camera do not), else all are held (_hold_distortion)."""
  from multical_amd import gauge
  from test_gpu_covariance import _hold_distortion, parameters_count
  hold = gauge.default_hold(c)
  if not rig.optimize["cameras"]:
    return hold
  hold = _hold_distortion(c, hold)
  fewer = hold.copy()
  pos = sum(parameters_count(c, k) for k in ("camera_poses", "board_poses", "motion") if c.optimize[k] is True)
  for cam in c.cameras:
    pos += len(cam.param_vec)
    fewer[pos - 1] = False
  cond, pivot2, _ = covariance_conditions(H, fewer)
  return fewer if cond <= COV_CONDITION and pivot2 >= COV_PIVOT2 else hold


# ---- what the handle does with a shape: the rules of mcba_create and launch_schur_syrk, restated for the records -------------------
def ntile(ns):
  return (ns + 1 + TILE - 1) // TILE


def syrk_form(ns, K, mfma=True, syrk3=None):
  """syrk3: None = the handle's own choice, True / False = forced (MCBA_SYRK3)"""
  if K == 0:
    return "none"
  if not mfma:
    return "k_schur_syrk<false>"
  three = ntile(ns) >= 9 if syrk3 is None else syrk3
  return "k_schur_syrk3" if three else "k_schur_syrk<true>"


def ksplit(ns, K, syrk3=None):
  nt = ntile(ns)
  ks = 1
  if nt >= 9 if syrk3 is None else syrk3:
    nt3 = (nt + 2) // 3
    np3 = nt3 * (nt3 + 1) // 2
    while ks < 64 and np3 * ks < 192 and K // (ks * 8) >= 16:
      ks *= 2
  else:
    nt2 = nt * (nt + 1) // 2
    while ks < 64 and nt2 * ks < 1024 and K // (ks * 2) >= 32:
      ks *= 2
  return ks


def cholesky_form(ns):
  return "LDS" if ns + 1 <= 160 else ("panel" if ns + 1 <= 1024 else "multi-workgroup")
