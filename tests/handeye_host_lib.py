"""TEST INFRASTRUCTURE: ctypes wrapper of tests/handeye_host (g++ build of multical_amd/csrc/mcba_handeye.h, the mathematics of
mcba_hand_eye) + the fixtures the hand-eye start tests share."""
import ctypes as C

import numpy as np
from scipy.spatial.transform import Rotation

import host_build
from multical_amd import _lib, tables

import pnp_host_lib


_host = host_build.HostLib("handeye_host", "he", extra=dict(
    hand_eye=[C.POINTER(_lib.HandEyeProblem), _lib.c_double_p, _lib.c_double_p, _lib.c_int32_p, _lib.c_uint8_p, _lib.c_double_p, C.c_int32]))
lib, build = _host.lib, _host.build


def hand_eye_batch(table_a, valid_a, table_b, valid_b, index_a, index_b, invert=False, reversed_order=False):
  """The host build behind tables.hand_eye_batch's signature; reversed_order: the pairs are summed last frame first."""
  inp = tables.HandEyeInputs(table_a, valid_a, table_b, valid_b, index_a, index_b, invert)
  X, Z, n_pairs, status, err = inp.outputs()
  s = inp.struct()
  _host.check(lib().he_hand_eye(C.byref(s), _lib.dp(X), _lib.dp(Z), _lib.ip(n_pairs), _lib.up(status), _lib.dp(err),
                                1 if reversed_order else 0))
  return X, Z, n_pairs, status, err


# ---- fixtures ------------------------------------------------------------------------------------------------------------
def random_poses(rng, n, rot_sigma=0.6, trans_sigma=1.0):
  T = np.tile(np.eye(4), (n, 1, 1))
  T[:, :3, :3] = Rotation.from_rotvec(rng.normal(0.0, rot_sigma, (n, 3))).as_matrix()
  T[:, :3, 3] = rng.normal(0.0, trans_sigma, (n, 3))
  return T


def exact_pairs(seed, n):
  """Random X, Z and B_i with rotations N(0, 0.6 rad); A_i = Z B_i X^-1.  Returns A, B [n, 4, 4], X, Z."""
  rng = np.random.default_rng(seed)
  X, Z = random_poses(rng, 2)
  B = random_poses(rng, n)
  A = Z @ B @ np.linalg.inv(X)
  return A, B, X, Z


def interleaved_problem(seed, n_pairs, F=None, n_rows=1):
  """Exact problems of n_pairs usable pairs each, spread over F frames with invalid frames in between (both sides invalid, one
  side invalid): tables [n_rows, F, 4, 4] x 2, validity x 2, truth X, Z [n_rows]."""
  rng = np.random.default_rng(seed)
  F = F or (2 * n_pairs + 7)
  ta, tb = np.tile(np.eye(4), (n_rows, F, 1, 1)), np.tile(np.eye(4), (n_rows, F, 1, 1))
  va, vb = np.zeros((n_rows, F), dtype=bool), np.zeros((n_rows, F), dtype=bool)
  Xs, Zs = np.zeros((n_rows, 4, 4)), np.zeros((n_rows, 4, 4))
  for r in range(n_rows):
    A, B, Xs[r], Zs[r] = exact_pairs(int(rng.integers(1 << 30)), n_pairs)
    use = np.sort(rng.choice(F, n_pairs, replace=False))
    ta[r, use], tb[r, use] = A, B
    va[r, use] = vb[r, use] = True
    rest = np.setdiff1d(np.arange(F), use)
    # frames that are valid on one side only carry a pose there that must not enter
    junk = random_poses(rng, len(rest))
    side = rng.integers(0, 3, len(rest))
    ta[r, rest[side == 1]], va[r, rest[side == 1]] = junk[side == 1], True
    tb[r, rest[side == 2]], vb[r, rest[side == 2]] = junk[side == 2], True
  return ta, va, tb, vb, Xs, Zs


_chains = {}


def camera_board_chain(name="cfg5_40", noise_seed=None):
  """The fixture's truth chain as the (camera, board) x frame table of the camera-pair start: poses [C B, F, 4, 4] board ->
  camera, valid [C B, F] where the fixture observes the view.  noise_seed: every pose perturbed by the rig's pose noise
  (2e-4 rad, 1e-4 m), seeded."""
  key = (name if isinstance(name, str) else id(name), noise_seed)
  if key not in _chains:
    rig = pnp_host_lib.golden_rig(name) if isinstance(name, str) else name     # (a fixture's name, or a rig)
    chain = pnp_host_lib.truth_chain(rig)                       # [C, F, B, 4, 4]
    C_, F, B = chain.shape[:3]
    valid = np.asarray(rig.valid).any(axis=-1)                  # [C, F, B]
    poses = np.ascontiguousarray(np.moveaxis(chain, 2, 1)).reshape(C_ * B, F, 4, 4)
    valid = np.ascontiguousarray(np.moveaxis(valid, 2, 1)).reshape(C_ * B, F)
    if noise_seed is not None:
      rng = np.random.default_rng(noise_seed)
      d = np.tile(np.eye(4), poses.shape[:2] + (1, 1))
      d[..., :3, :3] = Rotation.from_rotvec(rng.normal(0.0, 2e-4, (C_ * B * F, 3))).as_matrix().reshape(C_ * B, F, 3, 3)
      d[..., :3, 3] = rng.normal(0.0, 1e-4, (C_ * B, F, 3))
      poses = d @ poses
    _chains[key] = (poses, valid, rig, (C_, F, B))
  return _chains[key]


def camera_pair_problems(valid, C_, B, min_views=6, min_common=3):
  """Every (master camera, slave camera, master board, slave board) combination the camera-pair start solves: boards with more
  than min_views views of their camera, at least min_common common frames.  Returns index_a, index_b (rows of the [C B, F] table)
  and the (master, slave, boardM, boardS) list."""
  v = np.asarray(valid).reshape(C_, B, -1)
  seen = [[b for b in range(B) if v[c, b].sum() > min_views] for c in range(C_)]
  ia, ib, combos = [], [], []
  for m in range(C_):
    for s in range(C_):
      if s == m:
        continue
      for bm in seen[m]:
        for bs in seen[s]:
          if (v[m, bm] & v[s, bs]).sum() >= min_common:
            ia.append(m * B + bm)
            ib.append(s * B + bs)
            combos.append((m, s, bm, bs))
  return np.array(ia, dtype=np.int32), np.array(ib, dtype=np.int32), combos


def pose_distance(a, b):
  return pnp_host_lib.pose_distance(a, b)


def ref_inverse(m):
  """rigid inverse of [..., 4, 4] poses"""
  return tables.inverse_poses(m)
