"""TEST INFRASTRUCTURE: independent numpy restatement of the robot-world hand-eye closed form (Shah) behind mcba_hand_eye.

It shares no code with multical_amd/csrc/mcba_handeye.h and takes other numerical routes: np.linalg.svd of K = sum kron(R_A, R_B)
itself (not the eigenvectors of K^T K), np.linalg.svd for the nearest rotation (not the polar iteration) and np.linalg.lstsq on
the stacked [3n x 6] translation system (not the 6x6 normal equations)."""
import numpy as np

OK, TOO_FEW, DEGENERATE = 0, 1, 2
GAP_TOL = 1e-9 / 2      # on singular values: (s1 - s2) / s1 is half the relative gap of the squared ones
RANK_TOL = 1e-10 / 2    # smallest singular value of the translation system relative to sqrt(n): that of sqrt(I - M M^T)


def inverse(m):
  m = np.asarray(m, dtype=np.float64)
  out = np.zeros(m.shape)
  out[..., :3, :3] = np.swapaxes(m[..., :3, :3], -1, -2)
  out[..., :3, 3] = -np.einsum('...ij,...j->...i', out[..., :3, :3], m[..., :3, 3])
  out[..., 3, 3] = 1.0
  return out


def _rotation(v):
  m = v.reshape(3, 3)
  det = np.linalg.det(m)
  m = m * (np.sign(det) / abs(det) ** (1.0 / 3.0))
  u, _, vt = np.linalg.svd(m)
  r = u @ vt
  return r if np.linalg.det(r) > 0 else None


def solve(A, B):
  """A, B [n, 4, 4] -> (X, Z, status, err [n]); X = Z = identity and err = 0 unless status is OK."""
  A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
  n = len(A)
  X, Z, err = np.eye(4), np.eye(4), np.zeros(n)
  if n < 3:
    return X, Z, TOO_FEW, err
  if not (np.isfinite(A).all() and np.isfinite(B).all()):
    return X, Z, DEGENERATE, err
  RA, RB, tA, tB = A[:, :3, :3], B[:, :3, :3], A[:, :3, 3], B[:, :3, 3]
  K = np.zeros((9, 9))
  for ra, rb in zip(RA, RB):
    K += np.kron(ra, rb)
  U, S, Vt = np.linalg.svd(K)
  if not (S[0] > 0 and S[0] - S[1] > GAP_TOL * S[0]):
    return X, Z, DEGENERATE, err
  RX, RZ = _rotation(Vt[0]), _rotation(U[:, 0])
  if RX is None or RZ is None:
    return X, Z, DEGENERATE, err
  J = np.zeros((3 * n, 6))
  r = np.zeros(3 * n)
  for i in range(n):
    J[3 * i:3 * i + 3, :3] = RA[i]
    J[3 * i:3 * i + 3, 3:] = -np.eye(3)
    r[3 * i:3 * i + 3] = RZ @ tB[i] - tA[i]
  sol, _, _, sv = np.linalg.lstsq(J, r, rcond=None)
  if not (sv[-1] ** 2 / n > 2 * RANK_TOL):
    return X, Z, DEGENERATE, err
  X[:3, :3], X[:3, 3] = RX, sol[:3]
  Z[:3, :3], Z[:3, 3] = RZ, sol[3:]
  err = np.linalg.norm(A @ X - Z @ B, axis=(1, 2))
  return X, Z, OK, err


def batch(table_a, valid_a, table_b, valid_b, index_a, index_b, invert=False, reversed_order=False):
  """The signature of tables.hand_eye_batch, one solve() per problem."""
  table_a, table_b = np.asarray(table_a, dtype=np.float64), np.asarray(table_b, dtype=np.float64)
  n, F = len(index_a), table_a.shape[1]
  X, Z = np.tile(np.eye(4), (n, 1, 1)), np.tile(np.eye(4), (n, 1, 1))
  n_pairs, status, err = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8), np.zeros((n, F))
  for k, (ia, ib) in enumerate(zip(index_a, index_b)):
    f = np.flatnonzero(np.asarray(valid_a[ia]).astype(bool) & np.asarray(valid_b[ib]).astype(bool))
    if reversed_order:
      f = f[::-1]
    a, b = table_a[ia, f], table_b[ib, f]
    if invert:
      a, b = inverse(a), inverse(b)
    X[k], Z[k], status[k], e = solve(a, b)
    n_pairs[k] = len(f)
    err[k, f] = e
  return X, Z, n_pairs, status, err
