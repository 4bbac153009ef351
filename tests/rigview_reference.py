"""TEST INFRASTRUCTURE: an independent numpy restatement of what a view seen by several cameras adds -- it does
not read csrc/mcba_rigview.h and uses no analytic derivative.

  forward     the pixel of board point X in camera c is project(theta_c, T(rvec_c, tvec_c) exp(xi) Z X): guidance_reference's own
              projection, the STORED pose parameters of the camera through Rodrigues' formula, and a rigid motion exp(xi) of the new
              frame in the rig frame (a rotation about the rig's origin and a translation: the nuisance);
  rows        Richardson-extrapolated central differences over all stored parameters of the group (camera block | pose, camera after
              camera: K [2 P', p]) and over xi (E [2 P', 6]), for the points each contributing camera sees;
  Schur       S = (K F)^T (I - Q Q^T) (K F) with Q from a QR of E; the normal-equation route beside it gives the restatement's spread.
"""
import numpy as np

import guidance_reference as gr


def pose_matrix(rt):
  T = np.eye(4)
  T[:3, :3] = gr.rodrigues(np.asarray(rt[:3], dtype=np.float64))
  T[:3, 3] = rt[3:]
  return T


def motion(xi):
  return pose_matrix(xi)


def view(thetas, fish, fix_aspect, rtvecs, points, Z, F, image_size, min_points=4, margin=0.0):
  """(S_qr, S_ne, visible counts [C], contributing [C] bool, |K F|_F^2) of the rig view: board `points` at board-in-rig pose Z, the
  cameras given by their stored blocks thetas[c], flags and stored poses rtvecs [C, 6]; F [p, r] over (theta_c | rtvec_c) per camera"""
  Cn = len(thetas)
  X_rig = np.asarray(points, dtype=np.float64).reshape(-1, 3) @ np.asarray(Z)[:3, :3].T + np.asarray(Z)[:3, 3]
  sizes = [len(t) + 6 for t in thetas]
  x0 = np.concatenate([np.concatenate([thetas[c], rtvecs[c]]) for c in range(Cn)] + [np.zeros(6)])
  steps = np.concatenate([np.concatenate([gr.steps_of(len(thetas[c])), [gr.STEP["pose"]] * 6]) for c in range(Cn)] + [[gr.STEP["pose"]] * 6])
  masks = []
  for c in range(Cn):
    T = pose_matrix(rtvecs[c])
    masks.append(gr.visible(thetas[c], fish[c], fix_aspect[c], X_rig @ T[:3, :3].T + T[:3, 3], image_size, margin))
  counts = np.array([int(m.sum()) for m in masks])
  contributes = (counts >= min_points) & (counts > 0)

  def pixels(x):
    xi = motion(x[-6:])
    Xm = X_rig @ xi[:3, :3].T + xi[:3, 3]
    out, at = [], 0
    for c in range(Cn):
      th, rt = x[at:at + sizes[c] - 6], x[at + sizes[c] - 6:at + sizes[c]]
      at += sizes[c]
      if not contributes[c]:
        continue
      T = pose_matrix(rt)
      out.append(gr.project(th, fish[c], fix_aspect[c], Xm[masks[c]] @ T[:3, :3].T + T[:3, 3]).ravel())
    return np.concatenate(out) if out else np.zeros(0)

  J = gr.richardson(pixels, x0, steps)
  KW, E = J[:, :-6] @ F, J[:, -6:]
  return gr.schur(KW, E) + (counts, contributes, float((KW * KW).sum()))
