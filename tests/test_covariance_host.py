"""Host side of the parameter covariance: the default gauge hold (gauge.default_hold), the split of a standard-deviation
vector into named blocks (calibration.split_std) and the declared C entry points.  No GPU needed."""
import numpy as np
import pytest

from multical_amd import _lib, calibration, gauge, parameters, synthetic
from multical_amd.pose_set import PoseSet
from multical_amd.structs import Table


def _calib(name):
  return calibration.from_rig(synthetic.make_rig(name))


def _offsets(c):
  out, pos = {}, 0
  for k in ("camera_poses", "board_poses", "motion", "cameras", "boards"):
    if c.optimize[k] is True:
      n = parameters.count(c.params[k])
      out[k] = (pos, n)
      pos += n
  return out


def _invalidate_first(ps):
  valid = np.asarray(ps.valid).copy()
  valid[0] = False
  return PoseSet(Table.create(poses=np.asarray(ps.poses), valid=valid), ps.names)


FLAGS = [dict(camera_poses=cp, board_poses=bp, motion=m, cameras=ci)
         for cp in (True, False) for bp in (True, False) for m in (True, False) for ci in (True, False)]


@pytest.mark.parametrize("name", ["tiny", "tiny_rolling", "tiny_handeye"])
@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: "-".join(k for k, v in f.items() if v) or "none")
@pytest.mark.parametrize("invalid_first", [False, True])
def test_default_hold_is_the_first_valid_camera_and_board(name, flags, invalid_first):
  c = _calib(name)
  if invalid_first:
    c = c.copy(camera_poses=_invalidate_first(c.camera_poses), board_poses=_invalidate_first(c.board_poses))
  c = c.copy(optimize=c.optimize._extend(boards=False, **flags))
  hold = gauge.default_hold(c)
  assert hold.dtype == bool and hold.shape == c.param_vec.shape
  expect = np.zeros_like(hold)
  off = _offsets(c)
  first_c = 1 if invalid_first else 0
  first_b = 1 if invalid_first and c.size.boards > 1 else 0
  if invalid_first and c.size.boards == 1:
    first_b = 0          # no valid board at all: the (unobserved) first board, as gauge.canonical
  if "camera_poses" in off:
    expect[off["camera_poses"][0] + 6 * first_c:off["camera_poses"][0] + 6 * first_c + 6] = True
  if "board_poses" in off:
    expect[off["board_poses"][0] + 6 * first_b:off["board_poses"][0] + 6 * first_b + 6] = True
  np.testing.assert_array_equal(hold, expect)


@pytest.mark.parametrize("name", ["tiny", "tiny_rolling", "tiny_handeye"])
def test_default_hold_refuses_the_boards_block(name):
  c = _calib(name).enable(boards=True)
  with pytest.raises(ValueError, match="explicit hold"):
    gauge.default_hold(c)


def test_covariance_needs_a_hold_when_boards_are_adjusted():
  # the ValueError comes before any device work
  c = _calib("tiny").enable(boards=True)
  with pytest.raises(ValueError, match="explicit hold"):
    c.covariance()
  with pytest.raises(ValueError, match="explicit hold"):
    c.parameter_std()


@pytest.mark.parametrize("name", ["tiny", "tiny_rolling", "tiny_handeye", "tiny_fishmix", "tiny_mixed", "tiny_fixintr_like"])
def test_split_std_names_every_block(name):
  c = _calib("tiny" if name == "tiny_fixintr_like" else name)
  if name == "tiny_fixintr_like":
    c = c.enable(cameras=False)
  c = c.enable(boards=True)
  std = np.arange(c.param_vec.size, dtype=np.float64)
  s = calibration.split_std(c, std)
  off = _offsets(c)
  assert set(s.keys()) == set(off.keys())
  C, F, B = c.size.cameras, c.size.rig_poses, c.size.boards
  flat = []
  if "camera_poses" in s:
    assert s["camera_poses"].shape == (C, 6)
    flat.append(s["camera_poses"].ravel())
  assert s["board_poses"].shape == (B, 6)
  flat.append(s["board_poses"].ravel())
  m = s["motion"]
  if name in ("tiny_rolling", "tiny_fishmix"):
    assert [a.shape for a in m] == [(F, 6), (F, 6)]
    flat += [a.ravel() for a in m]
  elif name == "tiny_handeye":
    assert m["world_wrt_base"].shape == (6,) and m["gripper_wrt_camera"].shape == (6,)
    flat += [m["world_wrt_base"], m["gripper_wrt_camera"]]
  else:
    assert m.shape == (F, 6)
    flat.append(m.ravel())
  if "cameras" in s:
    assert [a.size for a in s["cameras"]] == [np.asarray(cam.param_vec).size for cam in c.cameras]
    flat += list(s["cameras"])
  assert [a.shape for a in s["boards"]] == [(b.num_points, 3) for b in c.boards]
  flat += [a.ravel() for a in s["boards"]]
  np.testing.assert_array_equal(np.concatenate(flat), std)


def test_ragged_cameras_split_into_their_own_sizes():
  c = _calib("tiny_mixed")
  sizes = [np.asarray(cam.param_vec).size for cam in c.cameras]
  assert len(set(sizes)) > 1
  s = calibration.split_std(c, np.arange(c.param_vec.size, dtype=np.float64))
  assert [a.size for a in s["cameras"]] == sizes


def test_covariance_entry_points_are_declared():
  names = {name for name, _, _ in _lib.SYMBOLS}
  assert {"mcba_covariance", "mcba_covariance_layout"} <= names
  import os
  header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "mcba.h")).read()
  assert "int32_t mcba_covariance(" in header and "int32_t mcba_covariance_layout(" in header
