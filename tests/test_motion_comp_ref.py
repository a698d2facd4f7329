"""The numpy restatement of the front end's motion compensation (tests/motion_comp_ref.py) against independent statements of
the same mathematics: exact end points, scipy's Slerp, the two branches of Eigen's slerp, and AverageTransforms by hand."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_comp_ref as mc  # noqa: E402


def _cloud(n, seed, reach=100.0):
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 5), np.float32)
    rows[:, :3] = rng.uniform(-reach / np.sqrt(3.0), reach / np.sqrt(3.0), (n, 3))      # within `reach` metres
    rows[:, 3] = rng.uniform(0, 255, n)
    rows[:, 4] = rng.uniform(0, 1, n)
    return rows


@pytest.mark.parametrize("name", ["drive", "half_turn", "tiny", "identity"])
def test_factor_zero_rows_come_back_bit_for_bit(name):
    rows = _cloud(2000, 1)
    rows[:, 4] = 0.0
    out = mc.motion_compensation(rows, mc.check_deltas()[name])
    assert out.tobytes() == rows.tobytes()


@pytest.mark.parametrize("name", ["drive", "half_turn", "tiny", "identity"])
def test_factor_one_rows_equal_delta_applied_in_double(name):
    delta = mc.check_deltas()[name]
    rows = _cloud(2000, 2)
    rows[:, 4] = 1.0
    got = mc.motion_compensation_f64(rows, delta)
    want = rows[:, :3].astype(np.float64) @ delta[:3, :3].T + delta[:3, 3]
    err = np.abs(got - want).max()
    print(name, "factor 1 against delta in double: %.3g m" % err)
    assert err <= 1e-12


@pytest.mark.parametrize("name", ["drive", "half_turn", "tiny", "identity"])
def test_rotation_agrees_with_scipy_slerp(name):
    from scipy.spatial.transform import Rotation, Slerp
    delta = mc.check_deltas()[name]
    rows = _cloud(5000, 3)
    f = rows[:, 4].astype(np.float64)
    key = Rotation.from_matrix(np.stack([np.eye(3), delta[:3, :3]]))
    want = Slerp([0.0, 1.0], key)(f).apply(rows[:, :3].astype(np.float64)) + np.outer(f, delta[:3, 3])
    got = mc.motion_compensation_f64(rows, delta)
    err = np.abs(got - want).max()
    print(name, "against scipy Slerp: %.3g m" % err)
    assert err <= 1e-12


def test_linear_branch_for_a_tiny_rotation():
    delta = mc.check_deltas()["tiny"]
    plan = mc.slerp_plan(delta)
    assert plan["linear"] and plan["d"] >= 1.0 - mc.DBL_EPSILON
    s0, s1 = mc.slerp_scales(plan, np.array([0.0, 0.25, 1.0]))
    assert np.array_equal(s0, [1.0, 0.75, 0.0]) and np.array_equal(s1, [0.0, 0.25, 1.0])
    # the interpolated quaternion is not normalised: at f = 0.5 it is (1, 0, 0, 2.5e-10), and the matrix is Eigen's formula of it
    R = mc.interpolated_rotations(delta, [0.5])[0]
    assert R[1, 0] == 2.0 * (0.5 * plan["qb"][3]) * 1.0 and R[0, 1] == -R[1, 0]
    assert not mc.slerp_plan(mc.check_deltas()["drive"])["linear"]


def test_negative_dot_branch():
    delta = mc.check_deltas()["half_turn"]
    R = delta[:3, :3]
    assert R[0, 0] + R[1, 1] + R[2, 2] <= 0 and R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]      # the largest-diagonal branch, i = 0
    plan = mc.slerp_plan(delta)
    assert plan["qb"][0] < 0 and plan["d"] < 0 and not plan["linear"]
    s0, s1 = mc.slerp_scales(plan, np.array([0.5]))
    assert s0[0] > 0 and s1[0] < 0                                                            # the second scale is negated
    # q_b and -q_b are the same rotation; negating the scale walks the short way: half the factor, half the angle
    half = mc.interpolated_rotations(delta, [0.5])[0]
    assert np.abs(half - mc.rotation_about((-1.0, 0.0, 0.0), 1.55)).max() < 1e-15
    # Eigen's branch, restated independently for i = 0: x = sqrt(m00 - m11 - m22 + 1) / 2, w = (m21 - m12) / (4 x)
    x = 0.5 * np.sqrt(R[0, 0] - R[1, 1] - R[2, 2] + 1.0)
    assert plan["qb"][1] == x and abs(plan["qb"][0] - (R[2, 1] - R[1, 2]) / (4.0 * x)) < 1e-16


def test_factor_outside_the_unit_interval_is_refused():
    rows = _cloud(10, 4)
    for bad in (-1e-6, 1.0 + 1e-6, np.nan):
        r = rows.copy()
        r[3, 4] = bad
        with pytest.raises(ValueError):
            mc.motion_compensation(r, np.eye(4))


def test_intensity_and_factor_are_carried():
    rows = _cloud(1000, 5)
    out = mc.motion_compensation(rows, mc.check_deltas()["drive"])
    assert out[:, 3:].tobytes() == rows[:, 3:].tobytes() and out.dtype == np.float32


def test_average_transforms_by_hand():
    # two rotations about z by 0.2 and 0.4 rad: Euler angles (0, 0, 0.2) and (0, 0, 0.4), mean (0, 0, 0.3);
    # translations (1, 2, 3) and (3, 4, 6): mean (2, 3, 4.5)
    def Tz(a, t):
        M = np.eye(4)
        M[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
        M[:3, 3] = t
        return M
    got = mc.average_transforms([Tz(0.2, (1, 2, 3)), Tz(0.4, (3, 4, 6))])
    want = Tz(0.3, (2, 3, 4.5))
    assert np.abs(got - want).max() < 1e-15
    # Euler angles are averaged, not rotations: Rx(0.2) and Ry(0.4) give the angles (0.1, 0.2, 0) -> Rz(0) Ry(0.2) Rx(0.1)
    Rx = np.eye(4); Rx[:3, :3] = mc.rotation_about((1, 0, 0), 0.2)
    Ry = np.eye(4); Ry[:3, :3] = mc.rotation_about((0, 1, 0), 0.4)
    got = mc.average_transforms([Rx, Ry])
    want = mc.rotation_about((0, 1, 0), 0.2) @ mc.rotation_about((1, 0, 0), 0.1)
    assert np.abs(got[:3, :3] - want).max() < 1e-15 and np.all(got[:3, 3] == 0)
    one = Tz(0.7, (1, -2, 3))
    assert np.abs(mc.average_transforms([one]) - one).max() < 1e-15


def test_interpolate_transform_is_the_per_row_transform():
    delta = mc.check_deltas()["drive"]
    rows = _cloud(50, 6)
    out = mc.motion_compensation_f64(rows, delta)
    for i in (0, 7, 49):
        T = mc.interpolate_transform(delta, rows[i, 4])
        p = T[:3, :3] @ rows[i, :3].astype(np.float64) + T[:3, 3]
        assert np.abs(p - out[i]).max() < 1e-13
