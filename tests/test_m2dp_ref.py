"""Self-tests of the restatement of descriptor::M2dp (tests/m2dp_ref.py) -- no GPU."""
import numpy as np

import m2dp_ref as mr
from staticmapping_amd import synth


def test_hand_computed_view():
    """p_ = 2, q_ = 1: view 1 has theta = pi/2, so m = (6e-17, 0, 1), projected_x_axis = (1, -0, -6e-17) and projected_y_axis =
    (0, 1, 0): the view's coordinates are (|x|, |y|) for coordinates of ordinary size.  r = 0.1, t = 16: angle_step = pi/8, l = 32."""
    o = mr.options(p=2, q=1)
    m, px, py = mr.view_axes(o)
    assert np.allclose(m[1], [0, 0, 1], atol=1e-7) and np.allclose(px[1], [1, 0, 0], atol=1e-7) and np.array_equal(py[1], [0, 1, 0])
    assert np.array_equal(m[0], [1, 0, 0]) and np.array_equal(px[0], [0, 0, 0]) and np.array_equal(py[0], [0, 0, 0])
    pts = np.array([[3, 4, 7],            # length 5: floor(sqrt(50)) = 7; atan2(4, 3) = 0.927 = 2.36 steps -> cell 7 * 16 + 2
                    [-1, 0, 2],           # length 1: floor(sqrt(10)) = 3; angle 0 -> cell 48
                    [0, -2, 1],           # length 2: floor(sqrt(20)) = 4; angle pi/2 = 4 steps (the last reachable bin) -> cell 68
                    [200, 0, 0]],         # length 200: sqrt(2000) = 44.7, clamped to 31; angle 0 -> cell 496
                   np.float32)
    s = mr.samples(pts, o)
    assert list(s["l_index"][:, 1]) == [7, 3, 4, 31] and list(s["t_index"][:, 1]) == [2, 0, 4, 0]
    assert (s["l_index"][:, 0] == 0).all() and (s["t_index"][:, 0] == 0).all() and (s["length"][:, 0] == 0).all()
    assert not s["flagged"][:, 0].any()                         # length 0 is never flagged
    A = mr.histogram_of(s, o)
    want = np.zeros((2, 32 * 16), np.int64)
    want[0, 0] = 4
    want[1, [114, 48, 68, 496]] = 1
    assert np.array_equal(A, want)
    assert s["t_index"].max() <= o["t"] // 4


def test_hand_computed_cloud():
    """(+-3, 0, 0), (0, +-1, 0): mean 0, covariance diag(6, 2/3, 0), so the axes are e1, e2, e3 and the rows project onto themselves"""
    o = mr.options(p=2, q=1)
    cloud = np.array([[3, 0, 0, 0.5], [-3, 0, 0, 0.5], [0, 1, 0, 0.5], [0, -1, 0, 0.5]], np.float32)
    r = mr.m2dp(cloud, o)
    assert np.allclose(r["eigenvalues"], [6, 2 / 3, 0], atol=1e-14)
    assert np.array_equal(r["projected3"], cloud[:, :3]) and r["kept"].all()
    want = np.zeros((2, 512), np.int64)
    want[0, 0] = 4
    want[1, 5 * 16 + 0] = 2                                     # length 3: floor(sqrt(30)) = 5, angle 0
    want[1, 3 * 16 + 4] = 2                                     # length 1: floor(sqrt(10)) = 3, angle pi/2
    assert np.array_equal(r["A"], want)
    assert len(r["descriptor"]) == mr.length(o) == 2 + 512 and r["descriptor"][:2].sum() >= 0
    far = mr.m2dp(cloud, mr.options(p=2, q=1, max_distance=2.0))  # getLength 3 > 2: the two far rows are dropped
    assert list(far["kept"]) == [False, False, True, True] and far["A"].sum() == 4 and mr.ring_count(mr.options(max_distance=2.0)) == 5


def test_rows_sum_to_kept_and_scores():
    a, b, _ = synth.scan_pair("cfg2", 4000)
    o = mr.options(max_distance=30.0)
    ra, rb = mr.m2dp(a, o), mr.m2dp(b, o)
    assert 0 < ra["kept"].sum() < len(a)
    assert (ra["A"].sum(axis=1) == ra["kept"].sum()).all() and ra["A"].shape == (64, mr.ring_count(o) * 16)
    assert ra["samples"]["t_index"].max() <= 4                   # both coordinates are absolute values: never above pi/2
    d, e = ra["descriptor"], rb["descriptor"]
    assert d.dtype == np.float32 and abs(np.linalg.norm(d[:64]) - 1) < 1e-6 and abs(np.linalg.norm(d[64:]) - 1) < 1e-6
    assert abs(mr.match(d, d) - 1.0) < 1e-12
    s = mr.match(d, e)
    assert 0.9 < s < 1.0
    assert mr.match(-d, e) == s and mr.match(d, -e) == s         # the score's absolute value (m2dp.cc:168)
    assert mr.match(d, e[:-1]) == -1.0 and mr.match(d[:9], e[:9]) == -1.0
    import pytest
    with pytest.raises(ValueError):
        mr.m2dp(a, mr.options(r=1e-7))
    with pytest.raises(ValueError):
        mr.m2dp(a[:0])


def test_rotated_and_shifted_copy_gives_the_same_histogram():
    """The copy is exact: the cloud lies on the lattice of multiples of 5/256, the rotation is the rational (4/5, 3/5) one
    about z and the shift a multiple of 1/256, so both clouds are float rows related exactly and only the f64 moments round
    differently.  The cloud's axes (-20 and 70 degrees in the xy plane) keep their dominant components' signs under the
    rotation (17 and 107 degrees), as the sign rule needs; eigenvalues 21 : 3 : 0.2."""
    rng = np.random.default_rng(4)
    local = rng.uniform(-1, 1, (3000, 3)) * np.array([8.0, 3.0, 0.8])
    c, s = np.cos(np.deg2rad(-20)), np.sin(np.deg2rad(-20))
    a = local @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]).T
    a = np.round(a * 256 / 5) * 5 / 256
    R = np.array([[0.8, -0.6, 0], [0.6, 0.8, 0], [0, 0, 1]])
    b = (np.stack([(4 * a[:, 0] - 3 * a[:, 1]) / 5, (3 * a[:, 0] + 4 * a[:, 1]) / 5, a[:, 2]], axis=1)) + np.array([64.0, -32.0, 16.0]) + 3 / 256
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a) and np.array_equal(b.astype(np.float32).astype(np.float64), b)
    assert np.allclose(b - np.array([64.0, -32.0, 16.0]) - 3 / 256, a @ R.T, atol=1e-12)
    o = mr.options(max_distance=7.0)                             # some rows are dropped, too
    ra, rb = mr.m2dp(a.astype(np.float32), o), mr.m2dp(b.astype(np.float32), o)
    w = ra["eigenvalues"]
    assert (w[0] - w[1]) / w[0] > 0.1 and (w[1] - w[2]) / w[1] > 0.1
    assert 0 < ra["kept"].sum() < len(a)
    assert np.abs(ra["projected3"].astype(np.float64) - rb["projected3"].astype(np.float64)).max() <= 1e-6
    s_a = ra["samples"]
    lo = mr.histogram_of(s_a, o, ~s_a["flagged"])
    F = mr.flagged_spread(s_a, o)
    assert s_a["flagged"].mean() < 1e-3
    assert (rb["A"] >= lo).all() and (rb["A"] <= lo + F).all()
    assert np.abs(rb["A"] - ra["A"]).sum() <= 2 * s_a["flagged"].sum()
    assert mr.match(ra["descriptor"], rb["descriptor"]) > 0.99999


def test_moved_histogram_moves_only_flagged_samples():
    a = synth.scan_pair("cfg2", 4000)[0]
    o = mr.options()
    r = mr.m2dp(a, o)
    s = r["samples"]
    moved = mr.moved_histogram(s, o)
    assert (moved.sum(axis=1) == r["A"].sum(axis=1)).all()
    assert 0 < np.abs(moved - r["A"]).sum() <= 2 * s["flagged"].sum()
    lo = mr.histogram_of(s, o, ~s["flagged"])
    assert (moved >= lo).all() and (moved <= lo + mr.flagged_spread(s, o)).all()
