"""tests/map_package_ref.py, the restatement of the reference's SaveTrajectoriesAsMapPackage, checked against figures worked out by
hand from builder/map_package.cc -- so that what the device is compared with is itself pinned.  No GPU, no library."""
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import map_package_cases as cases
import map_package_ref as ref


def test_one_submap_gives_one_piece_that_holds_the_whole_map():
    pl = ref.plan([(3.0, 4.0, 1.0)])                      # extent 200 x 200, half width 250: 0 steps -> 1
    assert (pl["x_steps"], pl["y_steps"]) == (1, 1)
    p = pl["pieces"][0]
    assert p["centre"] == (-97.0 + 250.0, -96.0 + 250.0)
    assert p["bb_min"] == (-97.0, -96.0) and p["bb_max"] == (103.0, 104.0)       # centre + 250 clamped to the extent
    assert p["members"] == [0]


def test_line_without_border_truncation_and_closed_membership():
    t, b, w = cases.plan_cases()["line_exact_multiple"]
    pl = ref.plan(t, b, w)
    assert (pl["x_steps"], pl["y_steps"]) == (5, 1)       # 40 / 8 = 5 exactly; y extent 0 -> 0 -> 1
    assert [p["centre"][0] for p in pl["pieces"]] == [8.0, 16.0, 24.0, 32.0, 40.0]
    assert all(p["bb_min"][1] == 5.0 and p["bb_max"][1] == 5.0 for p in pl["pieces"])
    assert pl["pieces"][0]["members"] == [0, 1] and pl["pieces"][1]["members"] == [1, 2]     # box [0, 16]: x = 0 and x = 10; [8, 24]: 10, 20
    assert pl["pieces"][4]["bb_max"][0] == 40.0           # 48 clamped
    t, b, w = cases.plan_cases()["line_just_short"]
    assert ref.plan(t, b, w)["x_steps"] == 4
    t, b, w = cases.plan_cases()["on_the_widened_bound"]
    pl = ref.plan(t, b, w)
    assert pl["pieces"][1]["bb_min"] == (2.0, -2.0) and pl["pieces"][1]["bb_max"] == (10.0, 2.0)
    assert pl["pieces"][1]["members"] == [0, 1]           # x = 0 = 2 - 2 and x = 12 = 10 + 2: on the bounds, kept


def test_pieces_overlap_by_half_and_outer_ones_are_clamped():
    t, b, w = cases.plan_cases()["clamped_outer_pieces"]
    pl = ref.plan(t, b, w)
    ys = pl["y_steps"]
    for p in pl["pieces"]:
        if p["x"] + 1 < pl["x_steps"]:
            q = pl["pieces"][(p["x"] + 1) * ys + p["y"]]
            assert q["centre"][0] - p["centre"][0] == w / 2
    last = pl["pieces"][-1]
    assert last["bb_max"][0] - last["centre"][0] < w / 2 and last["bb_max"] == (23.0, 15.0)
    assert any(len(p["members"]) == 0 for p in pl["pieces"]) and any(len(p["members"]) > 1 for p in pl["pieces"])


def test_the_reference_refuses_only_a_negative_step_count():
    for name, (t, b, w, by_reference) in cases.refused_cases().items():
        if by_reference:
            with pytest.raises(ref.Refused):
                ref.plan(t, b, w)
    t, b, w = cases.plan_cases()["slightly_inverted"]
    pl = ref.plan(t, b, w)                                # extent -2: int(-0.5) = 0 -> 1 piece, bounds clamped into an inverted interval
    assert (pl["x_steps"], pl["y_steps"]) == (1, 1) and pl["pieces"][0]["members"] == []


def test_clip_is_closed_in_double_and_a_nan_is_outside():
    rows = np.array([[1.0, 0.0, 0, 0], [2.0, 0.0, 0, 0], [np.float32(2.0000002), 0, 0, 0], [0.99999994, 0, 0, 0], [np.nan, 0, 0, 0], [1.5, np.inf, 0, 0],
                     [1.5, 0.5, np.nan, 0]], np.float32)
    assert ref.rows_in_box(rows, (1.0, -1.0), (2.0, 1.0)).tolist() == [True, True, False, False, False, False, True]
    out = ref.cut(rows, (1.0, -1.0), (2.0, 1.0), (0.1, -0.3))
    assert len(out) == 3 and out.dtype == np.float32
    assert out[0, 0] == np.float32(1.0 - 0.1) and out[0, 1] == np.float32(0.0 + 0.3)     # in double, rounded once


def test_a_member_outside_the_box_is_clipped_and_one_with_no_row_left_makes_no_insert():
    class Log:
        def __init__(self):
            self.calls = []

        def insert(self, rows, origin):
            self.calls.append((rows.copy(), origin.copy()))
    piece = dict(bb_min=(0.0, 0.0), bb_max=(4.0, 4.0), members=[0, 1, 2, 3])
    cloud = np.array([[0, 0, 0, 7, 0.5], [1, 1, 1, 8, 0.25], [3, 3, 0, 9, 0.75]], np.float32)
    P = lambda x, y: np.array([[1, 0, 0, x], [0, 1, 0, y], [0, 0, 1, 2.5], [0, 0, 0, 1.0]])
    submaps = [(P(1, 1), cloud), (P(-2, 0), cloud), (P(50, 50), cloud), (P(2, 2), np.zeros((0, 5), np.float32))]
    log = Log()
    assert ref.fill_piece(log, submaps, piece) == (1, 1, 2)
    assert len(log.calls) == 2
    assert np.array_equal(log.calls[0][0][:, :2], cloud[:, :2] + 1) and np.array_equal(log.calls[0][1], np.float32([1, 1, 2.5]))   # whole
    assert np.array_equal(log.calls[1][0], np.float32([[1, 3, 2.5, 9, 0.75]])) and np.array_equal(log.calls[1][1], np.float32([-2, 0, 2.5]))


def test_xml_parses_back_to_the_plan():
    t, b, w = cases.plan_cases()["walk"]
    pl = ref.plan(t, b, w)
    text = ref.xml_text(pl, "part_")
    assert text.startswith('<?xml version="1.0"?>\n<MapPackage>\n\t<Piece x="') and text.endswith(' />\n</MapPackage>\n')
    root = ET.fromstring(text)
    assert root.tag == "MapPackage" and len(root) == len(pl["pieces"]) > 4
    for e, p in zip(root, pl["pieces"]):
        assert e.tag == "Piece" and list(e.attrib) == ["x", "y", "file"]
        assert (float(e.get("x")), float(e.get("y"))) == p["centre"]             # %.17g gives the double back
        assert e.get("file") == "part_%d_%d.pcd" % (p["x"], p["y"])


def test_the_drivers_pose_arithmetic_restated():
    rng = np.random.default_rng(3)
    a = rng.normal(size=3); a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    P = np.eye(4); P[:3, :3] = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K; P[:3, 3] = [5, -3, 1]
    assert np.allclose(ref.affine_inverse(P) @ P, np.eye(4), atol=1e-14)
    assert np.allclose(ref.mul_pose(P, P), P @ P, atol=1e-14)
    lp = ref.submap_local_poses([P, P @ P])
    assert np.array_equal(lp[0], np.eye(4)) and np.allclose(lp[1], P, atol=1e-13)
