"""The map package's host half through the C ABI and the Python module, without a GPU: smhip_map_package_plan against the restatement
(tests/map_package_ref.py) -- centres, boxes, step counts and member lists exactly -- its refusals, and the description file."""
import ctypes
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import map_package_cases as cases
import map_package_ref as ref


def _mp():
    from staticmapping_amd import build
    build.build()
    from staticmapping_amd import map_package
    return map_package


def _assert_plan_equals(got, want):
    assert (got.x_steps, got.y_steps) == (want["x_steps"], want["y_steps"])
    assert len(got.centres) == len(want["pieces"])
    assert np.array_equal(got.centres, np.array([p["centre"] for p in want["pieces"]]))          # the same doubles, not close ones
    assert np.array_equal(got.bb_min, np.array([p["bb_min"] for p in want["pieces"]]))
    assert np.array_equal(got.bb_max, np.array([p["bb_max"] for p in want["pieces"]]))
    assert [m.tolist() for m in got.members] == [p["members"] for p in want["pieces"]]


@pytest.mark.parametrize("name", sorted(cases.plan_cases()))
def test_plan_equals_the_restatement(name):
    mp = _mp()
    t, border, width = cases.plan_cases()[name]
    got = mp.plan(t, mp.MapPackageOptions(border_offset=border, piece_width=width))
    _assert_plan_equals(got, ref.plan(t, border, width))


def test_defaults_are_the_references():
    mp = _mp()
    from staticmapping_amd import _capi
    o = _capi.MapPackageOptions()
    _capi.load_library().smhip_map_package_default_options(ctypes.byref(o))
    assert (o.border_offset, o.piece_width) == (ref.DEFAULTS["border_offset"], ref.DEFAULTS["piece_width"])
    d = mp.MapPackageOptions()
    assert (d.border_offset, d.piece_width, d.cloud_file_prefix, d.descript_filename) == (100.0, 500.0, "part_", "map_package.xml")
    t = cases.plan_cases()["one_submap"][0]
    _assert_plan_equals(mp.plan(t), ref.plan(t))


@pytest.mark.parametrize("name", sorted(cases.refused_cases()))
def test_refusals_say_why(name):
    mp = _mp()
    import staticmapping_amd as sm
    t, border, width, by_reference = cases.refused_cases()[name]
    with pytest.raises(sm.SmhipError) as e:
        mp.plan(t, mp.MapPackageOptions(border_offset=border, piece_width=width))
    assert e.value.status == 1 and len(str(e.value)) > len("smhip status 1: ") + 5  # SMHIP_ERR_INVALID_ARGUMENT and a reason
    if by_reference:
        with pytest.raises(ref.Refused):
            ref.plan(t, border, width)
        assert "No good bounding box" in str(e.value)


def test_the_counting_call_and_null_outputs():
    _mp()
    from staticmapping_amd import _capi
    lib = _capi.load_library()
    t, border, width = cases.plan_cases()["clamped_outer_pieces"]
    want = ref.plan(t, border, width)
    o = _capi.MapPackageOptions()
    lib.smhip_map_package_default_options(ctypes.byref(o))
    o.border_offset, o.piece_width = border, width
    t = np.ascontiguousarray(t)
    steps = np.zeros(2, np.int32)
    n = ctypes.c_int32(-1)
    guard = np.full(4, 7.0)
    st = lib.smhip_map_package_plan(len(t), t.ctypes.data_as(_capi.c_double_p), ctypes.byref(o), steps.ctypes.data_as(_capi.c_int32_p), 1,
                                    guard.ctypes.data_as(_capi.c_double_p), None, None, 0, None, ctypes.byref(n), None, 0)
    assert st == 0 and tuple(steps) == (want["x_steps"], want["y_steps"]) and n.value == sum(len(p["members"]) for p in want["pieces"])
    assert (guard == 7.0).all()                                                   # capacity 1 < pieces: only counted
    st = lib.smhip_map_package_plan(len(t), t.ctypes.data_as(_capi.c_double_p), None, steps.ctypes.data_as(_capi.c_int32_p), 0, None, None, None, 0, None,
                                    None, None, 0)
    assert st == 1


def test_description_file(tmp_path):
    mp = _mp()
    t, border, width = cases.plan_cases()["walk"]
    o = mp.MapPackageOptions(border_offset=border, piece_width=width, cloud_file_prefix="p&<\"_")
    pl = mp.plan(t, o)
    want = ref.plan(t, border, width)
    a, b = tmp_path / "a.xml", tmp_path / "b.xml"
    mp.write_xml(str(a), pl, o)
    mp.write_xml(str(b), pl, o)
    assert a.read_bytes() == b.read_bytes()                                       # byte-identical on a second write
    root = ET.parse(str(a)).getroot()
    assert root.tag == "MapPackage" and len(root) == len(want["pieces"])
    for e, p in zip(root, want["pieces"]):
        assert (float(e.get("x")), float(e.get("y"))) == p["centre"]
        assert e.get("file") == 'p&<"_%d_%d.pcd' % (p["x"], p["y"])
    # with the default prefix the text is the restatement's, byte for byte
    assert mp.xml_text(pl, mp.MapPackageOptions(border_offset=border, piece_width=width)) == ref.xml_text(want, "part_")
    # a missing directory: the write fails and leaves nothing
    with pytest.raises(OSError):
        mp.write_xml(str(tmp_path / "missing" / "map_package.xml"), pl, o)
    assert sorted(os.listdir(tmp_path)) == ["a.xml", "b.xml"]


def test_package_into_a_missing_directory_fails_before_any_device_work(tmp_path):
    """(no GPU needed: the description's place is taken first)"""
    mp = _mp()
    sub = [(np.eye(4), np.zeros((3, 5), np.float32))]
    with pytest.raises(OSError):
        mp.save_map_package(sub, str(tmp_path / "missing") + os.sep)
    assert os.listdir(tmp_path) == []
    import staticmapping_amd as sm
    with pytest.raises(sm.SmhipError):                                            # a refused plan: nothing written either
        mp.save_map_package(sub, str(tmp_path) + os.sep, mp.MapPackageOptions(piece_width=0.0))
    assert os.listdir(tmp_path) == []
