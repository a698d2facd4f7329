"""smhip_filter_output_to_source_compensated -- the front end's MotionCompensation (builder/map_builder.cc:232-257) of the
filter workspace's cloud into a source slot, on the device -- against the numpy restatement (tests/motion_comp_ref.py).

Rule of the comparisons: every float coordinate within 1 ulp, at most 1e-4 of them different at all (the device's double sin is
another correctly implemented sin than numpy's: a few double ulps, ~1e-13 m, which changes the float only when the double lies
that close to a rounding boundary, and then by exactly 1 ulp; the cap keeps a wrong formula from hiding behind "1 ulp")."""
import ctypes
import os
import sys

import numpy as np
import pytest

import staticmapping_amd as sm
from staticmapping_amd import _capi, filters as df, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_comp_ref as mc  # noqa: E402
from driver_ref import ROT_TOL, TRANS_TOL, SCORE_TOL  # noqa: E402

pytestmark = pytest.mark.gpu

OK, INVALID, NOT_READY, CAPACITY = 0, 1, 4, 7
DELTAS = ["drive", "half_turn", "tiny", "identity"]
KEEP = df.make_filter("AxisRange", min=-500.0, max=500.0, axis_index=2)          # drops the rows parked at z = 1000


@pytest.fixture(scope="module")
def matcher():
    m = sm.IcpFastHip(pair_slots=2, max_source_points=196608, max_target_points=196608)
    yield m
    m.close()


def raw_cloud(n_kept, seed):
    """KITTI rows of which exactly n_kept survive KEEP; every third row is parked outside, so the survivors' factors
    (i / N of the raw cloud, data_collector.h:202-204) are not i / n_kept"""
    rng = np.random.default_rng(seed)
    total = n_kept + n_kept // 2 + 1
    rows = np.zeros((total, 4), np.float32)
    rows[:, :3] = rng.uniform(-80.0, 80.0, (total, 3))
    rows[:, 3] = rng.uniform(0.0, 255.0, total)
    drop = np.ones(total, bool)
    drop[rng.choice(total, n_kept, replace=False)] = False
    rows[drop, 2] = 1000.0
    return rows


def filtered(matcher, n_kept, seed):
    rows, _ = df.run_chain(matcher, raw_cloud(n_kept, seed), [KEEP])
    assert rows.shape == (n_kept, 5)
    if n_kept > 10:
        assert not np.array_equal(rows[:, 4], (np.arange(n_kept) / n_kept).astype(np.float32))
    return rows


def workspace_rows(matcher, n):
    out = np.zeros((n, 5), np.float32)
    matcher._check(matcher._lib.smhip_filter_get_output(matcher._h, out.ctypes.data_as(_capi.c_float_p), None, n))
    return out


def source_in_caller_order(matcher, slot=0):
    p, idx = matcher.get_source(slot)
    assert sorted(idx.tolist()) == list(range(len(p)))                           # .w: a permutation of the workspace's rows
    out = np.empty_like(p)
    out[idx] = p
    return out


@pytest.mark.parametrize("n", [1, 255, 256, 257, 120_000])
@pytest.mark.parametrize("name", DELTAS)
def test_compensated_rows_match_the_restatement(matcher, n, name):
    rows = filtered(matcher, n, seed=n)
    delta = mc.check_deltas()[name]
    want = mc.motion_compensation(rows, delta)
    before = workspace_rows(matcher, n)
    got = df.output_to_source_compensated(matcher, delta, slot=0, download=True)
    assert got.shape == (n, 5) and got.dtype == np.float32
    assert got[:, 3:].tobytes() == rows[:, 3:].tobytes()                        # intensity and factor: bitwise the input's
    mc.assert_one_ulp(got[:, :3], want[:, :3], "points5_out, n = %d, %s" % (n, name))
    src = source_in_caller_order(matcher)
    assert src.tobytes() == got[:, :3].tobytes()                                 # the slot holds the rows that were handed back
    mc.assert_one_ulp(src, want[:, :3], "resident source, n = %d, %s" % (n, name))
    assert workspace_rows(matcher, n).tobytes() == before.tobytes() == rows.tobytes()   # the workspace is left as it was


def test_two_deltas_give_each_delta_its_own_result(matcher):
    n = 50_000
    rows = filtered(matcher, n, seed=7)
    d = mc.check_deltas()
    first = df.output_to_source_compensated(matcher, d["drive"], download=True)
    second = df.output_to_source_compensated(matcher, d["half_turn"], slot=1, download=True)
    again = df.output_to_source_compensated(matcher, d["drive"], download=True)
    mc.assert_one_ulp(first[:, :3], mc.motion_compensation(rows, d["drive"])[:, :3], "first delta")
    mc.assert_one_ulp(second[:, :3], mc.motion_compensation(rows, d["half_turn"])[:, :3], "second delta")
    assert again.tobytes() == first.tobytes()
    assert np.abs(first[:, :3] - second[:, :3]).max() > 1.0
    assert source_in_caller_order(matcher, 1).tobytes() == second[:, :3].tobytes()
    assert source_in_caller_order(matcher, 0).tobytes() == first[:, :3].tobytes()
    assert df.output_to_source_compensated(matcher, d["tiny"]) is None           # no download asked for


def test_align_on_the_compensated_source_equals_an_upload_of_the_restatement(matcher):
    scene = synth.make_scene(0)
    target = synth.velodyne_scan(scene, synth.make_pose(), seed=120, n_points=30_000)
    source = synth.velodyne_scan(scene, synth.make_pose(t=(0.3, 0.01, 0.0), rpy_deg=(0, 0, 0.4)), seed=121, n_points=30_000)
    delta = mc.check_deltas()["drive"]
    guess = synth.make_pose(t=(0.25, 0.0, 0.0))
    matcher.set_options(max_iteration=100, dist_outlier_ratio=0.7, early_exit=1)
    assert matcher.prepare_target(target) > 1000
    rows, _ = df.run_chain(matcher, source, [df.make_filter("Range", min_range=5.0, max_range=40.0)])
    assert 1000 < len(rows) < len(source)
    df.output_to_source_compensated(matcher, delta)
    ok_a, res_a = matcher.align(guess)
    score_a = matcher.get_fitness_score()
    matcher.set_input_source(mc.motion_compensation(rows, delta))
    ok_b, res_b = matcher.align(guess)
    score_b = matcher.get_fitness_score()
    da, dt = sm.se3_error(res_a, res_b)
    print("align on the device-compensated source against the uploaded restatement: %.3g rad, %.3g m, score %.9g / %.9g" % (da, dt, score_a, score_b))
    assert ok_a and ok_b and da <= ROT_TOL and dt <= TRANS_TOL and abs(score_a - score_b) <= SCORE_TOL


def _call(m, slot, delta, out=None):
    d = np.ascontiguousarray(np.asarray(delta, np.float64).T)
    st = m._lib.smhip_filter_output_to_source_compensated(m._h, slot, d.ctypes.data_as(_capi.c_double_p),
                                                          None if out is None else out.ctypes.data_as(_capi.c_float_p))
    return st, m._lib.smhip_last_error(m._h).decode()


def _source_size(m, slot=0):
    ns = ctypes.c_int32(-1)
    m._check(m._lib.smhip_get_cloud_sizes(m._h, slot, ctypes.byref(ns), None, None))
    return ns.value


def test_refusals_before_anything_is_touched():
    m = sm.IcpFastHip(pair_slots=1, max_source_points=4096, max_target_points=16384)
    try:
        st, msg = _call(m, 0, np.eye(4))
        assert st == NOT_READY and msg                                          # no cloud in the workspace
        rows = np.zeros((3000, 4), np.float32)
        rows[:, :3] = np.random.default_rng(0).uniform(-10, 10, (3000, 3))
        m.set_input_source(rows[:100])
        assert df.run_chain_resident(m, rows, [df.make_filter("Range", min_range=1e6)]) == 0
        st, msg = _call(m, 0, np.eye(4))
        assert st == INVALID and "empty" in msg                                 # an empty cloud
        assert df.run_chain_resident(m, rows, []) == 3000
        for bad in (np.nan, np.inf, -np.inf):
            d = np.eye(4)
            d[1, 3] = bad
            st, msg = _call(m, 0, d)
            assert st == INVALID and "finite" in msg                            # a non-finite delta
        for slot in (-1, 1):
            st, msg = _call(m, slot, np.eye(4))
            assert st == INVALID and "slot" in msg                              # a bad slot
        assert m._lib.smhip_filter_output_to_source_compensated(m._h, 0, None, None) == INVALID
        assert _source_size(m) == 100                                           # none of these touched the slot
        st, msg = _call(m, 0, np.eye(4))
        assert st == OK and _source_size(m) == 3000
        big = np.zeros((6000, 4), np.float32)
        big[:, :3] = np.random.default_rng(1).uniform(-10, 10, (6000, 3))
        assert df.run_chain_resident(m, big, []) == 6000                        # fits the workspace (the target side's size) ...
        st, msg = _call(m, 0, np.eye(4))
        assert st == CAPACITY and "max_source_points" in msg                    # ... but not a source slot
        assert _source_size(m) == 3000
    finally:
        m.close()


@pytest.mark.parametrize("bad", [1.0 + 2.0 ** -23, -1e-6, 1.5, float("nan"), float("inf")])
@pytest.mark.parametrize("row", [0, 255, 256, 999])
def test_a_factor_outside_the_unit_interval_is_reported_by_the_kernel(matcher, bad, row):
    rng = np.random.default_rng(3)
    rows = np.zeros((1000, 5), np.float32)
    rows[:, :4] = rng.uniform(-50, 50, (1000, 4))
    rows[:, 4] = rng.uniform(0, 1, 1000)
    good = rows.copy()
    rows[row, 4] = bad
    matcher.set_input_source(good)
    assert df.run_chain_resident(matcher, rows, []) == 1000
    out = np.full((1000, 5), -7.0, np.float32)
    st, msg = _call(matcher, 0, mc.check_deltas()["drive"], out)
    assert st == INVALID and "factor" in msg
    assert np.all(out == -7.0)                                                  # points5_out is not written
    assert _source_size(matcher) == 0                                           # the slot has no source after this failure
    assert workspace_rows(matcher, 1000).tobytes() == rows.tobytes()            # the workspace still holds the cloud
    matcher.set_input_target(good[:, :3], np.tile([0.0, 0.0, 1.0], (1000, 1)))     # a target, so that only the source is missing
    with pytest.raises(sm.SmhipError) as e:
        matcher.align(np.eye(4))
    assert e.value.status == NOT_READY
    # the device is fine and the next good cloud goes through; the edge factors 0 and 1 are inside
    good[0, 4], good[1, 4] = 0.0, 1.0
    assert df.run_chain_resident(matcher, good, []) == 1000
    got = df.output_to_source_compensated(matcher, mc.check_deltas()["drive"], download=True)
    mc.assert_one_ulp(got[:, :3], mc.motion_compensation(good, mc.check_deltas()["drive"])[:, :3], "after a refusal")
    assert _source_size(matcher) == 1000
