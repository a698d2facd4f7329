"""Device GroundRemoval, GroundRemoval2 and RangeImage (smhip_filter_chain_ex_f32) against the CPU restatement
(tests/ground_filters_ref.py): bit-exact rows and source indices on 120 000-point scans of the seed-5 drive, mixed chains
composed with oracle/filters.py, the old filters through the extended entry, edge cases and the hand-over to a matcher."""
import ctypes

import numpy as np
import pytest

import ground_filters_ref as gf
import staticmapping_amd as sm
from staticmapping_amd import _capi, filters as df, synth
from oracle import filters as of

pytestmark = pytest.mark.gpu

# config/lidar_only_kitti.xml: the commented-out pre-filter (lines 28-37) and the scan matcher's inner filters (lines 56-70)
KITTI_PRE = dict(r_min=0.1, start_ground_height=-1.5, long_line_threshold=10, max_slope=0.12, max_error=0.1,
                 max_dist_to_line=0.10, max_start_height=0.6, thread_num=4)
KITTI_INNER = dict(KITTI_PRE, start_ground_height=-0.35)
KITTI_IMAGE = dict(top_angle=30.0, btm_angle=-20.0, vertical_line_num=60)


@pytest.fixture(scope="module")
def matcher():
    m = sm.IcpFastHip(pair_slots=2, max_source_points=131072, max_target_points=131072)
    yield m
    m.close()


@pytest.fixture(scope="module")
def drive():
    """two consecutive 120 000-point scans of the seed-5 drive (KITTI rows)"""
    poses = synth.drive_poses(4, seed=5, speed=8.0, speed_spread=2.0, yaw_rate_max=0.2, segment_s=1.0)
    scene = synth.make_drive_scene(poses, seed=5)
    return [synth.velodyne_scan(synth.scene_near(scene, P[:3, 3]), P, seed=500 + k, n_points=120_000)
            for k, P in enumerate(poses[1:3])]


def ref_dict(d) -> dict:
    """a descriptor as the restatement / oracle dict"""
    t = d.type
    if t in df._PARAMS_EX:
        f = {"type": t}
        for name, (arr, slot) in df._PARAMS_EX[t].items():
            f[name] = int(d.i[slot]) if arr == "i" else float(d.p[slot])
        f.pop("thread_num", None)
        f.pop("max_b", None)
        return f
    e = df.widen(d)
    f = of.default(t)
    names = {of.RANGE: ("min_range", "max_range"), of.AXIS_RANGE: ("min", "max"), of.RANDOM_SAMPLER: ("sampling_rate",),
             of.VOXEL_GRID: ("voxel_size",), of.BOUNDING_BOX_REMOVAL: ("min_x", "min_y", "min_z", "max_x", "max_y", "max_z")}[t]
    for k, nme in enumerate(names):
        f[nme] = e.p[k]
    if t == of.AXIS_RANGE:
        f["axis_index"] = e.i[0]
    if t == of.RANDOM_SAMPLER:
        f["seed"] = e.seed
    return f


def check(matcher, raw, chain):
    got, gsrc = df.run_chain(matcher, raw, chain)
    want, wsrc = gf.run_chain(raw if raw.shape[1] == 5 else of.with_factor(raw), [ref_dict(d) for d in chain])
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(gsrc, wsrc)
    return got, gsrc


@pytest.mark.parametrize("params", [{}, KITTI_PRE, KITTI_INNER], ids=["defaults", "kitti_pre", "kitti_inner"])
def test_ground_removal2_matches_restatement(matcher, drive, params):
    for scan in drive:
        got, _ = check(matcher, scan, [df.make_filter("GroundRemoval2", **params)])
        assert 0 < len(got) <= len(scan)


@pytest.mark.parametrize("params", [{}, dict(leaf_size=0.4, height_threshold=0.1, min_point_num_in_voxel=3)], ids=["defaults", "fine"])
def test_ground_removal_matches_restatement(matcher, drive, params):
    for scan in drive:
        got, _ = check(matcher, scan, [df.make_filter("GroundRemoval", **params)])
        assert 0 < len(got) < len(scan)


@pytest.mark.parametrize("params", [{}, KITTI_IMAGE], ids=["40x1800", "60x1800"])
def test_range_image_matches_restatement(matcher, drive, params):
    for scan in drive:
        got, _ = check(matcher, scan, [df.make_filter("RangeImage", **params)])
        assert 0 < len(got) < len(scan)


def test_mixed_chains(matcher, drive):
    scan = drive[0]
    chain = [df.make_filter("Range", min_range=5.0), df.make_filter("AxisRange", min=-2.0), df.make_filter("GroundRemoval2", **KITTI_PRE),
             df.make_filter("RangeImage", **KITTI_IMAGE), df.make_filter("RandomSampler", sampling_rate=0.5, seed=11)]
    got, _ = check(matcher, scan, chain)
    assert 0 < len(got) < len(scan) // 4
    check(matcher, of.with_factor(scan), [df.make_filter("GroundRemoval"), df.make_filter("BoundingBoxRemoval", min_x=-3, max_x=3,
                                                                                       min_y=-2, max_y=2, min_z=-3, max_z=1),
                                          df.make_filter("GroundRemoval2", **KITTI_INNER), df.make_filter("VoxelGrid", voxel_size=0.5)])


def test_old_filters_through_the_extended_entry(matcher, drive):
    scan = np.ascontiguousarray(drive[1])
    chain = [df.make_filter("Range", min_range=3.0, max_range=60.0), df.make_filter("AxisRange", min=-1.8, axis_index=2),
             df.make_filter("BoundingBoxRemoval", min_x=-2, max_x=2, min_y=-2, max_y=2, min_z=-2, max_z=2),
             df.make_filter("RandomSampler", sampling_rate=0.7, seed=4), df.make_filter("VoxelGrid", voxel_size=0.3)]
    for k in range(1, len(chain) + 1):
        want, wsrc = df.run_chain(matcher, scan, chain[:k])                     # smhip_filter_chain_f32
        arr = (_capi.FilterDescEx * k)(*[df.widen(d) for d in chain[:k]])
        n_out = ctypes.c_int()
        matcher._check(matcher._lib.smhip_filter_chain_ex_f32(matcher._h, scan.ctypes.data_as(_capi.c_float_p), 4, len(scan), arr, k,
                                                               ctypes.byref(n_out)))
        got = np.zeros((n_out.value, 5), np.float32)
        src = np.zeros(n_out.value, np.int32)
        matcher._check(matcher._lib.smhip_filter_get_output(matcher._h, got.ctypes.data_as(_capi.c_float_p),
                                                            src.ctypes.data_as(_capi.c_int32_p), n_out.value))
        assert got.tobytes() == want.tobytes() and np.array_equal(src, wsrc)


def test_edge_cases(matcher, drive):
    ground = [df.make_filter("GroundRemoval"), df.make_filter("GroundRemoval2", **KITTI_PRE), df.make_filter("RangeImage")]
    for f in ground:                                                           # empty input
        got, src = df.run_chain(matcher, np.zeros((0, 5), np.float32), [f])
        assert len(got) == 0 and len(src) == 0
    one = np.zeros((500, 5), np.float32)                                       # all points in one pixel / one grid / one voxel
    one[:, 0] = 10.0
    one[:, 2] = -1.0 + 1e-5 * np.arange(500, dtype=np.float32)
    got, src = check(matcher, one, [df.make_filter("RangeImage")])
    assert len(got) == 1 and src[0] == 0
    for f in ground[:2]:
        check(matcher, one, [f])
    mid = [df.make_filter("Range", min_range=1e6), df.make_filter("GroundRemoval2"), df.make_filter("RangeImage")]
    assert len(check(matcher, drive[0], mid)[0]) == 0                          # everything removed mid-chain
    bad = of.with_factor(drive[0][:30000])                                     # non-finite rows
    bad[::7, 0] = np.nan
    bad[3::11, 2] = np.inf
    bad[5::13, 1] = -np.inf
    for f in ground:
        got, src = check(matcher, bad, [f])
        fin = np.isfinite(bad[:, :3]).all(axis=1)
        if f.type == df.RANGE_IMAGE:
            assert fin[src].all()                                              # dropped by RangeImage
        else:
            assert np.isin(np.flatnonzero(~fin), src).all()                    # kept by both ground filters


def test_invalid_and_oversize_configs(matcher):
    raw = of.with_factor(np.random.default_rng(1).uniform(-20, 20, (1000, 4)).astype(np.float32))
    bad = [df.make_filter("GroundRemoval2", bin_num=0), df.make_filter("GroundRemoval2", segment_num=-1),
           df.make_filter("GroundRemoval2", bin_num=4097), df.make_filter("GroundRemoval2", bin_num=4096, segment_num=1025),
           df.make_filter("GroundRemoval2", search_angle=800.0), df.make_filter("RangeImage", vertical_line_num=0),
           df.make_filter("RangeImage", horizontal_line_num=0), df.make_filter("RangeImage", vertical_line_num=4096, horizontal_line_num=1025),
           df.make_filter("GroundRemoval", leaf_size=0.0)]
    for d in bad:
        assert not df.config_valid(d)
        with pytest.raises(sm.SmhipError) as e:
            df.run_chain(matcher, raw, [df.make_filter("Range"), d])
        assert e.value.status == 1                                             # SMHIP_ERR_INVALID_ARGUMENT
    far = raw.copy()
    far[0, 0] = 1.0e7                                                          # voxel index beyond +-2^20 at leaf 0.8
    with pytest.raises(sm.SmhipError) as e:
        df.run_chain(matcher, far, [df.make_filter("GroundRemoval")])
    assert e.value.status == 1
    for d in (df.make_filter("GroundRemoval"), df.make_filter("GroundRemoval2"), df.make_filter("RangeImage")):
        arr = (_capi.FilterDesc * 1)()                                         # the old entry refuses the new ids
        arr[0].type = d.type
        n_out = ctypes.c_int()
        st = matcher._lib.smhip_filter_chain_f32(matcher._h, raw.ctypes.data_as(_capi.c_float_p), 5, len(raw), arr, 1, ctypes.byref(n_out))
        assert st == 1
    check(matcher, raw, [df.make_filter("GroundRemoval2", bin_num=4096, segment_num=1024)])   # the limits themselves run


def test_output_to_source_matches_the_host_hand_over(matcher, drive):
    a, b = drive
    chain = [df.make_filter("Range", min_range=5.0), df.make_filter("AxisRange", min=-2.0), df.make_filter("GroundRemoval2", **KITTI_INNER),
             df.make_filter("RangeImage", **KITTI_IMAGE)]
    q, n = sm.calculate_normals(a[:, :3].astype(np.float64))
    ok = np.isfinite(n).all(axis=1)
    guess = synth.make_pose(t=(0.8, 0, 0))
    matcher.set_options(max_iteration=30, early_exit=1)
    matcher.set_input_target(q[ok], n[ok])
    filtered, _ = df.run_chain(matcher, np.ascontiguousarray(b), chain)
    df.output_to_source(matcher, 0)                                            # device-resident hand-over
    _, R1 = matcher.align(guess)
    matcher.set_input_source(np.ascontiguousarray(filtered[:, :3]))            # the same cloud through the host
    _, R2 = matcher.align(guess)
    assert np.array_equal(R1, R2)
