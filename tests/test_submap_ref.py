"""The numpy restatement of Submap::InsertFrame's cloud (tests/submap_ref.py) on cases with known answers, and the Python
bookkeeping of static_map::Submap (staticmapping_amd/submap.py).  No GPU."""
import numpy as np
import pytest

import submap_ref as sr
from staticmapping_amd import synth
from staticmapping_amd.submap import SubmapBuilder, text_voxel_size


def test_one_identity_frame_without_voxel_filter_returns_the_rows():
    rng = np.random.default_rng(3)
    rows = rng.uniform(-50, 50, (1000, 5)).astype(np.float32)
    cloud, src = sr.build_submap([rows], [np.eye(4)], 0.0)
    assert cloud.dtype == np.float32 and np.array_equal(cloud, rows)
    assert np.array_equal(src, np.arange(1000))
    # rows of 4 floats get the collector's factor i / n of their own frame
    cloud4, _ = sr.build_submap([rows[:, :4], rows[:10, :4]], [np.eye(4), np.eye(4)], 0.0)
    assert np.array_equal(cloud4[:, :4], np.concatenate([rows[:, :4], rows[:10, :4]]))
    assert np.array_equal(cloud4[:1000, 4], (np.arange(1000) / 1000).astype(np.float32))
    assert np.array_equal(cloud4[1000:, 4], (np.arange(10) / 10).astype(np.float32))


def test_hand_built_grid_across_two_frames():
    # voxel 1.0: frame 0 holds two points of voxel (0, 0, 0) and one of voxel (2, 0, 0); frame 1, shifted by +2 m in x, brings
    # one more point into voxel (2, 0, 0) and one into voxel (-1, 3, 0)
    f0 = np.array([[0.25, 0.0, 0.0, 10.0, 0.5], [-0.25, 0.25, 0.0, 20.0, 0.5], [2.25, 0.0, 0.0, 30.0, 0.5]], np.float32)
    f1 = np.array([[-0.25, 0.25, 0.0, 50.0, 0.5], [-3.0, 3.0, 0.25, 70.0, 0.5]], np.float32)
    shift = np.eye(4); shift[0, 3] = 2.0
    cloud, src = sr.build_submap([f0, f1], [np.eye(4), shift], 1.0)
    assert np.array_equal(src, [-1, -1, -1])
    # key order: x, then y, then z of the voxel index
    expect = np.array([[-1.0, 3.0, 0.25, 70.0, 0.0], [0.0, 0.125, 0.0, 15.0, 0.0], [2.0, 0.125, 0.0, 40.0, 0.0]], np.float32)
    assert np.array_equal(cloud, expect)
    # without the filter: the plain concatenation, frame order then point order, factor carried
    plain, src = sr.build_submap([f0, f1], [np.eye(4), shift], 0.0)
    assert np.array_equal(src, np.arange(5))
    assert np.array_equal(plain[:3], f0) and np.array_equal(plain[3:, 0], [1.75, -1.0]) and np.array_equal(plain[3:, 3:], f1[:, 3:])


def test_voxel_sums_run_in_frame_order_then_point_order():
    # three values whose double sum depends on the order: (1e17 + 1) - 1e17 = 0 in double, 1e17 - 1e17 + 1 = 1
    big = np.float32(1e17)
    f0 = np.array([[0.0, 0.0, 0.0, big, 0.0]], np.float32)
    f1 = np.array([[0.0, 0.0, 0.0, 1.0, 0.0]], np.float32)
    f2 = np.array([[0.0, 0.0, 0.0, -big, 0.0]], np.float32)
    eye = np.eye(4)
    a, _ = sr.build_submap([f0, f1, f2], [eye, eye, eye], 1.0)
    b, _ = sr.build_submap([f0, f2, f1], [eye, eye, eye], 1.0)
    assert a[0, 3] == 0.0 and b[0, 3] == np.float32(1.0 / 3.0)


def test_voxel_size_travels_through_six_decimals():
    assert sr.text_voxel_size(0.1) == float(np.float32(0.1))                 # "0.100000"
    assert sr.text_voxel_size(0.1234567) == float(np.float32(0.123457))      # rounded to six decimals, then to float
    assert sr.text_voxel_size(0.1234564) == float(np.float32(0.123456))
    assert sr.text_voxel_size(2.5e-7) == 0.0                                 # "0.000000": below the text's resolution
    for v in (0.1, 0.1234567, 0.05, 0.2, 1.0):
        assert text_voxel_size(v) == sr.text_voxel_size(v)                   # the package takes it the same way


def test_output_is_in_key_order():
    scene = synth.make_scene(0)
    poses = [synth.make_pose(t=(0.8 * k, 0.03 * k, 0.0), rpy_deg=(0, 0, 0.6 * k)) for k in range(2)]
    frames = [synth.velodyne_scan(scene, P, seed=90 + k, n_points=3000) for k, P in enumerate(poses)]
    size = sr.text_voxel_size(0.1)
    cloud, _ = sr.build_submap(frames, sr.local_poses(poses), size)
    q = cloud[:, :3] / np.float32(size)
    ijk = np.where(q >= 0, np.floor(q.astype(np.float64) + 0.5), np.ceil(q.astype(np.float64) - 0.5)).astype(np.int64)
    key = ((ijk[:, 0] + (1 << 20)) << 42) | ((ijk[:, 1] + (1 << 20)) << 21) | (ijk[:, 2] + (1 << 20))
    # an average may leave its voxel by a rounding step, so order is checked on the voxels of the inputs, one output row each
    full = sr.concatenate(frames, sr.local_poses(poses))
    qi = full[:, :3] / np.float32(size)
    vi = np.where(qi >= 0, np.floor(qi.astype(np.float64) + 0.5), np.ceil(qi.astype(np.float64) - 0.5)).astype(np.int64)
    vkey = np.unique(((vi[:, 0] + (1 << 20)) << 42) | ((vi[:, 1] + (1 << 20)) << 21) | (vi[:, 2] + (1 << 20)))
    assert len(cloud) == len(vkey) < len(full)
    assert (key == vkey).mean() > 0.9 and np.all(np.diff(vkey) > 0)


def test_builder_bookkeeping():
    poses = [synth.make_pose(t=(1.0 + 0.8 * k, 0.1 * k, 0.0), rpy_deg=(0, 0, 5.0 * k)) for k in range(4)]
    b = SubmapBuilder(frame_count=3, enable_voxel_filter=True, voxel_size=0.1234567)
    for k in range(3):
        assert not b.full()
        b.insert_frame(np.zeros((4, 4), np.float32), poses[k])
    assert b.full()
    with pytest.raises(RuntimeError):
        b.insert_frame(np.zeros((4, 4), np.float32), poses[3])
    assert np.array_equal(b.local_pose(0), np.eye(4)) and np.array_equal(b.first_frame_pose(), poses[0])
    for k in (1, 2):
        assert np.allclose(b.local_pose(k), np.linalg.inv(poses[0]) @ poses[k], atol=1e-15)
        assert np.allclose(b.local_pose(k), sr.local_poses(poses[:3])[k], atol=1e-15)
    assert b.device_voxel_size() == float(np.float32(0.123457))
    assert SubmapBuilder().device_voxel_size() == 0.0                         # enable_voxel_filter = false by default
    assert (SubmapBuilder().frame_count, SubmapBuilder().voxel_size) == (5, 0.1)
