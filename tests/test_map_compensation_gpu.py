"""Motion compensation after optimisation on the device: smhip_mrvm_insert_compensated_f32,
smhip_submap_build_compensated_f32 and smhip_shard --map-compensate.

The two fused calls are compared bit for bit with the composition a caller had to make before: the rows through an unfiltered
chain, smhip_filter_output_to_source_compensated with the rows downloaded, then the plain stride-5 call.  Every part of that
composition is pinned against numpy and the oracle elsewhere (tests/test_motion_comp_gpu.py, tests/test_static_map_gpu.py,
tests/test_submap_gpu.py), so no tolerance enters here.  The one check with a bound is the purpose: the device's compensated map of a
skewed drive against the oracle's map of the unskewed scans."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import map_compensation_ref as ref
import motion_comp_ref as mc

INVALID = 1                                             # SMHIP_ERR_INVALID_ARGUMENT
ROWS = [1, 255, 256, 257, 5_000]                        # one row, around the 256-thread block, many blocks


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_dump(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
            and np.array_equal(_bits(a[4]), _bits(b[4])))


@pytest.fixture(scope="module")
def drive():
    return ref.skewed_drive(4, 5_000)


@pytest.fixture(scope="module")
def matcher():
    import staticmapping_amd as sm
    m = sm.IcpFastHip(device=0, pair_slots=1, max_source_points=16384, max_target_points=16384)
    yield m
    m.close()


def _rows(scan, n, stride):
    """n raw rows: KITTI rows (stride 4), or InnerPointType rows whose factors are not i / n and touch both ends of [0, 1]"""
    rows = np.ascontiguousarray(scan[:n, :4], np.float32)
    if stride == 4:
        return rows
    f = np.random.default_rng(n).random(n).astype(np.float32)
    f[:1] = 1.0                                           # (n may be 0: an empty frame of a submap)
    f[-1:] = 0.0
    return np.concatenate([rows, f[:, None]], axis=1)


def _composition_rows5(matcher, rows, delta):
    """What a caller needed before: the rows through an unfiltered chain, de-skewed by the filter unit, downloaded."""
    from staticmapping_amd import filters as df
    assert df.run_chain_resident(matcher, rows, []) == len(rows)
    out = df.output_to_source_compensated(matcher, delta, download=True)
    assert out.shape == (len(rows), 5)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [4, 5])
@pytest.mark.parametrize("delta_name", ["drive", "half_turn", "tiny", "identity"])
def test_fused_insert_equals_the_composition_bit_for_bit(drive, matcher, stride, delta_name):
    import staticmapping_amd as sm
    delta = mc.check_deltas()[delta_name]
    scale = 255.0 if stride == 4 else 1.0
    pose = drive["poses"][1]
    fused = sm.MultiResolutionVoxelMapHip(table_log2=14, max_cloud_points=5_000)
    composed = sm.MultiResolutionVoxelMapHip(table_log2=14, max_cloud_points=5_000)
    for n in ROWS:
        rows = _rows(drive["skewed"][1], n, stride)
        for m in (fused, composed):                       # a map that holds a frame already: the new rays meet existing voxels
            m.clear()
            m.insert_transformed(drive["clean"][0], drive["poses"][0], 255.0)
        fused.insert_compensated(rows, pose, delta, intensity_scale=scale)
        rows5 = _composition_rows5(matcher, rows, delta)
        if stride == 4:
            assert np.array_equal(_bits(rows5[:, 4]), _bits(ref.factors(rows)))          # the collector's i / n
        composed.insert_transformed(rows5, pose, intensity_scale=scale)
        assert fused.voxel_count() == composed.voxel_count(), n
        assert fused.last_skipped == composed.last_skipped == 0 and fused.last_warning == composed.last_warning == "", n
        a, b = fused.dump(), composed.dump()
        assert len(a[0]) > 0 and _same_dump(a, b), (n, stride, delta_name)
    fused.close(); composed.close()


@pytest.mark.gpu
def test_compensated_device_map_restores_the_static_map(drive):
    """The skewed 4 x 5 000 drive: the device's compensated map against the oracle's map A of the unskewed scans, and against the
    oracle's map of the restatement's rows (device sin and libm differ in the last bit: the same cap, not equality)."""
    import staticmapping_amd as sm
    from oracle import cref
    from test_static_map_gpu import oracle_rows
    dev = sm.MultiResolutionVoxelMapHip(table_log2=16, max_cloud_points=5_000)
    truth, restated = cref.Mrvm(), cref.Mrvm()
    for k, P in enumerate(drive["poses"]):
        origin = np.asarray(P, np.float64)[:3, 3].astype(np.float32)
        dev.insert_compensated(drive["skewed"][k], P, drive["motions"][k], 255.0)
        truth.insert(oracle_rows(drive["clean"][k], P, 255.0), origin)
        restated.insert(ref.compensated_world_rows(drive["skewed"][k], P, drive["motions"][k], 255.0), origin)
    A, D, R = ref.kept_keys(truth), ref.kept_keys(dev), ref.kept_keys(restated)
    to_truth, to_restated = ref.differing_share(A, D), len(D ^ R) / float(len(A))
    print("|A| = %d; device compensated map: differing keys / |A| = %.4f against A, %.4f against the restatement's map" % (len(A), to_truth, to_restated))
    assert len(A) > 300
    assert to_truth <= 0.01
    assert to_restated <= 0.01
    dev.close(); truth.close(); restated.close()


@pytest.mark.gpu
def test_refusals_leave_the_map_bit_for_bit_as_it_was(drive):
    import staticmapping_amd as sm
    from staticmapping_amd import _capi
    dev = sm.MultiResolutionVoxelMapHip(table_log2=12, max_cloud_points=5_000)      # (a small table: an insert of 5 000 rows would grow it)
    dev.insert_compensated(drive["skewed"][0][:1500], drive["poses"][0], drive["motions"][0], 255.0)
    before, voxels = dev.dump(), dev.voxel_count()
    good = _rows(drive["skewed"][1], 5_000, 5)
    pose, motion = drive["poses"][1], drive["motions"][1]
    for bad_factor in (np.nan, 1.5):
        rows = good.copy()
        rows[4_321, 4] = bad_factor
        with pytest.raises(sm.SmhipError) as e:
            dev.insert_compensated(rows, pose, motion)
        assert e.value.status == INVALID and "factor" in str(e.value)
        assert dev.voxel_count() == voxels and _same_dump(dev.dump(), before)
    bad_motion = motion.copy()
    bad_motion[0, 3] = np.inf
    with pytest.raises(sm.SmhipError) as e:
        dev.insert_compensated(good, pose, bad_motion)
    assert e.value.status == INVALID and "motion" in str(e.value)
    cm = np.ascontiguousarray(np.asarray(pose, np.float64).T).ravel()
    st = dev._lib.smhip_mrvm_insert_compensated_f32(dev._h, good.ctypes.data_as(_capi.c_float_p), 5, len(good), cm.ctypes.data_as(_capi.c_double_p), None, 1.0)
    assert st == INVALID
    # what the plain call refuses: a non-finite pose, an origin beyond +-2^20 voxels, stride 3, an empty cloud
    nan_pose = pose.copy(); nan_pose[1, 2] = np.nan
    far_pose = pose.copy(); far_pose[0, 3] = 3.0e5
    for rows, P in ((good, nan_pose), (good, far_pose), (good[:, :3], pose), (good[:0], pose)):
        with pytest.raises(sm.SmhipError) as e:
            dev.insert_compensated(rows, P, motion)
        assert e.value.status == INVALID
    assert dev.voxel_count() == voxels and _same_dump(dev.dump(), before)
    dev.insert_compensated(good, pose, motion)                                      # an ordinary insert afterwards succeeds
    assert dev.voxel_count() > voxels and dev.last_warning == ""
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [4, 5])
@pytest.mark.parametrize("voxel_size", [0.0, 0.2])
def test_compensated_submap_build_equals_the_composition_bit_for_bit(drive, matcher, stride, voxel_size):
    import staticmapping_amd as sm
    from map_package_ref import submap_local_poses
    deltas = mc.check_deltas()
    sizes, motions = [257, 0, 255], [deltas["half_turn"], deltas["drive"], deltas["tiny"]]     # (the empty frame has a motion too)
    frames = [_rows(drive["skewed"][k], n, stride) for k, n in enumerate(sizes)]
    local = submap_local_poses([drive["poses"][k] for k in range(3)])
    composed = [_composition_rows5(matcher, f, d) if len(f) else np.zeros((0, 5), np.float32) for f, d in zip(frames, motions)]
    want, want_src = sm.build_submap(matcher, composed, local, voxel_size)
    got, got_src = sm.build_submap(matcher, frames, local, voxel_size, motions=motions)
    assert len(want) > 0 and (voxel_size > 0 or len(want) == sum(sizes))
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want))       # rows and factors
    assert np.array_equal(got_src, want_src)
    plain, _ = sm.build_submap(matcher, frames, local, voxel_size)                  # (and the motions were not ignored)
    assert plain.shape != got.shape or not np.array_equal(_bits(plain), _bits(got))


@pytest.mark.gpu
def test_compensated_submap_build_refusals(drive, matcher):
    import staticmapping_amd as sm
    from map_package_ref import submap_local_poses
    frames = [_rows(drive["skewed"][k], 300, 5) for k in range(2)]
    local = submap_local_poses([drive["poses"][k] for k in range(2)])
    motions = [drive["motions"][0], drive["motions"][1]]
    kept, _ = sm.build_submap(matcher, frames, local, 0.0, motions=motions)
    bad = [m.copy() for m in motions]
    bad[1][2, 1] = np.nan
    with pytest.raises(sm.SmhipError) as e:                                         # refused before anything is touched
        sm.build_submap(matcher, frames, local, 0.2, motions=bad)
    assert e.value.status == INVALID and "motion" in str(e.value)
    from staticmapping_amd.submap import get_submap
    assert np.array_equal(_bits(get_submap(matcher, len(kept))[0]), _bits(kept))
    # a bad factor: reported after the rows were written, the unfiltered concatenation resident (also with a voxel size)
    frames[1][7, 4] = 1.5
    with pytest.raises(sm.SmhipError) as e:
        sm.build_submap(matcher, frames, local, 0.2, motions=motions)
    assert e.value.status == INVALID and "factor" in str(e.value)
    rows, src = get_submap(matcher, 600)
    assert np.array_equal(src, np.arange(600)) and np.array_equal(_bits(rows[:300]), _bits(kept[:300]))
    assert np.array_equal(_bits(rows[300:, 4]), _bits(frames[1][:, 4]))
    frames[1][7, 4] = 0.5
    assert len(sm.build_submap(matcher, frames, local, 0.0, motions=motions)[0]) == 600


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
def _exe():
    from staticmapping_amd import build
    build.build()
    return build.build_shard_driver()


def _run(args):
    r = subprocess.run([_exe()] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def drive_on_disk(drive, tmp_path_factory):
    """The skewed drive as KITTI .bin files and its pose file; the poses and motions are those of the file AS WRITTEN."""
    from staticmapping_amd import kitti
    root = tmp_path_factory.mktemp("compensated_drive")
    seq = root / "seq"
    seq.mkdir()
    for k, s in enumerate(drive["skewed"]):
        kitti.write_bin(kitti.scan_path(str(seq), k), s)
    pose_file = root / "poses.txt"
    base = np.linalg.inv(drive["poses"][0])
    kitti.write_poses(str(pose_file), np.stack([base @ P for P in drive["poses"]]))
    poses = kitti.read_poses(str(pose_file))
    files = kitti.list_scans(str(seq))
    return dict(seq=str(seq), pose_file=str(pose_file), poses=poses, motions=ref.sweep_motions(poses),
                rows=[kitti.read_bin(f, scale_intensity=False) for f in files])


@pytest.mark.gpu
def test_driver_map_compensate(drive_on_disk, tmp_path):
    import staticmapping_amd as sm
    from staticmapping_amd import pcd
    from test_static_map_gpu import MAP_KEYS
    d = drive_on_disk
    common = ["--scans", d["seq"], "--map-poses", d["pose_file"]]
    comp, off, none = tmp_path / "comp.pcd", tmp_path / "off.pcd", tmp_path / "none.pcd"
    line = _run(common + ["--map", str(comp), "--map-compensate", "1"])
    assert list(line) == ["driver", "poses_file", "poses_in_file"] + MAP_KEYS + ["map_compensated"] and line["map_compensated"] == 1
    dev = sm.MultiResolutionVoxelMapHip(table_log2=16, max_cloud_points=5_000)
    for k in range(4):
        dev.insert_compensated(d["rows"][k], d["poses"][k], d["motions"][k], 255.0)
    want = dev.output_to_point_cloud(0.6, sorted=True)
    dev.close()
    rows, fields = pcd.read_pcd(str(comp))
    assert fields == ["x", "y", "z", "intensity"] and len(want) > 300
    assert np.array_equal(_bits(rows), _bits(want))
    # without the flag, and with --map-compensate 0: the bytes and the line of today
    line_off = _run(common + ["--map", str(off), "--map-compensate", "0"])
    line_none = _run(common + ["--map", str(none)])
    assert off.read_bytes() == none.read_bytes() and off.read_bytes() != comp.read_bytes()
    assert list(line_off) == list(line_none) == ["driver", "poses_file", "poses_in_file"] + MAP_KEYS
    # --map-every does not change a frame's motion: frames 0 and 2 under their own motions
    every = tmp_path / "every.pcd"
    _run(common + ["--map", str(every), "--map-compensate", "1", "--map-every", "2"])
    dev = sm.MultiResolutionVoxelMapHip(table_log2=16, max_cloud_points=5_000)
    for k in (0, 2):
        dev.insert_compensated(d["rows"][k], d["poses"][k], d["motions"][k], 255.0)
    assert np.array_equal(_bits(pcd.read_pcd(str(every))[0]), _bits(dev.output_to_point_cloud(0.6, sorted=True)))
    dev.close()


@pytest.mark.gpu
def test_driver_map_package_compensate(drive_on_disk, matcher, tmp_path):
    import staticmapping_amd as sm
    from map_package_ref import submap_local_poses
    from staticmapping_amd import map_package as mp
    from staticmapping_amd.submap import text_voxel_size
    d = drive_on_disk
    out, want = tmp_path / "driver", tmp_path / "python"
    out.mkdir(); want.mkdir()
    line = _run(["--scans", d["seq"], "--map-poses", d["pose_file"], "--map-package", str(out), "--submap-frames", "2", "--map-compensate", "1"])
    assert line["package_submaps"] == 2 and list(line)[-1] == "map_compensated" and line["map_compensated"] == 1
    submaps, plain = [], []
    for k in range(2):
        idx = [2 * k, 2 * k + 1]
        local = submap_local_poses([d["poses"][f] for f in idx])
        args = (matcher, [d["rows"][f] for f in idx], local, text_voxel_size(0.1))
        submaps.append((d["poses"][2 * k], sm.build_submap(*args, motions=[d["motions"][f] for f in idx])[0]))
        plain.append(sm.build_submap(*args)[0])
    assert any(a.shape != b[1].shape or not np.array_equal(_bits(a), _bits(b[1])) for a, b in zip(plain, submaps))
    mp.save_map_package(submaps, str(want) + os.sep, mp.MapPackageOptions(), intensity_scale=255.0)
    assert sorted(os.listdir(out)) == sorted(os.listdir(want)) and len(os.listdir(out)) >= 2
    for name in os.listdir(want):
        assert (out / name).read_bytes() == (want / name).read_bytes(), name
