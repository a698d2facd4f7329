"""The map package on the device (builder/map_package.cc): the clipped insert, the clipped and recentred output, the clear, and the
package end to end through staticmapping_amd.map_package.save_map_package and smhip_shard --map-package.  Every comparison is bit
for bit; the expected value is oracle.cref.Mrvm fed the rows the restatement (tests/map_package_ref.py) clips, compared through
dump() as tests/test_static_map_gpu.py does."""
import json
import os
import subprocess
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import map_package_ref as ref

# smhip_shard's summary line without --map-package (tests/test_static_map_gpu.py::TODAY_KEYS) and what the flag adds
TODAY_KEYS = ["driver", "n_gpus", "pairs", "pairs_rank0", "seconds", "pairs_per_s", "read_upload_prepare_s_rank0", "wait_for_readers_s_rank0",
              "upload_s_rank0", "prepare_targets_s_rank0", "mean_score", "mean_iterations", "unfinished_pairs", "batch", "readers",
              "pinned_read_buffers", "warmup_batch_before_the_clock_s", "steady_state_pairs_per_s_rank0", "poses_file"]
PACKAGE_KEYS = ["package_dir", "package_pieces", "package_submaps", "package_points", "package_seconds"]
SETTINGS = [dict(), dict(high_resolution=0.25, hit_prob=0.7, miss_prob=0.4, max_point_num_in_cell=3, z_offset=0.3)]
HUGE = ((-1.0e6, -1.0e6), (1.0e6, 1.0e6))
# the package of the end-to-end tests: 20 scans of 10 000 points, 0.8 m apart, four submaps of five frames about 4 m apart.  With
# pieces 8 m wide and a border of 2 m the plan has three pieces along the drive; piece 0 (box x in [-2, 6]) takes submaps 0 and 1
# whole and submap 2 clipped, and submap 3 is not in it -- asserted on the restatement in the `drive` fixture
SUBMAP_FRAMES, PIECE_WIDTH, BORDER_OFFSET = 5, 8.0, 2.0


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _scans(n_scans=8, n_points=20_000, seed=5):
    from staticmapping_amd import synth
    poses = synth.drive_poses(n_scans, seed=seed, speed=8.0, hz=10.0, yaw_rate_max=0.2)
    scene = synth.make_drive_scene(poses, seed=seed)
    return [synth.velodyne_scan(synth.scene_near(scene, P[:3, 3]), P, seed=1000 + k, n_points=n_points) for k, P in enumerate(poses)], poses


def _assert_same_map(dev, ora):
    kd, pd, md, nd, qd = dev.dump()
    ko, po, mo, no, qo = ora.dump()
    assert np.array_equal(kd, ko)
    assert np.array_equal(pd, po), int((pd != po).sum())
    assert np.array_equal(md, mo) and np.array_equal(nd, no)
    assert np.array_equal(_bits(qd), _bits(qo))


def _same_dump(a, b):
    return all(np.array_equal(x, y) if x.dtype != np.float32 else np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _rows(scan, stride):
    if stride == 4:
        return np.ascontiguousarray(scan[:, :4], np.float32)
    return np.concatenate([scan[:, :4], (np.arange(len(scan), dtype=np.float32) / len(scan))[:, None]], axis=1).astype(np.float32)


def _clipped_insert_both(dev, ora, rows, pose, box, scale):
    """One clipped insert on the device and the reference's on the oracle (map_package.cc:169-182); returns (kept on the device, kept
    by the restatement)."""
    kept = dev.insert_transformed_clipped(rows, pose, box[0], box[1], intensity_scale=scale)
    world = ref.transform_rows(rows, pose, scale)
    want = world[ref.rows_in_box(world, box[0], box[1])]
    if len(want):                                                 # :177: an empty selection makes no insert
        ora.insert(want, np.asarray(pose, np.float64)[:3, 3].astype(np.float32))
    return kept, len(want)


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [4, 5])
@pytest.mark.parametrize("settings", SETTINGS)
def test_clipped_insert_equals_the_reference_loop_on_the_clipped_rows(stride, settings):
    import staticmapping_amd as sm
    from oracle import cref
    scans, poses = _scans(4)
    scale = 255.0 if stride == 4 else 1.0
    dev = sm.MultiResolutionVoxelMapHip(table_log2=16, max_cloud_points=20_000, **settings)
    ora = cref.Mrvm(**settings)
    maxp = settings.get("max_point_num_in_cell", 10)
    res = np.float32(settings.get("high_resolution", 0.1))

    def step(rows, pose, box, expect=None):
        kept, want = _clipped_insert_both(dev, ora, rows, pose, box, scale)
        assert kept == want and (expect is None or expect(kept)), (kept, want, len(rows))
        assert dev.last_warning == ""
        _assert_same_map(dev, ora)                                # after EVERY insert
        return kept

    def half_box(rows, pose):                                     # x' up to its median: about half of the rows
        x = ref.transform_rows(rows, pose, scale)[:, 0].astype(np.float64)
        return ((-1.0e6, -1.0e6), (float(np.median(x)) + 1e-3, 1.0e6))

    r0, r1, r2 = _rows(scans[0], stride), _rows(scans[1], stride), _rows(scans[2], stride)
    step(r0, poses[0], HUGE, lambda k: k == 20_000)                                          # keeps every row: n = 20 000
    step(r1, poses[1], half_box(r1, poses[1]), lambda k: 9_000 < k < 11_000)                # about half, more than one block
    before = dev.dump()
    step(r2[:257], poses[2], ((500.0, 500.0), (600.0, 600.0)), lambda k: k == 0)            # keeps none: no insert
    assert _same_dump(before, dev.dump())
    for n in (257, 256, 255, 1):                                                            # around one block of 256 rows
        step(r2[1000:1000 + n], poses[2], HUGE, lambda k, n=n: k == n)
        step(r2[3000:3000 + n], poses[2], half_box(r2[3000:3000 + 257], poses[2]))
    # rows whose transformed x or y EQUALS a bound: the pose is an integer translation and the coordinates small integers, so the float
    # results are exact; both bounds keep them (closed test).  Their neighbours one float outside, a NaN row and Inf rows are dropped.
    T = np.eye(4); T[:3, 3] = [3.0, -2.0, 1.0]
    box = ((2.0, 0.0), (8.0, 4.0))
    out_lo, out_hi = np.nextafter(np.float32(-1), np.float32(-9)), np.float32(5 + 2.0 ** -20)     # (3 + either is a float: 2 - 2^-23, 8 + 2^-20)
    edge = np.array([[-1, 3, 0], [5, 3, 0], [1, 2, 0], [1, 6, 0], [-1, 2, 0], [5, 6, 0], [2, 4, 0.5],
                     [out_lo, 3, 0], [out_hi, 3, 0], [1, np.nextafter(np.float32(2), np.float32(0)), 0], [1, np.nextafter(np.float32(6), np.float32(9)), 0],
                     [np.nan, 3, 0], [1, np.nan, 0], [np.inf, 3, 0], [1, -np.inf, 0], [1, 3, np.inf], [1, 3, np.nan]], np.float32)
    rows = np.concatenate([edge, np.full((len(edge), stride - 3), 0.5, np.float32)], axis=1)
    mask = ref.rows_in_box(ref.transform_rows(rows, T, scale), *box)
    assert mask.tolist() == [True] * 7 + [False] * 10             # (a non-finite coordinate makes TransformPoint's x', y' NaN: outside)
    step(rows, T, box, lambda k: k == 7)
    # stability: 25 rows inside the box and 25 outside alternate within ONE voxel; more rows are kept than a voxel stores, and the
    # stored ones must be the first kept in their original order
    k = np.arange(50, dtype=np.float32)
    world = np.stack([np.where(k % 2 == 0, 1.02, 1.08), np.full(50, 1.05), 1.01 + 0.001 * k], axis=1).astype(np.float32)
    raw = (world - np.float32([3.0, -2.0, 1.0])).astype(np.float32)
    rows = np.concatenate([raw, (10 + k)[:, None]] + ([k[:, None] / 50] if stride == 5 else []), axis=1).astype(np.float32)
    w = ref.transform_rows(rows, T, scale)
    box = ((0.0, 0.0), (1.05, 2.0))
    inside = ref.rows_in_box(w, *box)
    assert inside.sum() == 25 > maxp and (~inside).sum() == 25
    assert len(np.unique(np.floor(w[:, :3] / res), axis=0)) == 1  # one voxel holds all fifty
    step(rows, T, box, lambda n: n == 25)
    dev.close(); ora.close()


@pytest.mark.gpu
def test_none_kept_leaves_the_map_as_it_was():
    import staticmapping_amd as sm
    scans, poses = _scans(2, 5_000)
    dev = sm.MultiResolutionVoxelMapHip(table_log2=12, max_cloud_points=5_000)
    far = ((900.0, 900.0), (901.0, 901.0))
    assert dev.insert_transformed_clipped(scans[0][:, :4], poses[0], *far, intensity_scale=255.0) == 0      # on an empty map
    assert dev.voxel_count() == 0 and dev.last_warning == ""
    dev.insert_transformed(scans[0][:, :4], poses[0], 255.0)
    before, log2 = dev.dump(), dev.table_log2
    assert dev.insert_transformed_clipped(scans[1][:, :4], poses[1], *far, intensity_scale=255.0) == 0      # status OK: nothing raised
    assert dev.last_warning == "" and dev.table_log2 == log2
    assert _same_dump(before, dev.dump())
    # and the next insert behaves as if that call had never been made
    twin = sm.MultiResolutionVoxelMapHip(table_log2=12, max_cloud_points=5_000)
    twin.insert_transformed(scans[0][:, :4], poses[0], 255.0)
    for m in (dev, twin):
        m.insert_transformed(scans[1][:, :4], poses[1], 255.0)
    assert _same_dump(dev.dump(), twin.dump())
    dev.close(); twin.close()


@pytest.mark.gpu
def test_clipped_insert_refusals_leave_the_map_unchanged():
    import staticmapping_amd as sm
    scans, poses = _scans(2, 5_000)
    dev = sm.MultiResolutionVoxelMapHip(table_log2=14, max_cloud_points=5_000)
    dev.insert_transformed(scans[0][:, :4], poses[0], 255.0)
    before = dev.dump()
    rows, P = scans[1][:, :4], poses[1]
    bad_pose = P.copy(); bad_pose[1, 2] = np.nan
    far = P.copy(); far[0, 3] = 3.0e5                                     # an origin beyond +-2^20 voxels
    big = np.tile(rows, (2, 1))[:5_001]                                  # one row more than max_cloud_points
    cases = [(rows, P, (np.nan, -50.0), (50.0, 50.0)), (rows, P, (-50.0, -50.0), (50.0, np.inf)), (rows, P, (-np.inf, -50.0), (50.0, 50.0)),
             (np.zeros((10, 3), np.float32), P, *HUGE), (np.zeros((10, 6), np.float32), P, *HUGE), (rows, bad_pose, *HUGE), (rows, far, *HUGE),
             (big, P, *HUGE), (np.zeros((0, 4), np.float32), P, *HUGE)]
    for r, pose, lo, hi in cases:
        with pytest.raises(sm.SmhipError):
            dev.insert_transformed_clipped(r, pose, lo, hi, intensity_scale=255.0)
        assert _same_dump(before, dev.dump())
    with pytest.raises(sm.SmhipError):
        dev.output_clipped((np.nan, 0.0), (1.0, 1.0), (0.0, 0.0))
    with pytest.raises(sm.SmhipError):
        dev.output_clipped((0.0, 0.0), (1.0, 1.0), (0.0, np.inf))
    dev.close()


@pytest.mark.gpu
def test_clipped_output_equals_sorted_output_clipped_and_recentred():
    import staticmapping_amd as sm
    from oracle import cref
    scans, poses = _scans(4)
    dev = sm.MultiResolutionVoxelMapHip(table_log2=12, max_cloud_points=20_000)          # (the table grows)
    ora = cref.Mrvm()
    for s, P in zip(scans, poses):
        dev.insert_transformed(s[:, :4], P, 255.0)
        ora.insert(ref.transform_rows(np.concatenate([s[:, :4], np.zeros((len(s), 1), np.float32)], axis=1), P, 255.0), P[:3, 3].astype(np.float32))
    _assert_same_map(dev, ora)
    # a box through the middle of the map whose bounds are no multiples of the voxel size, a centre that is no float
    middle = ((-7.13, -11.77), (3.03, 6.41))
    centre = (-2.05, -2.68)
    _, prob, _, npts, pts = ora.dump()
    both = 0
    for v in np.nonzero((npts > 1) & (prob >= int(np.float32(0.52) * np.float32(256))))[0]:
        m = ref.rows_in_box(pts[v, :npts[v]], *middle)
        both += bool(m.any() and not m.all())
    assert both >= 1                                               # a voxel with stored points on both sides of the box
    for thr in (0.6, 0.52):
        for kw in (dict(), dict(average=True), dict(rgb=True), dict(average=True, rgb=True)):
            whole = ref.sorted_output(ora, thr, **kw)
            want = ref.cut(whole, *middle, centre)
            assert 100 < len(want) < len(whole) - 100
            got = dev.output_clipped(*middle, centre, threshold=thr, **kw)
            assert np.array_equal(_bits(got), _bits(want)), (thr, kw)
            assert dev.output_clipped(*middle, centre, threshold=thr, count_only=True, **kw) == len(want)   # the counting call
            assert np.array_equal(_bits(dev.output_clipped(*middle, centre, threshold=thr, **kw)), _bits(got))   # the same bits again
            # a box that keeps nothing: 0 rows, no error
            assert dev.output_clipped((900.0, 900.0), (901.0, 901.0), (900.5, 900.5), threshold=thr, **kw).shape == (0, 4)
            # a box that keeps everything around centre 0: the SORTED output itself
            everything = dev.output_clipped(*HUGE, (0.0, 0.0), threshold=thr, **kw)
            assert np.array_equal(_bits(everything), _bits(dev.output_to_point_cloud(thr, sorted=True, **kw)))
            assert np.array_equal(_bits(everything), _bits(whole))
    packed = dev.output_clipped(*middle, centre, rgb=True, packed_rgb=True)[:, 3].view(np.uint32)
    assert len(packed) and np.all(packed >> 24 == 0xff)
    dev.close(); ora.close()


@pytest.mark.gpu
def test_clear_gives_a_fresh_map_in_the_grown_table():
    import staticmapping_amd as sm
    scans, poses = _scans(3)
    half = ((-1.0e6, -1.0e6), (2.5, 1.0e6))

    def fill(m):
        m.insert_transformed(scans[0][:, :4], poses[0], 255.0)
        m.insert_transformed_clipped(scans[1][:, :4], poses[1], *half, intensity_scale=255.0)
        m.insert_transformed(scans[2][:, :4], poses[2], 255.0)

    dev = sm.MultiResolutionVoxelMapHip(table_log2=12, max_cloud_points=20_000)
    fill(dev)
    grown = dev.table_log2
    assert grown > 12 and dev.voxel_count() > 4096
    first = (dev.dump(), dev.output_to_point_cloud(0.52, sorted=True))
    dev.clear()
    assert dev.voxel_count() == 0 and dev.table_log2 == grown and dev.last_warning == ""
    assert len(dev.output_to_point_cloud(0.52, sorted=True)) == 0 and len(dev.dump()[0]) == 0
    fill(dev)
    assert dev.table_log2 == grown
    fresh = sm.MultiResolutionVoxelMapHip(table_log2=12, max_cloud_points=20_000)
    fill(fresh)
    for m in (dev.dump(), first[0]):
        assert _same_dump(m, fresh.dump())
    want = fresh.output_to_point_cloud(0.52, sorted=True)
    assert np.array_equal(_bits(dev.output_to_point_cloud(0.52, sorted=True)), _bits(want)) and np.array_equal(_bits(first[1]), _bits(want))
    dev.close(); fresh.close()


# ---- the package end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drive(tmp_path_factory):
    """The drive on disk, its pose file AS WRITTEN, the submaps restated on the CPU (tests/submap_ref.py, which the device build equals
    bit for bit) and the package the restatement makes of them."""
    import submap_ref as sr
    from oracle import cref
    from staticmapping_amd import kitti
    scans, world = _scans(20, 10_000)
    root = tmp_path_factory.mktemp("package_drive")
    seq = root / "seq"
    seq.mkdir()
    for k, s in enumerate(scans):
        kitti.write_bin(kitti.scan_path(str(seq), k), s)
    base = np.linalg.inv(world[0])
    pose_file = root / "poses.txt"
    kitti.write_poses(str(pose_file), np.stack([base @ P for P in world]))
    poses = kitti.read_poses(str(pose_file))
    files = kitti.list_scans(str(seq))
    voxel = sr.text_voxel_size(0.1)
    frames, locals_, submaps = [], [], []
    for k in range(20 // SUBMAP_FRAMES):
        idx = range(SUBMAP_FRAMES * k, SUBMAP_FRAMES * (k + 1))
        frames.append([kitti.read_bin(files[f], scale_intensity=False) for f in idx])
        locals_.append(ref.submap_local_poses([poses[f] for f in idx]))
        submaps.append((poses[SUBMAP_FRAMES * k], sr.build_submap(frames[-1], locals_[-1], voxel)[0]))
    want, pl, stats = ref.package(submaps, cref.Mrvm, BORDER_OFFSET, PIECE_WIDTH, scale=255.0)
    # what the chosen width and border must give on this drive (on the restatement, before anything is compared with it)
    assert len(pl["pieces"]) >= 3
    assert any(whole > 0 and clipped > 0 for whole, clipped, _ in stats)          # a piece with a whole-inserted and a clipped member
    assert any(len(p["members"]) < len(submaps) for p in pl["pieces"])            # a submap that is absent from a piece
    assert sum(len(r) for r in want.values()) > 1_000
    return dict(seq=str(seq), pose_file=str(pose_file), frames=frames, local_poses=locals_, submaps=submaps, voxel=voxel, want=want, plan=pl)


def _check_package(directory, drive, descript="map_package.xml"):
    from staticmapping_amd import pcd
    assert sorted(os.listdir(directory)) == sorted(list(drive["want"]) + [descript])           # exactly the expected names
    for name, want in drive["want"].items():
        rows, fields = pcd.read_pcd(os.path.join(directory, name))
        assert fields == ["x", "y", "z", "intensity"]
        assert np.array_equal(_bits(rows), _bits(want)), name
    root = ET.parse(os.path.join(directory, descript)).getroot()
    assert root.tag == "MapPackage" and len(root) == len(drive["plan"]["pieces"])
    for e, p in zip(root, drive["plan"]["pieces"]):                                              # x-major
        assert (float(e.get("x")), float(e.get("y"))) == p["centre"] and e.get("file") == ref.piece_file("part_", p["x"], p["y"])
    assert open(os.path.join(directory, descript)).read() == ref.xml_text(drive["plan"], "part_")


def _exe():
    from staticmapping_amd import build
    build.build()
    return build.build_shard_driver()


def _run(args, rc=0):
    r = subprocess.run([_exe()] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == rc, r.stderr[-2000:]
    return r


@pytest.mark.gpu
def test_save_map_package_equals_the_restatement(drive, tmp_path):
    import staticmapping_amd as sm
    from staticmapping_amd import map_package as mp
    cap = max(sum(len(f) for f in fr) for fr in drive["frames"])
    matcher = sm.IcpFastHip(device=0, max_source_points=cap, max_target_points=cap)
    submaps = []
    for (pose, want), frames, lp in zip(drive["submaps"], drive["frames"], drive["local_poses"]):
        cloud, _ = sm.build_submap(matcher, frames, lp, drive["voxel"])                          # each submap built once on the device
        assert np.array_equal(_bits(cloud), _bits(want))
        submaps.append((pose, cloud))
    matcher.close()
    o = mp.MapPackageOptions(border_offset=BORDER_OFFSET, piece_width=PIECE_WIDTH)
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    res = mp.save_map_package(submaps, str(a) + os.sep, o, intensity_scale=255.0, table_log2=14)
    _check_package(str(a), drive)
    assert res["points"] == sum(len(r) for r in drive["want"].values()) and res["clipped_inserts"] > 0
    assert [os.path.basename(f) for f in res["files"]] == [ref.piece_file("part_", p["x"], p["y"]) for p in drive["plan"]["pieces"]] + ["map_package.xml"]
    mp.save_map_package(submaps, str(b) + os.sep, o, intensity_scale=255.0)                      # a second run: the same bytes
    for name in os.listdir(a):
        assert (a / name).read_bytes() == (b / name).read_bytes(), name


@pytest.mark.gpu
def test_driver_package_from_a_pose_file_equals_the_restatement(drive, tmp_path):
    out = tmp_path / "package"
    out.mkdir()
    flags = ["--submap-frames", str(SUBMAP_FRAMES), "--package-piece-width", str(PIECE_WIDTH), "--package-border-offset", str(BORDER_OFFSET)]
    r = _run(["--scans", drive["seq"], "--map-poses", drive["pose_file"], "--map-package", str(out)] + flags)
    _check_package(str(out), drive)
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert list(line) == ["driver", "poses_file", "poses_in_file"] + PACKAGE_KEYS
    assert line["package_dir"] == str(out) and line["package_pieces"] == len(drive["plan"]["pieces"]) and line["package_submaps"] == 4
    assert line["package_points"] == sum(len(x) for x in drive["want"].values()) and line["package_seconds"] > 0
    # other names, and a refused plan ends the run before any file is written
    other = tmp_path / "other"
    other.mkdir()
    _run(["--scans", drive["seq"], "--map-poses", drive["pose_file"], "--map-package", str(other) + "/", "--package-prefix", "piece_",
          "--package-descript", "index.xml"] + flags)
    assert sorted(os.listdir(other)) == sorted(["piece_%d_%d.pcd" % (p["x"], p["y"]) for p in drive["plan"]["pieces"]] + ["index.xml"])
    for p in drive["plan"]["pieces"]:
        assert (other / ("piece_%d_%d.pcd" % (p["x"], p["y"]))).read_bytes() == (out / ref.piece_file("part_", p["x"], p["y"])).read_bytes()
    bad = tmp_path / "bad"
    bad.mkdir()
    r = _run(["--scans", drive["seq"], "--map-poses", drive["pose_file"], "--map-package", str(bad), "--submap-frames", str(SUBMAP_FRAMES),
              "--package-piece-width", "8", "--package-border-offset", "-30"], rc=2)
    assert "No good bounding box" in r.stderr and os.listdir(bad) == []
    r = _run(["--scans", drive["seq"], "--map-poses", drive["pose_file"], "--map-package", str(tmp_path / "missing")] + flags, rc=2)
    assert "cannot write" in r.stderr and not (tmp_path / "missing").exists()      # a missing directory: refused before any device work


@pytest.mark.gpu
def test_align_and_package(drive, tmp_path):
    common = ["--scans", drive["seq"], "--gpus", "1", "--batch", "4", "--iterations", "20", "--guess-tx", "0.8"]
    flags = ["--submap-frames", str(SUBMAP_FRAMES), "--package-piece-width", str(PIECE_WIDTH), "--package-border-offset", str(BORDER_OFFSET)]
    p0, p1 = tmp_path / "p0.txt", tmp_path / "p1.txt"
    d1, d2 = tmp_path / "d1", tmp_path / "d2"
    d1.mkdir(); d2.mkdir()
    r0 = _run(common + ["--out", str(p0)])
    r1 = _run(common + ["--out", str(p1), "--map-package", str(d1)] + flags)
    line0 = json.loads(r0.stdout.strip().splitlines()[-1])
    line1 = json.loads(r1.stdout.strip().splitlines()[-1])
    assert list(line0) == TODAY_KEYS                              # without --map-package: exactly today's line
    assert list(line1) == TODAY_KEYS + PACKAGE_KEYS
    assert p0.read_bytes() == p1.read_bytes()                     # the package leaves the poses alone
    assert line1["package_submaps"] == 4 and line1["package_pieces"] >= 3
    # the package is a function of the pose file as written: a package-only run on it gives the same bytes
    _run(["--scans", drive["seq"], "--map-poses", str(p1), "--map-package", str(d2)] + flags)
    names = sorted(os.listdir(d1))
    assert names == sorted(os.listdir(d2)) and "map_package.xml" in names and len(names) == line1["package_pieces"] + 1
    for name in names:
        assert (d1 / name).read_bytes() == (d2 / name).read_bytes(), name
