"""What the map package costs on the device, and what the clipped insert and output save a caller.

The workload is the bench's `end_to_end` drive (1 025 scans of 120 000 points, 8 m/s, 10 Hz, seed 5) under its true poses, grouped
into submaps of 5 frames built on the device at 0.1 m, packaged with the reference's default options (border_offset 100,
piece_width 500) and MrvmSettings.  Two ways to the same files are timed, median of --repeats after --warmup:

  package      staticmapping_amd.map_package.save_map_package: smhip_mrvm_insert_transformed[_clipped]_f32, smhip_mrvm_output_clipped,
               smhip_mrvm_clear -- one handle for all pieces
  composition  what a caller needs without those three calls: numpy float32 TransformPoint and clip on the host,
               smhip_mrvm_insert_f32, smhip_mrvm_output_ex (SORTED), numpy clip and recentre, a new map per piece

Both must write the same bytes; the probe checks that before it reports.  Writes profiles/map_package_probe.json.
`--calls-only N` runs the package N times and nothing else: the run to wrap in `rocprofv3 --kernel-trace --stats` for the share of
mrvm_clip_flags / mrvm_transform_kept / mrvm_row_counts_clipped / mrvm_sorted_rows_clipped.

Usage: python tools/map_package_probe.py [--scans 1025] [--points 120000] [--piece-width 500] [--border-offset 100] [--repeats 5] [--warmup 1]
       [--calls-only N] [--out FILE]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

try:
    import torch  # noqa: F401  (one HIP runtime per process: PyTorch's first, see staticmapping_amd/_capi.py)
except ImportError:
    pass
import numpy as np  # noqa: E402


def transform_rows(rows5, pose, scale):
    """TransformPoint in float32 numpy (builder/data/cloud_types.cc:167-178): every product and sum rounded to float."""
    m = np.asarray(pose, np.float64).astype(np.float32)
    x, y, z = rows5[:, 0], rows5[:, 1], rows5[:, 2]
    out = np.empty((len(rows5), 5), np.float32)
    for i in range(3):
        out[:, i] = ((m[i, 0] * x + m[i, 1] * y) + m[i, 2] * z) + m[i, 3]
    out[:, 3] = rows5[:, 3] * np.float32(scale)
    out[:, 4] = rows5[:, 4]
    return out


def in_box(rows, lo, hi):
    x, y = rows[:, 0].astype(np.float64), rows[:, 1].astype(np.float64)
    return (x >= lo[0]) & (x <= hi[0]) & (y >= lo[1]) & (y <= hi[1])


def composition(submaps, directory, options, scale, max_cloud):
    import staticmapping_amd as sm
    from staticmapping_amd import map_package as mp, pcd
    pl = mp.plan(np.array([P[:3, 3] for P, _ in submaps]), options)
    for i in range(len(pl.centres)):
        x, y = divmod(i, pl.y_steps)
        lo, hi, c = pl.bb_min[i], pl.bb_max[i], pl.centres[i]
        m = sm.MultiResolutionVoxelMapHip(table_log2=22, max_cloud_points=max_cloud)
        for k in pl.members[i]:
            P, cloud = submaps[k]
            world = transform_rows(cloud, P, scale)
            if not (lo[0] <= P[0, 3] <= hi[0] and lo[1] <= P[1, 3] <= hi[1]):
                world = world[in_box(world, lo, hi)]
            if len(world):
                m.insert_point_cloud(world, P[:3, 3].astype(np.float32))
        rows = m.output_to_point_cloud(sorted=True)
        m.close()
        rows = rows[in_box(rows, lo, hi)]
        rows[:, 0] = (rows[:, 0].astype(np.float64) - c[0]).astype(np.float32)
        rows[:, 1] = (rows[:, 1].astype(np.float64) - c[1]).astype(np.float32)
        with open(os.path.join(directory, mp.piece_file(options, x, y)), "wb") as f:
            f.write(pcd.header(len(rows)))
            f.write(rows.tobytes())
    mp.write_xml(os.path.join(directory, options.descript_filename), pl, options)
    return pl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1025)
    ap.add_argument("--points", type=int, default=120_000)
    ap.add_argument("--submap-frames", type=int, default=5)
    ap.add_argument("--piece-width", type=float, default=500.0)
    ap.add_argument("--border-offset", type=float, default=100.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls-only", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_package_probe.json"))
    a = ap.parse_args()
    import staticmapping_amd as sm
    from staticmapping_amd import map_package as mp, submap, synth

    poses = synth.drive_poses(a.scans, seed=5, speed=8.0, hz=10.0, yaw_rate_max=0.2)
    scene = synth.make_drive_scene(poses, seed=5)
    base = np.linalg.inv(poses[0])
    N, S = a.submap_frames, a.scans // a.submap_frames
    matcher = sm.IcpFastHip(device=0, max_source_points=N * a.points, max_target_points=N * a.points)
    voxel = submap.text_voxel_size(0.1)
    submaps = []
    t = time.perf_counter()
    for k in range(S):                                            # scans are generated a submap at a time and dropped: only the clouds are kept
        frames = [synth.velodyne_scan(synth.scene_near(scene, poses[f][:3, 3]), poses[f], seed=1000 + f, n_points=a.points)[:, :4] for f in range(k * N, (k + 1) * N)]
        G = [base @ poses[f] for f in range(k * N, (k + 1) * N)]
        local = [np.eye(4)] + [np.linalg.inv(G[0]) @ P for P in G[1:]]
        submaps.append((G[0], sm.build_submap(matcher, frames, local, voxel)[0]))
    matcher.close()
    prepare_s = time.perf_counter() - t
    max_cloud = max(len(c) for _, c in submaps)
    options = mp.MapPackageOptions(piece_width=a.piece_width, border_offset=a.border_offset)
    root = tempfile.mkdtemp(prefix="smhip_map_package_probe_")
    try:
        def run(fn, tag, n):
            times = []
            for rep in range(n):
                d = os.path.join(root, "%s_%d" % (tag, rep))
                os.makedirs(d)
                t0 = time.perf_counter()
                fn(d)
                times.append(time.perf_counter() - t0)
                if rep + 1 < n:
                    shutil.rmtree(d)
            return times, d

        package = lambda d: mp.save_map_package(submaps, d + os.sep, options, intensity_scale=255.0)     # noqa: E731
        if a.calls_only:
            run(package, "calls", a.calls_only)
            return
        tp, dp = run(package, "package", a.warmup + a.repeats)
        tc, dc = run(lambda d: composition(submaps, d, options, 255.0, max_cloud), "composition", a.warmup + a.repeats)
        names = sorted(os.listdir(dp))
        same = names == sorted(os.listdir(dc)) and all(open(os.path.join(dp, n), "rb").read() == open(os.path.join(dc, n), "rb").read() for n in names)
        pl = mp.plan(np.array([P[:3, 3] for P, _ in submaps]), options)
        out = {"workload": f"{a.scans}-scan synthetic drive (8 m/s, 10 Hz, seed 5; {a.points} points per scan), true poses, {S} submaps of {N} frames at 0.1 m, "
                           f"piece_width {a.piece_width:g}, border_offset {a.border_offset:g}, default MrvmSettings", "submaps": S, "submap_points_max": int(max_cloud), "pieces": len(pl.centres),
               "inserts": int(sum(len(m) for m in pl.members)), "prepare_submaps_s": round(prepare_s, 2),
               "package_s": {"median": statistics.median(tp[a.warmup:]), "all": tp}, "composition_s": {"median": statistics.median(tc[a.warmup:]), "all": tc},
               "composition_over_package": statistics.median(tc[a.warmup:]) / statistics.median(tp[a.warmup:]), "same_bytes": bool(same),
               "repeats": a.repeats, "warmup": a.warmup}
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out))
        if not same:
            sys.exit("the two paths wrote different files")
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
