"""Device time of GroundRemoval, GroundRemoval2, RangeImage and StatisticRemoval (defaults and point_num_meank = 10) on one
120 000-point scan of the seed-5 drive, beside the CPU restatement's (tests/ground_filters_ref.py; for StatisticRemoval, with
--statistic-cpu, tests/statistic_removal_ref.py -- brute force, about a minute -- and a scipy k-d tree query).

Each call of smhip_filter_chain_ex_f32 stages the rows on the host, uploads them and runs the chain; the empty chain measures
the staging and upload alone, and `filter_ms` is a chain's median minus the empty chain's median.  Medians over --repeats calls
after --warmup calls.  One JSON line on stdout (and in --out when given)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-repeats", type=int, default=1)
    ap.add_argument("--statistic-cpu", action="store_true", help="also time StatisticRemoval's restatement and scipy's cKDTree")
    ap.add_argument("--cpu-only", action="store_true", help="skip the device: the CPU times alone (no GPU needed)")
    ap.add_argument("--only-statistic", action="store_true", help="the empty chain and the StatisticRemoval cases alone")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    try:
        import torch  # noqa: F401   (one HIP runtime per process: torch's first, as in tests/conftest.py)
    except ImportError:
        pass
    import ground_filters_ref as gf
    import staticmapping_amd as sm
    from staticmapping_amd import filters as df, synth
    from oracle import filters as of

    poses = synth.drive_poses(3, seed=5, speed=8.0, speed_spread=2.0, yaw_rate_max=0.2, segment_s=1.0)
    scene = synth.make_drive_scene(poses, seed=5)
    scan = np.ascontiguousarray(synth.velodyne_scan(synth.scene_near(scene, poses[1][:3, 3]), poses[1], seed=500, n_points=120_000))
    kitti_pre = dict(r_min=0.1, start_ground_height=-1.5, long_line_threshold=10, max_slope=0.12, max_error=0.1,
                     max_dist_to_line=0.10, max_start_height=0.6)
    kitti_inner = dict(kitti_pre, start_ground_height=-0.35)
    image60 = dict(top_angle=30.0, btm_angle=-20.0, vertical_line_num=60)
    cases = {
        "empty_chain": [],
        "GroundRemoval": [df.make_filter("GroundRemoval")],
        "GroundRemoval2_defaults": [df.make_filter("GroundRemoval2")],
        "GroundRemoval2_kitti_pre": [df.make_filter("GroundRemoval2", **kitti_pre)],
        "GroundRemoval2_kitti_inner": [df.make_filter("GroundRemoval2", **kitti_inner)],
        "RangeImage_40x1800": [df.make_filter("RangeImage")],
        "RangeImage_60x1800": [df.make_filter("RangeImage", **image60)],
        "kitti_inner_chain": [df.make_filter("GroundRemoval2", **kitti_inner), df.make_filter("RangeImage", **image60)],
        "kitti_pre_chain": [df.make_filter("Range", min_range=5.0), df.make_filter("AxisRange", min=-2.0),
                            df.make_filter("GroundRemoval2", **kitti_pre), df.make_filter("RandomSampler", sampling_rate=0.5, seed=1)],
        "StatisticRemoval_defaults": [df.make_filter("StatisticRemoval")],
        "StatisticRemoval_k10": [df.make_filter("StatisticRemoval", point_num_meank=10)],
    }
    if a.only_statistic:
        cases = {k: v for k, v in cases.items() if k == "empty_chain" or k.startswith("StatisticRemoval")}
    m = None if a.cpu_only else sm.IcpFastHip(pair_slots=1, max_source_points=131072, max_target_points=131072)
    res = {"n_points": len(scan), "repeats": a.repeats, "device_ms": {}, "filter_ms": {}, "kept": {}, "cpu_ms": {}}
    for name, chain in ({} if a.cpu_only else cases).items():
        # widen even the empty chain so every case goes through smhip_filter_chain_ex_f32
        chain_ex = [df.widen(d) for d in chain] if chain else [df.make_filter("Range")]
        for _ in range(a.warmup):
            df.run_chain_resident(m, scan, chain_ex)
        t = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            k = df.run_chain_resident(m, scan, chain_ex)
            t.append((time.perf_counter() - t0) * 1e3)
        res["device_ms"][name] = float(np.median(t))
        res["kept"][name] = int(k)
    base = res["device_ms"].get("empty_chain")
    for name in cases:
        if name != "empty_chain" and not a.cpu_only:
            res["filter_ms"][name] = round(res["device_ms"][name] - base, 4)
    rows5 = of.with_factor(scan)
    cpu = [] if a.only_statistic else [("GroundRemoval", lambda: gf.ground_removal(rows5)),
                                       ("GroundRemoval2_kitti_pre", lambda: gf.ground_removal2(rows5, **kitti_pre)),
                                       ("RangeImage_40x1800", lambda: gf.range_image(rows5))]
    if a.statistic_cpu:
        import statistic_removal_ref as sr
        from scipy.spatial import cKDTree
        xyz = rows5[:, :3].astype(np.float64)
        cpu += [("StatisticRemoval_defaults", lambda: sr.statistic_removal(rows5)),
                ("StatisticRemoval_defaults_scipy_ckdtree_query", lambda: cKDTree(xyz).query(xyz, k=31))]
    for name, fn in cpu:
        t = []
        for _ in range(a.cpu_repeats):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        res["cpu_ms"][name + ("" if "scipy" in name else "_restatement")] = float(np.median(t))
    if m is not None:
        m.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
