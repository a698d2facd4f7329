"""Time of one frame's way into the static map, with and without motion compensation: a 120 000-point scan of the seed-5 synthetic
drive (8 m/s, 10 Hz), skewed by the motion to the next pose, inserted into a map that holds the drive's first frame.

  plain         smhip_mrvm_insert_transformed_f32: no compensation (what --map does without --map-compensate)
  compensated   smhip_mrvm_insert_compensated_f32: de-skew and TransformPoint in one kernel, the factor flag read before the table is
                touched (one stream synchronise more than the plain insert)
  composition   what a caller had to compose before that entry existed: the rows through an unfiltered chain,
                smhip_filter_output_to_source_compensated with the rows downloaded, the plain insert of the stride-5 rows

Before every timed call the map is cleared and the first frame inserted again (not timed), so every call meets the same map; the
three take turns.  A host clock around calls that end in a synchronise; the median of --repeats calls after --warmup calls.
--kernel-stats CSV adds the transform kernels' own time from a `rocprofv3 --kernel-trace --stats` run of this tool (a run of its
own).  One JSON line on stdout (and in --out when given)."""
import argparse
import csv
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_POINTS, SEED = 120_000, 5


def frames():
    """(frame 0 unskewed, frame 1 skewed by its sweep motion, their poses, frame 1's motion)"""
    from staticmapping_amd import synth
    import map_compensation_ref as ref
    poses = np.asarray(synth.drive_poses(3, seed=SEED, speed=8.0, hz=10.0, yaw_rate_max=0.2))
    scene = synth.make_drive_scene(poses, seed=SEED)
    scans = [synth.velodyne_scan(synth.scene_near(scene, P[:3, 3]), P, seed=1000 + k, n_points=N_POINTS)[:, :4] for k, P in enumerate(poses[:2])]
    motions = ref.sweep_motions(poses)
    return np.ascontiguousarray(scans[0], np.float32), np.ascontiguousarray(ref.skew(scans[1], motions[1]), np.float32), poses, motions[1]


def kernel_times(path):
    """the transform kernels' mean time in a rocprofv3 kernel_stats.csv"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row["Name"].replace("(anonymous namespace)::", "").split("(")[0].split("::")[-1].replace("void ", "").strip()
            if name in ("mrvm_transform_comp", "mrvm_transform", "filt_motion_comp", "mrvm_hit", "mrvm_miss"):
                t = float(row["TotalDurationNs"]) if "TotalDurationNs" in row else float(row["TotalDurationUs"]) * 1e3
                out[name] = {"calls": int(row["Calls"]), "mean_us": round(t / 1e3 / max(int(row["Calls"]), 1), 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    try:
        import torch  # noqa: F401   (one HIP runtime per process: torch's first, as in tests/conftest.py)
    except ImportError:
        pass
    from staticmapping_amd import _capi
    lib = _capi.load_library()
    first, rows, poses, motion = frames()
    n = len(rows)
    fp, dp = _capi.c_float_p, _capi.c_double_p
    cm = [np.ascontiguousarray(P.T).ravel() for P in poses]
    mm = np.ascontiguousarray(motion.T).ravel()
    settings = _capi.MrvmSettings()
    lib.smhip_mrvm_default_settings(ctypes.byref(settings))
    m, h = ctypes.c_void_p(), ctypes.c_void_p()
    if lib.smhip_mrvm_create(0, 22, N_POINTS, ctypes.byref(settings), ctypes.byref(m)) != 0 or lib.smhip_create(0, None, 1, 131072, 131072, ctypes.byref(h)) != 0:
        raise SystemExit("no gfx950 device: nothing is measured without one")

    def ok(st, what):
        if st != 0:
            raise SystemExit("%s: %s / %s" % (what, lib.smhip_mrvm_last_error(m).decode(), lib.smhip_last_error(h).decode()))

    rows5 = np.empty((n, 5), np.float32)
    n_out = ctypes.c_int()

    def plain():
        ok(lib.smhip_mrvm_insert_transformed_f32(m, rows.ctypes.data_as(fp), 4, n, cm[1].ctypes.data_as(dp), 255.0), "plain")

    def compensated():
        ok(lib.smhip_mrvm_insert_compensated_f32(m, rows.ctypes.data_as(fp), 4, n, cm[1].ctypes.data_as(dp), mm.ctypes.data_as(dp), 255.0), "compensated")

    def composition():
        ok(lib.smhip_filter_chain_f32(h, rows.ctypes.data_as(fp), 4, n, None, 0, ctypes.byref(n_out)), "chain")
        ok(lib.smhip_filter_output_to_source_compensated(h, 0, mm.ctypes.data_as(dp), rows5.ctypes.data_as(fp)), "de-skew")
        ok(lib.smhip_mrvm_insert_transformed_f32(m, rows5.ctypes.data_as(fp), 5, n, cm[1].ctypes.data_as(dp), 255.0), "insert")

    calls = {"plain": plain, "compensated": compensated, "composition": composition}
    times = {k: [] for k in calls}
    voxels = {}
    for rep in range(a.warmup + a.repeats):
        for name, fn in calls.items():
            ok(lib.smhip_mrvm_clear(m), "clear")
            ok(lib.smhip_mrvm_insert_transformed_f32(m, first.ctypes.data_as(fp), 4, len(first), cm[0].ctypes.data_as(dp), 255.0), "first frame")
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if rep >= a.warmup:
                times[name].append(dt)
            v = ctypes.c_int32()
            lib.smhip_mrvm_voxel_count(m, ctypes.byref(v))
            voxels[name] = v.value
    lib.smhip_mrvm_destroy(m)
    lib.smhip_destroy(h)
    med = {k: round(float(np.median(v)) * 1e3, 4) for k, v in times.items()}
    res = {"points": n, "repeats": a.repeats, "warmup": a.warmup, "median_ms": med,
           "p10_p90_ms": {k: [round(float(np.percentile(v, 10)) * 1e3, 4), round(float(np.percentile(v, 90)) * 1e3, 4)] for k, v in times.items()},
           "compensated_minus_plain_ms": round(med["compensated"] - med["plain"], 4),
           "compensated_over_composition": round(med["compensated"] / med["composition"], 4), "voxels_after": voxels}
    if a.kernel_stats:
        res["kernel_trace"] = kernel_times(a.kernel_stats)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
