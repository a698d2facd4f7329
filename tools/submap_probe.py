"""Time of one full-size submap, cloud and target: 5 x 120 000-point scans of the straight drive at voxel 0.1.

  --mode new     smhip_submap_build_f32 + smhip_filter_output_to_target: the frames' raw rows go up once, everything else
                 happens on the device
  --mode parent  what had to be composed before those entries existed: TransformPoint on the host (numpy float32, the
                 restatement of tests/test_transform_point.py) -> smhip_filter_chain_f32([VoxelGrid]) -> smhip_filter_get_output
                 -> smhip_prepare_target_f32 on the downloaded rows.  --lib PATH runs it on another build of libsmhip.so (the
                 parent commit's); only entries that build has are bound
  --mode both    each of the two in a fresh child process (--parent-lib PATH for the second), medians side by side and their
                 ratio
Both modes end with the same target in slot 0 (tests/test_submap_gpu.py checks that bit for bit).  Median of --repeats calls after
--warmup calls.  --kernel-stats CSV adds the share of submap_transform_keys in the kernel time of a `rocprofv3 --kernel-trace
--stats` run of `--mode new` (a run of its own).  One JSON line on stdout (and in --out when given)."""
import argparse
import ctypes
import csv
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_FRAMES, N_POINTS, VOXEL = 5, 120_000, 0.1


def bind(path, names):
    from staticmapping_amd import _capi
    lib = ctypes.CDLL(path)
    for name in names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _capi.SIGNATURES[name]
    return lib


def frames_and_poses():
    from staticmapping_amd import synth
    scene = synth.make_scene(0)
    poses = [synth.make_pose(t=(0.8 * k, 0.03 * k, 0.0), rpy_deg=(0, 0, 0.6 * k)) for k in range(N_FRAMES)]
    scans = [np.ascontiguousarray(synth.velodyne_scan(scene, P, seed=90 + k, n_points=N_POINTS)) for k, P in enumerate(poses)]
    first = np.linalg.inv(poses[0])
    return scans, [np.eye(4)] + [first @ P for P in poses[1:]]


def run(a):
    try:
        import torch  # noqa: F401   (one HIP runtime per process: torch's first, as in tests/conftest.py)
    except ImportError:
        pass
    from staticmapping_amd import _capi, build
    from staticmapping_amd.submap import text_voxel_size
    from oracle import filters as of
    from test_transform_point import transform_point_f32
    scans, local = frames_and_poses()
    size = text_voxel_size(VOXEL)
    fp, ip = _capi.c_float_p, _capi.c_int32_p
    names = ["smhip_create", "smhip_destroy", "smhip_last_error", "smhip_filter_default", "smhip_filter_chain_f32", "smhip_filter_get_output",
             "smhip_prepare_target_f32"] + (["smhip_submap_build_f32", "smhip_filter_output_to_target"] if a.mode == "new" else [])
    lib = bind(a.lib or build.LIB_PATH, names)
    h = ctypes.c_void_p()
    if lib.smhip_create(0, None, 1, 131072, 1 << 20, ctypes.byref(h)) != 0:
        raise SystemExit("smhip_create failed: no gfx950 device?")

    def ok(st):
        if st != 0:
            raise SystemExit(lib.smhip_last_error(h).decode())

    split = {}
    if a.mode == "new":
        rows = (fp * N_FRAMES)(*[s.ctypes.data_as(fp) for s in scans])
        n = np.array([len(s) for s in scans], np.int32)
        poses = np.ascontiguousarray([P.T.reshape(16) for P in local]).reshape(-1)
        n_cloud, n_target = ctypes.c_int(), ctypes.c_int()

        def once():
            t0 = time.perf_counter()
            ok(lib.smhip_submap_build_f32(h, N_FRAMES, rows, 4, n.ctypes.data_as(ip), poses.ctypes.data_as(_capi.c_double_p), size,
                                          ctypes.byref(n_cloud)))
            t1 = time.perf_counter()
            ok(lib.smhip_filter_output_to_target(h, 0, ctypes.byref(n_target)))
            t2 = time.perf_counter()
            return {"build": t1 - t0, "to_target": t2 - t1, "total": t2 - t0}
    else:
        desc = _capi.FilterDesc()
        lib.smhip_filter_default(4, ctypes.byref(desc))                       # SMHIP_FILTER_VOXEL_GRID
        desc.p[0] = size
        n_cloud, n_target = ctypes.c_int(), ctypes.c_int32()

        def once():
            t0 = time.perf_counter()
            parts = []
            for s, P in zip(scans, local):                                      # 1. the host transform
                r5 = of.with_factor(s)
                r5[:, :3] = transform_point_f32(r5, P)
                parts.append(r5)
            rows5 = np.ascontiguousarray(np.concatenate(parts))
            t1 = time.perf_counter()
            ok(lib.smhip_filter_chain_f32(h, rows5.ctypes.data_as(fp), 5, len(rows5), ctypes.byref(desc), 1, ctypes.byref(n_cloud)))   # 2.
            t2 = time.perf_counter()
            out = np.empty((n_cloud.value, 5), np.float32)
            ok(lib.smhip_filter_get_output(h, out.ctypes.data_as(fp), None, n_cloud.value))                                          # 3.
            t3 = time.perf_counter()
            ok(lib.smhip_prepare_target_f32(h, 0, out.ctypes.data_as(fp), 5, n_cloud.value, ctypes.byref(n_target)))                 # 4.
            t4 = time.perf_counter()
            return {"host_transform": t1 - t0, "filter_chain": t2 - t1, "get_output": t3 - t2, "prepare_target": t4 - t3, "total": t4 - t0}

    for _ in range(a.warmup):
        once()
    runs = [once() for _ in range(a.repeats)]
    for k in runs[0]:
        split[k + "_ms"] = round(float(np.median([r[k] for r in runs])) * 1e3, 4)
    lib.smhip_destroy(h)
    return {"mode": a.mode, "library": os.path.relpath(a.lib or build.LIB_PATH, ROOT), "frames": N_FRAMES, "points_per_frame": N_POINTS,
            "voxel_size": size, "repeats": a.repeats, "warmup": a.warmup, "cloud_points": n_cloud.value, "target_points": n_target.value,
            "median_ms": split.pop("total_ms"), "split_median_ms": split}


def kernel_share(path):
    """share of submap_transform_keys in the summed kernel time of a rocprofv3 kernel_stats.csv"""
    total = ours = 0.0
    calls = 0
    with open(path) as f:
        for row in csv.DictReader(f):
            t = float(row["TotalDurationNs"]) if "TotalDurationNs" in row else float(row["TotalDurationUs"]) * 1e3
            total += t
            if "submap_transform_keys" in row["Name"]:
                ours += t
                calls += int(row["Calls"])
    return {"kernel": "submap_transform_keys", "calls": calls, "total_us": round(ours / 1e3, 3), "mean_us": round(ours / 1e3 / max(calls, 1), 3),
            "share_of_kernel_time": round(ours / total, 5) if total else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("new", "parent", "both"), default="both")
    ap.add_argument("--lib", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.mode == "both":
        res = {}
        for mode, lib in (("new", ""), ("parent", a.parent_lib)):
            cmd = [sys.executable, os.path.abspath(__file__), "--mode", mode, "--repeats", str(a.repeats), "--warmup", str(a.warmup)] + (["--lib", lib] if lib else [])
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                raise SystemExit(f"{' '.join(cmd)} ended with {p.returncode}: {p.stderr[-2000:]}")
            res[mode] = json.loads(p.stdout.strip().splitlines()[-1])
        res["new_over_parent"] = round(res["new"]["median_ms"] / res["parent"]["median_ms"], 4)
        res["new_over_parent_without_host_transform"] = round(
            res["new"]["median_ms"] / (res["parent"]["median_ms"] - res["parent"]["split_median_ms"]["host_transform_ms"]), 4)
    else:
        res = run(a)
    if a.kernel_stats:
        res["kernel_trace"] = kernel_share(a.kernel_stats)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
