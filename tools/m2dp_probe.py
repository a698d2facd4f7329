"""Time of one M2DP descriptor on a full-size submap: 5 x 120 000-point scans of the straight drive at voxel 0.1, built on the
device (smhip_submap_build_f32) and left resident.

  resident   smhip_m2dp_from_filter_output on the resident cloud (no upload)
  uploaded   smhip_m2dp_f32 on the same rows handed over from host memory (staging, upload, the same kernels)
Median of --repeats calls after --warmup calls, a host clock around calls that end in a synchronise.  Beside them, as context only,
the numpy restatement's time for the same cloud (tests/m2dp_ref.py, one call).  --calls-only N: N resident calls and nothing else
(the run that `rocprofv3 --kernel-trace --stats` wraps); --kernel-stats CSV adds each m2dp kernel's mean time from such a run.
One JSON line on stdout (and in --out when given)."""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_FRAMES, N_POINTS, VOXEL = 5, 120_000, 0.1


def kernel_times(path):
    """mean time per launch of every m2dp kernel in a rocprofv3 kernel_stats.csv"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            if "m2dp_" not in row["Name"]:
                continue
            t = float(row["TotalDurationNs"]) if "TotalDurationNs" in row else float(row["TotalDurationUs"]) * 1e3
            name = re.search(r"m2dp_[a-z]+", row["Name"]).group(0)      # kernel names are m2dp_ + lower-case letters, mangled or not
            out[name] = {"calls": int(row["Calls"]), "mean_us": round(t / 1e3 / max(int(row["Calls"]), 1), 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls-only", type=int, default=0)
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--no-restatement", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    try:
        import torch  # noqa: F401   (one HIP runtime per process: torch's first, as in tests/conftest.py)
    except ImportError:
        pass
    import staticmapping_amd as sm
    from staticmapping_amd import m2dp as dm
    from staticmapping_amd import submap as dsub
    from staticmapping_amd import synth
    scene = synth.make_scene(0)
    poses = [synth.make_pose(t=(0.8 * k, 0.03 * k, 0.0), rpy_deg=(0, 0, 0.6 * k)) for k in range(N_FRAMES)]
    scans = [np.ascontiguousarray(synth.velodyne_scan(scene, P, seed=90 + k, n_points=N_POINTS)) for k, P in enumerate(poses)]
    first = np.linalg.inv(poses[0])
    local = [np.eye(4)] + [first @ P for P in poses[1:]]
    m = sm.IcpFastHip(pair_slots=1, max_source_points=131072, max_target_points=1 << 20)
    n = dsub.build_submap_resident(m, scans, local, dsub.text_voxel_size(VOXEL))
    opts = dm.make_options()
    if a.calls_only:
        for _ in range(a.calls_only):
            dm.m2dp_from_filter_output(m, opts)
        print(json.dumps({"resident_calls": a.calls_only, "cloud_points": n}))
        return
    rows, _ = dsub.get_submap(m, n)

    def median_ms(call):
        for _ in range(a.warmup):
            call()
        t = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            call()
            t.append(time.perf_counter() - t0)
        return round(float(np.median(t)) * 1e3, 4)

    res = {"frames": N_FRAMES, "points_per_frame": N_POINTS, "voxel_size": dsub.text_voxel_size(VOXEL), "cloud_points": n, "repeats": a.repeats,
           "warmup": a.warmup, "descriptor_length": dm.length(opts),
           "resident_median_ms": median_ms(lambda: dm.m2dp_from_filter_output(m, opts)),
           "uploaded_median_ms": median_ms(lambda: dm.m2dp(m, rows, opts))}
    _, kept, _, n_kept = dm.last(m, n, opts)
    res["kept_rows"] = n_kept
    if not a.no_restatement:
        import m2dp_ref as mr
        t0 = time.perf_counter()
        ref = mr.m2dp(rows)
        res["numpy_restatement_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["score_device_vs_restatement"] = round(mr.match(dm.m2dp_from_filter_output(m, opts), ref["descriptor"]), 9)
    if a.kernel_stats:
        res["kernel_trace"] = kernel_times(a.kernel_stats)
    m.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
