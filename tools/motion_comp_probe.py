"""Time of one motion compensation of a 120 000-point scan (seed 5 of the synthetic drive) into a source slot.

  --mode new     one smhip_filter_output_to_source_compensated on the scan already resident in the filter workspace (the rows go up
                 once per scan, smhip_filter_chain_f32 with no filter, timed separately as `upload_ms`); also with points5_out, the
                 form of the front end's second pass
  --mode parent  what a caller of a library without that entry composes for the same source: the header's host MotionCompensation
                 (include/smhip/front_end.h, tools/motion_comp_host.cc compiled with g++ -O2, timed in a process of its own) plus
                 smhip_set_source_f32 of the compensated rows.  --lib PATH runs the upload on another build of libsmhip.so (the
                 parent commit's)
  --mode both    each of the two in a fresh child process (--parent-lib PATH for the second), medians side by side and their ratio
A host clock around calls that end in a synchronise; the median of --repeats calls after --warmup calls.  --kernel-stats CSV adds
filt_motion_comp's own time from a `rocprofv3 --kernel-trace --stats` run of `--mode new` (a run of its own).  One JSON line on
stdout (and in --out when given)."""
import argparse
import csv
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_POINTS, SEED = 120_000, 5


def bind(path, names):
    from staticmapping_amd import _capi
    lib = ctypes.CDLL(path)
    for name in names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _capi.SIGNATURES[name]
    return lib


def scan_and_delta():
    from staticmapping_amd import synth
    import motion_comp_ref as mc
    rows4 = synth.velodyne_scan(synth.make_scene(0), synth.make_pose(t=(0.3 * SEED, 0.01 * SEED, 0.0), rpy_deg=(0, 0, 0.4 * SEED)), seed=SEED,
                                n_points=N_POINTS)
    rows = np.zeros((len(rows4), 5), np.float32)
    rows[:, :4] = rows4[:, :4]
    rows[:, 4] = (np.arange(len(rows), dtype=np.float64) / len(rows)).astype(np.float32)
    return np.ascontiguousarray(rows), mc.check_deltas()["drive"]


def host_exe():
    from staticmapping_amd import build
    lib = build.build()
    exe = os.path.join(ROOT, "tools", "_build", "motion_comp_host")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(ROOT, "tools", "motion_comp_host.cc")
    hdr = os.path.join(ROOT, "include", "smhip", "front_end.h")
    if not os.path.exists(exe) or max(os.path.getmtime(src), os.path.getmtime(hdr)) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", os.path.dirname(lib), "-lsmhip",
                               "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def median_ms(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return round(float(np.median(t)) * 1e3, 4)


def run(a):
    try:
        import torch  # noqa: F401   (one HIP runtime per process: torch's first, as in tests/conftest.py)
    except ImportError:
        pass
    from staticmapping_amd import _capi, build
    import motion_comp_ref as mc
    rows, delta = scan_and_delta()
    fp, dp = _capi.c_float_p, _capi.c_double_p
    names = ["smhip_create", "smhip_destroy", "smhip_last_error", "smhip_set_source_f32", "smhip_filter_chain_f32"]
    if a.mode == "new":
        names.append("smhip_filter_output_to_source_compensated")
    lib = bind(a.lib or build.LIB_PATH, names)
    h = ctypes.c_void_p()
    if lib.smhip_create(0, None, 1, 131072, 131072, ctypes.byref(h)) != 0:
        raise SystemExit("smhip_create failed: no gfx950 device?")

    def ok(st):
        if st != 0:
            raise SystemExit(lib.smhip_last_error(h).decode())

    res = {"mode": a.mode, "library": os.path.relpath(a.lib or build.LIB_PATH, ROOT), "points": len(rows), "repeats": a.repeats, "warmup": a.warmup}
    if a.mode == "new":
        d = np.ascontiguousarray(delta.T)
        n_out = ctypes.c_int()
        out = np.empty_like(rows)
        res["upload_ms"] = median_ms(lambda: ok(lib.smhip_filter_chain_f32(h, rows.ctypes.data_as(fp), 5, len(rows), None, 0, ctypes.byref(n_out))),
                                     a.repeats, a.warmup)
        res["median_ms"] = median_ms(lambda: ok(lib.smhip_filter_output_to_source_compensated(h, 0, d.ctypes.data_as(dp), None)), a.repeats, a.warmup)
        res["with_points5_out_ms"] = median_ms(lambda: ok(lib.smhip_filter_output_to_source_compensated(h, 0, d.ctypes.data_as(dp), out.ctypes.data_as(fp))),
                                               a.repeats, a.warmup)
    else:
        comp = np.ascontiguousarray(mc.motion_compensation(rows, delta))
        with tempfile.TemporaryDirectory() as tmp:
            rows.tofile(os.path.join(tmp, "rows.bin"))
            np.ascontiguousarray(delta.T).tofile(os.path.join(tmp, "delta.bin"))
            host = json.loads(subprocess.check_output([host_exe(), os.path.join(tmp, "rows.bin"), os.path.join(tmp, "delta.bin"), str(a.repeats), str(a.warmup)],
                                                      text=True, timeout=600).strip().splitlines()[-1])
        res["host_motion_compensation_ms"] = host["median_ms"]
        res["set_source_ms"] = median_ms(lambda: ok(lib.smhip_set_source_f32(h, 0, comp.ctypes.data_as(fp), 5, len(comp))), a.repeats, a.warmup)
        res["median_ms"] = round(res["host_motion_compensation_ms"] + res["set_source_ms"], 4)
    lib.smhip_destroy(h)
    return res


def kernel_time(path):
    """filt_motion_comp and the rest of a call (the Morton ordering's kernels) in a rocprofv3 kernel_stats.csv"""
    rows = []
    with open(path) as f:
        for row in csv.DictReader(f):
            t = float(row["TotalDurationNs"]) if "TotalDurationNs" in row else float(row["TotalDurationUs"]) * 1e3
            rows.append((row["Name"], int(row["Calls"]), t))
    ours = [r for r in rows if "filt_motion_comp" in r[0]]
    calls = sum(r[1] for r in ours)
    t_ours = sum(r[2] for r in ours)
    total = sum(r[2] for r in rows)
    return {"kernel": "filt_motion_comp", "calls": calls, "mean_us": round(t_ours / 1e3 / max(calls, 1), 3),
            "share_of_kernel_time": round(t_ours / total, 5) if total else None,
            "other_kernels_us_per_call": round((total - t_ours) / 1e3 / max(calls, 1), 3)}


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
        res["new_over_parent_set_source_alone"] = round(res["new"]["median_ms"] / res["parent"]["set_source_ms"], 4)
    else:
        res = run(a)
    if a.kernel_stats:
        res["kernel_trace"] = kernel_time(a.kernel_stats)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
