"""The derivative kernel and the whole Align of registrators::Ndt under each neighbourhood rule (smhip_ndt_options.search_method:
KDTREE, DIRECT26, DIRECT7, DIRECT1) on BASELINE config #3, one 120 k-point scan against a 500 k-point submap, alone and as a
lock-step batch of 64.

  ndt_search_probe.py [--launches 25] [--batch 64] [--aligns 10] [--modes kdtree,direct26,direct7,direct1] [--out profiles/ndt_search_probe.json]

Per mode: the kernel's time per launch through smhip_ndt_time_derivatives (HIP events around one launch at the pose the Align
ended with; the median, minimum and maximum of --launches such calls after the call's own warm launch), the (point, voxel) pairs a
launch works through, its ALGORITHMIC bytes 12 N_s + 36 pairs (SURVEY section 8(d)'s per-call term, as bench.py quotes it) and
the rate they give -- a rate on algorithmic bytes, not on HBM traffic: the kernel's records are served by the caches -- and the
host-clock time of a whole Align with the voxel table kept (median of --aligns).  SMHIP_PROBE_ROOT=<another checkout> takes the
package and bench.py from there; a library without the option (an older commit) is measured in its only mode, so the same
file times KDTREE on both sides of a comparison."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("SMHIP_PROBE_ROOT", ROOT))
MODES = {"kdtree": 0, "direct26": 1, "direct7": 2, "direct1": 3}


def measure(m, K, guesses, launches, aligns):
    def align():
        return m.align(guesses[0]) if K == 1 else m.align_batch(K, guesses)
    align()                                                  # builds the tables (kept from here on), warms every kernel
    dts = []
    for _ in range(aligns):
        t = time.perf_counter()
        align()                                              # ends in the Align's own synchronise
        dts.append(time.perf_counter() - t)
    stats = m.last_ndt_stats if K == 1 else m.last_ndt_stats[0]
    ms, pairs = [], 0.0
    for _ in range(launches):
        a, pairs = m.time_derivatives(npairs=K, launches=1)
        ms.append(a)
    return {"ms_per_launch_median": statistics.median(ms), "ms_per_launch_min": min(ms), "ms_per_launch_max": max(ms), "launches": launches,
            "pairs_per_launch": pairs, "align_ms_median": 1e3 * statistics.median(dts), "align_ms_min": 1e3 * min(dts), "aligns": aligns,
            "iterations": stats["iterations"], "derivative_calls": stats["derivative_calls"]}


def main(args):
    import torch
    import numpy as np                                       # noqa: F401
    import staticmapping_amd as sm
    import bench
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU: this probe measures on the device only"}))
        return 1
    has_option = hasattr(sm._capi.NdtOptions, "search_method")
    modes = [x for x in args.modes.split(",") if x] if has_option else ["kdtree"]
    src, tgt, T, G = bench._submap_case(5, 500_000, 4, torch.device("cuda", 0))
    ns = len(src)
    out = {"workload": "BASELINE config #3: 120k-point scan vs 500k-point submap, resolution 1.0, guess 0.3 m / 1 degree off; voxel tables kept",
           "has_search_method": has_option, "ns": ns, "nt": len(tgt),
           "bytes": "algorithmic: 12 ns + 36 pairs per evaluation; the rate is on these bytes, not on HBM traffic", "single": {}, "batch": {}}
    from staticmapping_amd import synth
    for K, key in ((1, "single"), (args.batch, "batch")):
        if K < 1:
            continue
        m = sm.NdtHip(max_source_points=ns, max_target_points=len(tgt), pair_slots=K)
        for k in range(K):
            m.set_input_source(src, slot=k); m.set_input_target(tgt, slot=k)
        m.set_target_cache(True)
        gs = [G @ synth.make_pose(t=(0.01 * (k % 8), -0.01 * (k % 5), 0.0), rpy_deg=(0, 0, 0.05 * (k % 7))) for k in range(K)]
        gs[0] = G
        for name in modes:
            if has_option:
                m.set_ndt_options(search_method=MODES[name])
            r = measure(m, K, gs, args.launches, args.aligns if K == 1 else max(2, args.aligns // 4))
            r["pairs_per_point"] = r["pairs_per_launch"] / (ns * K)
            r["algorithmic_bytes_per_launch"] = 12.0 * ns * K + 36.0 * r["pairs_per_launch"]
            r["algorithmic_GB_per_s"] = r["algorithmic_bytes_per_launch"] / r["ms_per_launch_median"] / 1e6
            out[key][name] = r
            print(f"{key} K={K} {name}: {r['ms_per_launch_median']:.5f} ms/launch (min {r['ms_per_launch_min']:.5f}, max {r['ms_per_launch_max']:.5f}), "
                  f"{r['pairs_per_point']:.3f} pairs/point, align {r['align_ms_median']:.3f} ms", flush=True)
        m.close()
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=25)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--aligns", type=int, default=10)
    ap.add_argument("--modes", default="kdtree,direct26,direct7,direct1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ndt_search_probe.json"))
    sys.exit(main(ap.parse_args()))
