"""Time of smhip_icp_information_range on 120 000-point drive pairs, for 1 and for 64 pairs, against smhip_icp_trimmed_score on the same
slots (the matching pass both run; the information call adds exact matches and one pass over the source).  Median of --repeats calls
after --warmup calls, a host clock around calls that end in a synchronise (both do).  Two distinct pairs of the synthetic drive are
uploaded and copied over the slots (smhip_copy_slot).

  python tools/icp_information_probe.py --out profiles/icp_information_probe.json
  rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/icp_information_probe.py --pairs 64 --repeats 10 --out DIR/traced.json
  python tools/icp_information_probe.py --kernel-stats DIR/.../trace_kernel_stats.csv --traced DIR/traced.json --merge profiles/icp_information_probe.json

The last form adds, from the trace (a run of its own: tracing slows the host), information_sums' time per launch and its algorithmic
bytes -- 24 B per row + 32 B per kept row -- over that time, beside what DESIGN.md section 5 records for a no-arithmetic kernel of the
same access shape (4.6-5.0 TB/s).  The comparison is reported, not asserted.  One JSON line on stdout (and in --out / --merge)."""
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

N_POINTS, RATIO = 120_000, 0.7
NO_ARITHMETIC_TBPS = (4.6, 5.0)          # a no-arithmetic kernel of the same access shape


def run(a):
    device = None
    try:
        import torch  # noqa: F401   (one HIP runtime per process: torch's first, as in tests/conftest.py)
        device = "cuda" if torch.cuda.is_available() else None
    except ImportError:
        pass
    import staticmapping_amd as sm
    from staticmapping_amd import _capi, synth
    lib = _capi.load_library()
    if lib.smhip_device_count() < 1:
        raise SystemExit("no gfx950 device visible: nothing can be timed")
    counts = [int(k) for k in a.pairs.split(",")]
    slots = max(counts)
    pairs = synth.drive_pairs(2, n_points=a.points, device=device)
    cap_t = max(len(p["q"]) for p in pairs)
    m = sm.IcpFastHip(pair_slots=slots, max_source_points=a.points, max_target_points=cap_t)
    for k, p in enumerate(pairs[:slots]):
        m.set_input_source(p["src"], slot=k)
        m.set_input_target(p["q"], p["n"], slot=k)
    for k in range(len(pairs), slots):
        m.copy_slot(k % len(pairs), k)
    Ts = [pairs[k % len(pairs)]["T"] for k in range(slots)]
    packed = m._pack_guesses(slots, Ts)
    out = (_capi.IcpInformation * slots)()
    score, kept = ctypes.c_double(), ctypes.c_int32()
    res = {"points": a.points, "target_points": [len(p["q"]) for p in pairs], "ratio": RATIO, "repeats": a.repeats, "warmup": a.warmup, "pairs": {}}

    def information(k):
        m._check(lib.smhip_icp_information_range(m._h, 0, k, packed.ctypes.data_as(_capi.c_double_p), RATIO, out))

    def trimmed(k):
        for s in range(k):
            m._check(lib.smhip_icp_trimmed_score(m._h, s, packed[s].ctypes.data_as(_capi.c_double_p), RATIO, ctypes.byref(score), ctypes.byref(kept)))

    for k in counts:
        row = {}
        for name, call in (("information_range_ms", information), ("trimmed_score_ms", trimmed)):
            for _ in range(a.warmup):
                call(k)
            t = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                call(k)
                t.append(time.perf_counter() - t0)
            row[name] = round(float(np.median(t)) * 1e3, 4)
            row[name.replace("_ms", "_spread_ms")] = [round(float(np.min(t)) * 1e3, 4), round(float(np.max(t)) * 1e3, 4)]
        information(k)
        row["rows"] = int(a.points) * k
        row["kept_rows"] = int(sum(out[s].kept for s in range(k)))
        row["algorithmic_bytes_per_launch"] = 24 * row["rows"] + 32 * row["kept_rows"]
        row["information_over_trimmed_score"] = round(row["information_range_ms"] / row["trimmed_score_ms"], 4)
        res["pairs"][str(k)] = row
    m.close()
    return res


def kernel_row(path, traced):
    """information_sums in a rocprofv3 kernel_stats.csv of a run that launched it for one pair count only"""
    only = list(traced["pairs"].values())
    assert len(only) == 1, "trace one pair count at a time (--pairs 64)"
    with open(path) as f:
        for row in csv.DictReader(f):
            if "information_sums" in row["Name"]:
                total_ns = float(row["TotalDurationNs"]) if "TotalDurationNs" in row else float(row["TotalDurationUs"]) * 1e3
                calls = int(row["Calls"])
                mean_us = total_ns / 1e3 / max(calls, 1)
                tbps = only[0]["algorithmic_bytes_per_launch"] / (mean_us * 1e-6) / 1e12
                return {"kernel": "information_sums", "pairs_per_launch": int(list(traced["pairs"])[0]), "launches": calls, "mean_us": round(mean_us, 3),
                        "algorithmic_bytes_per_launch": only[0]["algorithmic_bytes_per_launch"], "algorithmic_tb_per_s": round(tbps, 4),
                        "no_arithmetic_kernel_tb_per_s": list(NO_ARITHMETIC_TBPS), "share_of_that": [round(tbps / NO_ARITHMETIC_TBPS[1], 4), round(tbps / NO_ARITHMETIC_TBPS[0], 4)]}
    raise SystemExit("no information_sums row in " + path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1,64")
    ap.add_argument("--points", type=int, default=N_POINTS)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--traced", default="")
    ap.add_argument("--merge", default="")
    a = ap.parse_args()
    if a.kernel_stats:
        res = json.load(open(a.merge)) if a.merge and os.path.exists(a.merge) else {}
        res["kernel_trace"] = kernel_row(a.kernel_stats, json.load(open(a.traced)))
        a.out = a.merge or a.out
    else:
        res = run(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
