"""What IcpFast's inner motion compensation costs: a 120 000-point pair and a 64-pair batch of them, 20 fixed iterations, the
compensated Align against the rigid form of the same plan (no_certify = 1, no_single_kernel = 1, the mode off), median of 20 calls
after 3.  Writes profiles/inner_compensation_probe.json.

usage: inner_comp_probe.py [out=profiles/inner_compensation_probe.json]
       inner_comp_probe.py trace=1     a few compensated calls only, for a kernel trace taken around this program (comp_apply's own
                                       time); add stats=<the trace's kernel stats csv> to a later plain run to fold them into the json"""
import csv, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import staticmapping_amd as sm
from staticmapping_amd import synth

kv = dict(x.split("=") for x in sys.argv[1:])
N, ITERS, REPS, WARM = 120_000, 20, 20, 3
a, b, T = synth.scan_pair("cfg2", n_points=N)
q, n = sm.calculate_normals(a[:, :3].astype(np.float64))
guess = synth.make_pose(t=(0.6, 0.0, 0.0))


def run(pairs, compensated, reps=REPS, warm=WARM):
    m = sm.IcpFastHip(pair_slots=pairs, max_source_points=len(b), max_target_points=len(q), max_iteration=ITERS, early_exit=0,
                      no_certify=1, no_single_kernel=1, inner_compensation=bool(compensated))
    m.set_input_source(b); m.set_input_target(q, n)
    for s in range(1, pairs):
        m.copy_slot(0, s)
    ms = []
    for k in range(warm + reps):
        t = time.perf_counter()
        R, sc, st = m.align_batch(pairs, [guess] * pairs)
        if k >= warm:
            ms.append((time.perf_counter() - t) * 1e3)
    m.close()
    assert all(s["iterations"] == ITERS for s in st)
    return dict(ms_median=round(float(np.median(ms)), 4), ms_min=round(float(np.min(ms)), 4), ms_max=round(float(np.max(ms)), 4))


if kv.get("trace"):
    for pairs in (1, 64):
        run(pairs, True, reps=3, warm=1)
    sys.exit(0)

out = dict(points=N, target_points=int(len(q)), iterations=ITERS, calls=REPS, warmup=WARM, cases=[])
for pairs in (1, 64):
    rigid, comp = run(pairs, False), run(pairs, True)
    case = dict(pairs=pairs, rigid_no_certify=rigid, compensated=comp,
                extra_ms_per_call=round(comp["ms_median"] - rigid["ms_median"], 4),
                extra_us_per_pair_and_iteration=round((comp["ms_median"] - rigid["ms_median"]) * 1e3 / (pairs * ITERS), 3),
                ratio=round(comp["ms_median"] / rigid["ms_median"], 4))
    out["cases"].append(case)
    print(json.dumps(case))
if kv.get("stats"):
    rows = [r for r in csv.DictReader(open(kv["stats"])) if any(t in r.get("Name", "") for t in ("comp_apply", "accumulate_comp", "finalize_comp"))]
    out["kernel_trace"] = [dict(name=r["Name"], calls=int(r["Calls"]), average_us=round(float(r["AverageNs"]) / 1e3, 3),
                                total_ms=round(float(r["TotalDurationNs"]) / 1e6, 3)) for r in rows]
path = kv.get("out", os.path.join(ROOT, "profiles", "inner_compensation_probe.json"))
with open(path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote", path)
