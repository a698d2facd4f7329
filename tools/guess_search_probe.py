"""Time of the device correlative guess search (smhip_guess_search_f32, DESIGN.md section 6 "Guess search") on the pair of
tests/guess_search_cases.py (7.6 m of drift): at scan size (20 000 points) and at submap size (3 x 120 000 points around each pose, voxel
0.1), with the default window (+-20 x +-20 x +-2 voxels of 0.5 m, +-10 steps of 2 degrees: 176 505 candidates) and a +-20 m window
(half_xy 40: 688 905 candidates).  Median of --repeats calls after --warmup calls, a host clock around calls that end in a synchronise (a
call stages and uploads both clouds, launches, reads the box back once in the middle, and copies the result back).  Beside it, on the
same box: ONE call of the numpy restatement (tests/guess_search_ref.py) for the same inputs, checked to give the same pick and scores, and
ONE IcpPointMatcherHip alignment of the same pair from the searched guess and from the drifted one -- the question being whether the search
is small next to the ICP it precedes.  --only CASE runs one case without the yardsticks (for a kernel trace:
rocprofv3 --kernel-trace --stats -- python tools/guess_search_probe.py --only scan_default).
One JSON line on stdout (and in --out when given)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

try:                                  # one HIP runtime per process: torch's first
    import torch  # noqa: F401
except ImportError:
    pass
import numpy as np

WINDOWS = {"default": {}, "wide": {"half_xy": 40}}


def voxel_first(points, size):
    """the first row of every voxel, in order (what a voxel filter keeps of a submap's frames, near enough for a timing)"""
    key = np.floor(points[:, :3] / np.float32(size)).astype(np.int64)
    _, first = np.unique(key, axis=0, return_index=True)
    return np.ascontiguousarray(points[np.sort(first)])


def submap_pair():
    """three 120 000-point scans 0.4 m apart around each pose of the experiment, in the first one's frame, voxel 0.1"""
    import guess_search_cases as cases
    from staticmapping_amd import synth
    _, _, truth, guess = cases.experiment()
    scene = synth.make_scene(0)
    pose_t = synth.make_pose(t=(10.0, -10.0, 0.0), rpy_deg=(0, 0, 90.0))
    out = []
    for base, seed in ((pose_t, 500), (pose_t @ truth, 600)):
        rows = []
        for f in range(3):
            local = synth.make_pose(t=(0.4 * f, 0.0, 0.0))
            scan = synth.velodyne_scan(scene, base @ local, seed=seed + f, n_points=120_000)
            scan[:, :3] = scan[:, :3].astype(np.float64) @ local[:3, :3].T + local[:3, 3]
            rows.append(scan)
        out.append(voxel_first(np.concatenate(rows), 0.1))
    return out[0], out[1], truth, guess


def median_ms(call, warmup, repeats):
    for _ in range(warmup):
        call()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    return float(np.median(t) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import guess_search_cases as cases
    import guess_search_ref as ref
    import staticmapping_amd as sm
    from staticmapping_amd import guess_search as gs
    pairs = {"scan": cases.experiment}
    if not a.only or a.only.startswith("submap"):
        pairs["submap"] = submap_pair
    result = {"repeats": a.repeats, "warmup": a.warmup, "cases": {}}
    for size, make in pairs.items():
        target, source, truth, guess = make()
        cap = max(len(target), len(source))
        h = sm.IcpFastHip(pair_slots=1, max_source_points=cap, max_target_points=cap)
        for wname, window in WINDOWS.items():
            name = size + "_" + wname
            if a.only and a.only != name:
                continue
            got = gs.search(h, target, source, guess, **window)
            case = {"target_points": len(target), "source_points": len(source), "n_candidates": got["n_candidates"], "n_source_used": got["n_source_used"],
                    "best": list(got["best"]), "best_score": got["best_score"], "guess_score": got["guess_score"], "runner_up_score": got["runner_up_score"],
                    "translation_error_of_the_pick_m": float(np.linalg.norm(got["transform"][:3, 3] - truth[:3, 3])),
                    "box_voxels": [int(v) for v in gs.last(h, got)["extent"]],
                    "search_ms": median_ms(lambda: gs.search(h, target, source, guess, **window), a.warmup, a.repeats)}
            if not a.only:
                t0 = time.perf_counter()
                want = ref.search(target, source, guess, **window)
                case["numpy_restatement_ms"] = (time.perf_counter() - t0) * 1e3
                case["equals_restatement"] = bool(want["best"] == got["best"] and want["best_score"] == got["best_score"] and
                                                  want["guess_score"] == got["guess_score"] and want["runner_up_score"] == got["runner_up_score"])
                case["numpy_over_device"] = case["numpy_restatement_ms"] / case["search_ms"]
            result["cases"][name] = case
        h.close()
        if not a.only:
            # the ICP the search precedes: IcpUsingPointMatcher on the same pair, one alignment each (after one to warm the handle up)
            pm = sm.IcpPointMatcherHip(max_points=cap)
            pm.set_input_source(source)
            pm.set_input_target(target)
            pm.align(guess)
            for start_name, start in (("drifted", guess), ("searched", gs_transform(result, size, guess))):
                pm.set_input_source(source)
                pm.set_input_target(target)
                t0 = time.perf_counter()
                _, T = pm.align(start)
                ms = (time.perf_counter() - t0) * 1e3
                result["cases"][size + "_default"]["icp_from_%s" % start_name] = {
                    "align_ms": ms, "score": float(pm.get_fitness_score()), "translation_error_m": float(np.linalg.norm(T[:3, 3] - truth[:3, 3]))}
            d = result["cases"][size + "_default"]
            d["search_over_icp_from_drifted"] = d["search_ms"] / d["icp_from_drifted"]["align_ms"]
            pm.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


def gs_transform(result, size, guess):
    """the searched transform of the default window: rule 8 from the recorded pick"""
    import guess_search_ref as ref
    a_, i_, j_, k_ = result["cases"][size + "_default"]["best"]
    R, t = ref.yaw_transform(guess, a_ * ref.DEFAULTS["yaw_step"])
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t + 0.5 * np.array([i_, j_, k_], np.float64)
    return T


if __name__ == "__main__":
    main()
