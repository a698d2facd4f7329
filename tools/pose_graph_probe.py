"""Time of one device pose-graph optimisation (smhip_pose_graph_optimize: one kernel launch) at the size of a KITTI-00 run: a
circle drive of 909 submaps (tests/pose_graph_ref.py circle_drive), once overlapping its start by 4 submaps with 3 loop edges and once by 64 with 60, from the
chained odometry.  Median of --repeats calls after --warmup calls, a host clock around calls that end in a synchronise (the call uploads
the graph, launches, and copies the poses back).  Beside it, as the yardstick on the same box, the restatement with scipy's sparse
direct solve: its whole time (the linearisation there is a Python loop) and the time inside the sparse solves alone.
--gps: instead, the same size as four laps with no loop edge and a GPS (ENU) factor on every submap (profiles/pose_graph_gps_probe.json).
--huber K: the two loop cases through smhip_pose_graph_optimize_robust with the Huber threshold K on every loop edge (DESIGN.md section 6,
"Robust factors"); --bad-loops M: M wrong loop edges beside the good ones, alternately 3 m ahead and 3 m behind (as many as the overlap has
room for: one with 3 loop edges, four with 60), with or without --huber.  Without either flag the run is what it was.
--odom: instead, the drive with 3 loop edges re-based to start at the identity, with an odometry calibration (HANDEYE) factor of threshold
1 on every submap through smhip_pose_graph_optimize_calib ("Odometry calibration factor"): the calibration node is a
chord to every submap.  The calibration is held at the truth; with --odom-calib it is free from a start 0.1 rad off.
--join: instead, two drives of 909 submaps joined (tests/multi_trajectory_ref.py: the graph MultiTrajectoryMapBuilder solves, DESIGN.md
section 6, "Joining maps"): the second loaded 0.5 m and 0.5 degrees off, a cross edge on every second of its submaps, once with the base
map free and once held (profiles/pose_graph_join_probe.json).  The free solve can run for a minute: use --repeats 2 --warmup 1.
--marginals: instead, the two loop cases optimised and then smhip_pose_graph_marginals for ALL their free submaps (DESIGN.md section 6,
"Marginal covariances"): the time of the marginals call beside the optimise call's, and beside both the time numpy.linalg.inv takes
(median of the same repeats after the same warm-up) for the same H (5 454 x 5 454, built by tests/pose_graph_marginals_ref.py at the device's poses) on the host, with the largest
difference between the two (profiles/pose_graph_marginals_probe.json).
One JSON line on stdout (and in --out when given)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_NODES = 909


def gps_case(m, a):
    """909 submaps, four laps of a circle with no loop edge, a GPS factor on every submap (tests/pose_graph_gps_cases.py): the frame
    node last, its prior at the alone-solve result of the first 25 submaps"""
    import pose_graph_gps_cases as cases
    import pose_graph_gps_ref as gps
    from staticmapping_amd import pose_graph
    g = cases.circle_gps(N_NODES, 1, loops=(), every=1, overlap=682)

    def call():
        return pose_graph.optimize_factors(m, g["poses"], g["kinds"], g["ij"], g["data"], fixed=g["fixed"], sigmas=g["sigmas"])
    for _ in range(a.warmup):
        call()
    t = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        poses, stats = call()
        t.append(time.perf_counter() - t0)
    case = {"gps_factors": int((g["kinds"] == gps.POINT).sum()), "factors": int(len(g["kinds"])), "device_median_ms": round(float(np.median(t)) * 1e3, 4),
            "device_min_ms": round(float(np.min(t)) * 1e3, 4), "outer_steps": stats["iterations"], "rejected_steps": stats["rejected_steps"],
            "pcg_iterations": stats["pcg_iterations"], "pcg_longest_solve": stats["pcg_max_iterations"], "pcg_cap": stats["pcg_cap"],
            "levels": stats["levels"], "stop": stats["stop"], "initial_cost": stats["initial_cost"], "final_cost": stats["final_cost"],
            "enu_error_before_m": cases.enu_error(g, g["poses"]), "enu_error_after_m": cases.enu_error(g, poses)}
    if not a.no_restatement:
        t0 = time.perf_counter()
        want, st = gps.optimize(g, solver="sparse")
        case["restatement_sparse_total_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        case["restatement_steps"] = st["accepted"] + st["rejected"]
        case["difference_m"] = float(np.abs(poses[:, :3, 3] - want[:, :3, 3]).max())
    return case


def odom_case(m, a):
    """909 submaps with 3 loop edges and a HANDEYE factor on every submap (tests/pose_graph_calib_cases.py): the calibration node last"""
    import pose_graph_calib_cases as cases
    import pose_graph_calib_ref as calib
    from staticmapping_amd import pose_graph
    g = cases.ring_odom(N_NODES, 1, a.odom_calib)

    def call():
        return pose_graph.optimize_calib(m, g["poses"], g["kinds"], g["ij"], g["data"], fixed=g["fixed"], sigmas=g["sigmas"], huber=g["huber"])
    for _ in range(a.warmup):
        call()
    t = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        poses, stats = call()
        t.append(time.perf_counter() - t0)
    r0, t0m = cases.calib_errors(g["poses"][g["calib_node"]])
    r1, t1m = cases.calib_errors(poses[g["calib_node"]])
    return {"odom_factors": int((g["kinds"] == calib.HANDEYE).sum()), "calibration": "free" if a.odom_calib else "held", "factors": int(len(g["kinds"])),
            "device_median_ms": round(float(np.median(t)) * 1e3, 4), "device_min_ms": round(float(np.min(t)) * 1e3, 4), "outer_steps": stats["iterations"],
            "rejected_steps": stats["rejected_steps"], "pcg_iterations": stats["pcg_iterations"], "pcg_longest_solve": stats["pcg_max_iterations"],
            "pcg_cap": stats["pcg_cap"], "levels": stats["levels"], "stop": stats["stop"], "initial_cost": stats["initial_cost"], "final_cost": stats["final_cost"],
            "truth_error_before_m": cases.truth_error(g, g["poses"]), "truth_error_after_m": cases.truth_error(g, poses),
            "calib_rotation_error_rad": [r0, r1], "calib_translation_error_m": [t0m, t1m]}


def join_cases(m, a):
    """909 + 909 submaps, a cross edge on every second incremental submap from the fourth on; the base free, then held"""
    import multi_trajectory_ref as mt
    from staticmapping_amd import pose_graph
    case = mt.join_case(N_NODES, N_NODES, every=2)
    with_edge = [s for _, s, _ in case["cross"]]
    out = []
    for hold in (False, True):
        g = mt.assemble(case, hold_base=hold)

        def call():
            return pose_graph.optimize_robust(m, g["poses"], g["kinds"], g["ij"], g["data"], fixed=g["fixed"], sigmas=g["sigmas"], huber=g["huber"])
        for _ in range(a.warmup):
            call()
        t = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            poses, stats = call()
            t.append(time.perf_counter() - t0)
        rep = pose_graph.last_robust(m, len(g["kinds"]))
        before = [mt.mutual_error(case, g["poses"], s) for s in with_edge]
        after = [mt.mutual_error(case, poses, s) for s in with_edge]
        out.append({"join": "909 + 909", "hold_base": hold, "nodes": int(len(g["poses"])), "factors": int(len(g["kinds"])), "cross_edges": len(with_edge),
                    "device_median_ms": round(float(np.median(t)) * 1e3, 4), "device_min_ms": round(float(np.min(t)) * 1e3, 4), "outer_steps": stats["iterations"],
                    "rejected_steps": stats["rejected_steps"], "pcg_iterations": stats["pcg_iterations"], "pcg_longest_solve": stats["pcg_max_iterations"],
                    "pcg_cap": stats["pcg_cap"], "pcg_total_limit": 200000, "levels": stats["levels"],
                    "stop": stats["stop"], "initial_cost": stats["initial_cost"], "final_cost": stats["final_cost"],
                    "cross_edges_downweighted": int((rep["weight"][g["loops"]] < 1.0).sum()),
                    "mutual_error_before_m": [round(float(np.min(before)), 4), round(float(np.max(before)), 4)],
                    "mutual_error_after_m": [round(float(np.median(after)), 4), round(float(np.max(after)), 4)],
                    "mutual_error_after_at_submap_0_m": round(mt.mutual_error(case, poses, 0), 4),
                    "base_moved_m": float(np.linalg.norm(poses[:N_NODES, :3, 3] - case["base"][:, :3, 3], axis=1).max())})
    return out


def marginals_case(m, a, g, n_loops):
    """optimise, then the marginal covariances of every free submap in one call; numpy's dense inverse of the same H as the yardstick"""
    import pose_graph_marginals_ref as mref
    from staticmapping_amd import pose_graph

    def timed(call):
        for _ in range(a.warmup):
            call()
        t, out = [], None
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            out = call()
            t.append(time.perf_counter() - t0)
        return t, out
    t_opt, (poses, stats) = timed(lambda: pose_graph.optimize(m, g["poses"], g["edges"], g["Z"], fixed=g["fixed"]))
    free = [k for k in range(N_NODES) if not g["fixed"][k]]
    t_mar, (cov, _, ms) = timed(lambda: pose_graph.marginals(m, N_NODES, free))
    t_one, _ = timed(lambda: pose_graph.marginals(m, N_NODES, free[-1:]))
    case = {"loop_edges": n_loops, "edges": int(len(g["edges"])), "queries": len(free), "optimise_median_ms": round(float(np.median(t_opt)) * 1e3, 4),
            "optimise_pcg_iterations": stats["pcg_iterations"], "marginals_median_ms": round(float(np.median(t_mar)) * 1e3, 4),
            "marginals_min_ms": round(float(np.min(t_mar)) * 1e3, 4), "marginals_one_query_median_ms": round(float(np.median(t_one)) * 1e3, 4),
            "workgroups": ms["workgroups"], "marginals_pcg_iterations": ms["pcg_iterations"],
            "marginals_pcg_longest_column": ms["pcg_max_iterations"], "pcg_cap": ms["pcg_cap"],
            "iterations_per_query": round(ms["pcg_iterations"] / len(free), 2),
            "queries_per_workgroup": -(-len(free) // ms["workgroups"]),
            "largest_position_sigma_m": float(np.sqrt(np.trace(cov[:, 3:, 3:], axis1=1, axis2=2)).max())}
    if not a.no_restatement:
        H, fixed, _ = mref.system(g, poses)
        Hd = np.asarray(H)
        t_inv, X = timed(lambda: np.linalg.inv(Hd))                        # the same warm-up and repeats as the device calls
        case["host_numpy_inv_ms"] = round(float(np.median(t_inv)) * 1e3, 1)
        case["host_numpy_inv_min_ms"] = round(float(np.min(t_inv)) * 1e3, 1)
        case["host_threads_note"] = "numpy.linalg.inv of the %d x %d H, LAPACK on every core the process may use" % H.shape
        want = np.stack([0.5 * (X[6 * k:6 * k + 6, 6 * k:6 * k + 6] + X[6 * k:6 * k + 6, 6 * k:6 * k + 6].T) for k in free])
        case["difference_to_inv_relative"] = float(np.abs(cov - want).max() / np.abs(want).max())
    return case


def robust_case(m, a, drive, n_loops, overlap):
    """the loop case `drive` as factors, plus --bad-loops wrong loop edges, solved with the threshold --huber on the loop edges"""
    import pose_graph_robust_cases as cases
    from staticmapping_amd import pose_graph
    period = N_NODES - overlap
    bad = [(n_loops + q, n_loops + q + period, (3.0 if q % 2 == 0 else -3.0, 0.0, 0.0), 0.0) for q in range(min(a.bad_loops, overlap - n_loops))]
    g = cases.as_factors(drive, n_loops, bad, k=a.huber)
    hub = g["huber"] if a.huber > 0.0 else None

    def call():
        return pose_graph.optimize_robust(m, g["poses"], g["kinds"], g["ij"], g["data"], fixed=g["fixed"], sigmas=g["sigmas"], huber=hub)
    for _ in range(a.warmup):
        call()
    t = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        poses, stats = call()
        t.append(time.perf_counter() - t0)
    rep = pose_graph.last_robust(m, len(g["kinds"]))
    return {"loop_edges": n_loops, "bad_loop_edges": len(bad), "huber": a.huber, "edges": int(len(g["kinds"])), "device_median_ms": round(float(np.median(t)) * 1e3, 4),
            "device_min_ms": round(float(np.min(t)) * 1e3, 4), "outer_steps": stats["iterations"], "rejected_steps": stats["rejected_steps"],
            "pcg_iterations": stats["pcg_iterations"], "pcg_longest_solve": stats["pcg_max_iterations"], "pcg_cap": stats["pcg_cap"],
            "levels": stats["levels"], "stop": stats["stop"], "initial_cost": stats["initial_cost"], "final_cost": stats["final_cost"],
            "loop_edges_downweighted": int((rep["weight"] < 1.0).sum()), "bad_loop_weights": [float(w) for w in rep["weight"][g["bad"]]],
            "truth_error_m": cases.truth_error(g, poses)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-restatement", action="store_true")
    ap.add_argument("--gps", action="store_true", help="the 909-submap drive that never closes a loop, with a GPS factor on every submap, instead of the two loop cases")
    ap.add_argument("--huber", type=float, default=0.0, help="the Huber threshold of every loop edge (0: none), through smhip_pose_graph_optimize_robust")
    ap.add_argument("--bad-loops", type=int, default=0, help="wrong loop edges added beside the good ones")
    ap.add_argument("--odom", action="store_true", help="an odometry calibration factor on every submap of the drive with 3 loop edges, instead of the two loop cases")
    ap.add_argument("--odom-calib", action="store_true", help="with --odom: the calibration free, from a start 0.1 rad off")
    ap.add_argument("--join", action="store_true", help="two 909-submap drives joined, a cross edge on every second incremental submap, with the base free and held")
    ap.add_argument("--marginals", action="store_true", help="the two loop cases, then the marginal covariances of all their free submaps, beside numpy's dense inverse")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    try:
        import torch  # noqa: F401   (one HIP runtime per process: torch's first, as in tests/conftest.py)
    except ImportError:
        pass
    import pose_graph_ref as ref
    import staticmapping_amd as sm
    from staticmapping_amd import pose_graph
    m = sm.IcpFastHip(pair_slots=1, max_source_points=1024, max_target_points=1024)
    res = {"nodes": N_NODES, "repeats": a.repeats, "warmup": a.warmup, "cases": []}
    if a.gps:
        res["cases"].append(gps_case(m, a))
    if a.odom:
        res["cases"].append(odom_case(m, a))
    if a.join:
        res["cases"] += join_cases(m, a)
    for n_loops in (() if a.gps or a.odom or a.join else (3, 60)):
        # the drive overlaps its start by four submaps (three loop edges) or by 64 (sixty: every revisited submap closes on its first visit)
        g = ref.circle_drive(N_NODES, seed=1, loops=[(k, None) for k in range(n_loops)], overlap=4 if n_loops <= 4 else 64)
        if a.marginals:
            res["cases"].append(marginals_case(m, a, g, n_loops))
            continue
        if a.huber > 0.0 or a.bad_loops > 0:
            res["cases"].append(robust_case(m, a, g, n_loops, 4 if n_loops <= 4 else 64))
            continue

        def call():
            return pose_graph.optimize(m, g["poses"], g["edges"], g["Z"], fixed=g["fixed"])
        for _ in range(a.warmup):
            call()
        t = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            poses, stats = call()
            t.append(time.perf_counter() - t0)
        case = {"loop_edges": n_loops, "edges": int(len(g["edges"])), "device_median_ms": round(float(np.median(t)) * 1e3, 4),
                "device_min_ms": round(float(np.min(t)) * 1e3, 4), "outer_steps": stats["iterations"], "rejected_steps": stats["rejected_steps"],
                "pcg_iterations": stats["pcg_iterations"], "pcg_longest_solve": stats["pcg_max_iterations"], "pcg_cap": stats["pcg_cap"],
                "levels": stats["levels"], "stop": stats["stop"], "initial_cost": stats["initial_cost"], "final_cost": stats["final_cost"]}
        # barriers of one launch: per M^-1 application 2 levels + 2, per factorisation 2 levels + 2, per PCG iteration that plus H p (2),
        # two dot products (2 each) and two vector updates
        case["barriers_per_minv"] = 2 * stats["levels"] + 2
        if not a.no_restatement:
            t0 = time.perf_counter()
            want, st = ref.optimize(g["poses"], g["fixed"], g["edges"], g["Z"], solver="sparse")
            case["restatement_sparse_total_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            case["restatement_sparse_solves_ms"] = round(st.get("solve_seconds", 0.0) * 1e3, 1)
            case["restatement_steps"] = st["accepted"] + st["rejected"]
            case["difference_m"] = float(np.abs(poses[:, :3, 3] - want[:, :3, 3]).max())
        res["cases"].append(case)
    m.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
