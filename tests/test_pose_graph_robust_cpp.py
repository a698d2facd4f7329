"""Huber-robust factors without a GPU: tests/cpp/test_pose_graph_robust.cc `host` checks every refusal of smhip_pose_graph_plan_robust,
PoseGraph and IsamOptimizer carrying the threshold to the loop edges and to nothing else, and which entry PoseGraph::Optimize takes;
its `solve` mode runs the kernel's own loop (csrc/pose_graph_kernel.h), compiled for the CPU as one thread, over the graphs of
tests/pose_graph_robust_cases.py against tests/pose_graph_robust_ref.py -- the same code the device runs; its `isam host` mode feeds
IsamOptimizer a ring with one wrong loop edge through AddDetected."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import pose_graph_cases as base
import pose_graph_gps_ref as gps
import pose_graph_ref as ref
import pose_graph_robust_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_pose_graph_robust.cc")


def _build_exe():
    from staticmapping_amd import build
    lib = build.build()
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "test_pose_graph_robust")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = [os.path.join(ROOT, "include", "smhip", h) for h in ("pose_graph.h", "submap.h", "back_end.h", "m2dp.h", "registrator.h", "filters.h")]
    deps += [os.path.join(ROOT, "include", "smhip.h"), os.path.join(ROOT, "staticmapping_amd", "csrc", "pose_graph_kernel.h"),
             os.path.join(ROOT, "staticmapping_amd", "csrc", "pose_graph_plan.h"), SRC, lib]
    if (not os.path.exists(exe)) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                               "-L", os.path.dirname(lib), "-lsmhip", "-ldl", "-Wl,-rpath," + os.path.dirname(lib),
                               "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_the_source_compiles_without_a_gpu():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), SRC])


def test_refusals_thresholds_on_loop_edges_only_and_the_choice_of_entry_on_the_host():
    out = subprocess.run([_build_exe(), "host"], text=True, capture_output=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout


def _pack12(X):
    return np.concatenate([X[:, :3, :3].reshape(len(X), 9), X[:, :3, 3]], axis=1)


def host_solve(g, tmp_path, v, huber, max_iterations=50):
    """the kernel's loop on the CPU: (poses [N, 4, 4], stats dict, the report at them, the first linearisation with its weights, the
    output's bytes).  huber: None (no threshold array at all) or [F]."""
    n, m = len(g["poses"]), len(g["kinds"])
    Z, sinv = np.zeros((m, 12)), np.zeros((m, 6))
    for k in range(m):
        if g["kinds"][k] == gps.POINT:
            Z[k, :6], sinv[k, :3] = g["data"][k, :6], 1.0 / g["sigmas"][k, :3]
        else:
            Z[k], sinv[k] = _pack12(g["data"][k].reshape(1, 4, 4).transpose(0, 2, 1))[0], 1.0 / g["sigmas"][k]
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as fh:
        fh.write(struct.pack("<ii", n, m))
        fh.write(_pack12(g["poses"]).astype("<f8").tobytes())
        fh.write(Z.astype("<f8").tobytes())
        fh.write(sinv.astype("<f8").tobytes())
        fh.write(np.asarray(v, "<f8").tobytes())
        fh.write(np.asarray(g["fixed"]).astype("<i4").tobytes())
        fh.write(g["ij"].astype("<i4").tobytes())
        fh.write(g["kinds"].astype("<i4").tobytes())
        fh.write(struct.pack("<ii", max_iterations, 0 if huber is None else 1))
        if huber is not None:
            fh.write(np.asarray(huber, "<f8").tobytes())
    out = subprocess.run([_build_exe(), "solve", str(src), str(dst)], text=True, capture_output=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(dst, "rb").read()
    a = np.frombuffer(raw, "<f8")
    at = [0]

    def take(*shape):
        k = int(np.prod(shape))
        r = a[at[0]:at[0] + k].reshape(shape)
        at[0] += k
        return r
    p12 = take(n, 12)
    poses = np.tile(np.eye(4), (n, 1, 1))
    poses[:, :3, :3] = p12[:, :9].reshape(n, 3, 3)
    poses[:, :3, 3] = p12[:, 9:]
    od, oi = take(3), take(6).astype(int)
    stats = dict(initial_cost=od[0], final_cost=od[1], damping=od[2], stop_reason=oi[0], iterations=oi[1], accepted_steps=oi[2], rejected_steps=oi[3],
                 pcg_iterations=oi[4], pcg_max_iterations=oi[5])
    report = (take(m), take(m), take(m))
    lin = dict(r=take(m, 6), A=take(m, 6, 6), B=take(m, 6, 6), g=take(n, 6), minv_v=take(n, 6), w=take(m))
    assert at[0] == len(a)
    return poses, stats, report, lin, raw


@pytest.mark.parametrize("name", cases.SMALL)
def test_the_kernels_loop_on_the_cpu_agrees_with_the_restatement(name, tmp_path):
    """Stage by stage with the weights (cases.check_stage_parity), then the result: poses within 1e-9 m and 1e-9 of the restatement's
    direct solve, the same stop reason, counts and damping, every iteration count below its cap; then the report at the result."""
    g, want, st, rep = cases.reference(name)
    v = base.probe_vector(len(g["poses"]))
    poses, stats, report, lin, _ = host_solve(g, tmp_path, v, g["huber"])
    cases.check_stage_parity(g, lin, v)
    dt, dr = base.pose_difference(poses, want)
    print(name, "difference", dt, dr, stats, "restatement", st["stop"], st["accepted"], st["rejected"])
    assert dt < 1e-9 and dr < 1e-9
    base.check_costs(stats, st)
    assert (stats["stop_reason"], stats["accepted_steps"], stats["rejected_steps"], stats["damping"]) == (st["stop"], st["accepted"], st["rejected"], st["damping"])
    assert 0 < stats["pcg_max_iterations"] < 12 * gps.non_chain_edges(g) + 64
    fx = np.asarray(g["fixed"]).astype(bool)
    assert (poses[fx] == g["poses"][fx]).all()
    cases.check_report_parity(g, report, rep)
    assert abs(report[2].sum() - stats["final_cost"]) <= 1e-12 * stats["final_cost"]       # the report's terms are the loop's cost
    assert (report[1][g["bad"]] < 0.1).all() and (np.delete(report[1], g["bad"]) == 1.0).all()


def test_thresholds_that_never_act_leave_every_bit(tmp_path):
    """circle64 through the same binary without a threshold array, with zeros and with 1e30: the same bytes -- poses, costs, counts, the
    report and the first linearisation"""
    d = base.circle_cases()["circle64"]
    g = gps.make_graph(d["poses"], d["fixed"], [(gps.BETWEEN, int(i), int(j), gps.between_data(Z), ref.DEFAULT_SIGMAS) for (i, j), Z in zip(d["edges"], d["Z"])])
    v = base.probe_vector(64)
    m = len(g["kinds"])
    poses, stats, report, lin, raw = host_solve(g, tmp_path, v, None)
    assert stats["stop_reason"] in (1, 2) and (report[1] == 1.0).all() and (lin["w"] == 1.0).all()
    assert (report[0] ** 2).sum() == pytest.approx(stats["final_cost"], rel=1e-12)
    for hub in (np.zeros(m), np.full(m, 1e30)):
        assert host_solve(g, tmp_path, v, hub)[4] == raw
    want, st = ref.optimize(d["poses"], d["fixed"], d["edges"], d["Z"])                     # ... and they are the plain loop's
    assert max(base.pose_difference(poses, want)) < 1e-9 and (stats["accepted_steps"], stats["rejected_steps"]) == (st["accepted"], st["rejected"])


# ---- IsamOptimizer ----------------------------------------------------------------------------------------------------------------

def write_ring(path, g, huber):
    """robust16 as IsamOptimizer is fed it: the first pose, every chain factor as the matched transform from the previous frame, the loop
    factors as detector results"""
    n = len(g["poses"])
    with open(path, "w") as fh:
        fh.write("%.17g\n%d\n" % (huber, n))
        fh.write(" ".join("%.17g" % x for x in g["poses"][0].ravel()) + "\n")
        for k in range(n - 1):
            assert tuple(g["ij"][k]) == (k, k + 1)
            fh.write(" ".join("%.17g" % x for x in g["data"][k].reshape(4, 4).T.ravel()) + "\n")
        fh.write("%d\n" % len(g["loops"]))
        for k in g["loops"]:
            fh.write("%d %d " % tuple(g["ij"][k]) + " ".join("%.17g" % x for x in g["data"][k].reshape(4, 4).T.ravel()) + "\n")


def run_isam(where, tmp_path, g, huber):
    src = tmp_path / ("ring_%g.txt" % huber)
    write_ring(src, g, huber)
    out = subprocess.run([_build_exe(), "isam", where, str(src)], text=True, capture_output=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    res = json.loads(out.stdout.strip().splitlines()[-1])
    res["poses"] = np.array(res["poses"]).reshape(-1, 4, 4)
    return res


def check_isam(g, robust, plain):
    """what both the CPU and the device run of the AddDetected sequence must show"""
    assert robust["ok"] and plain["ok"] and robust["stop_reason"] in (1, 2) and plain["stop_reason"] in (1, 2)
    assert robust["loop_edges"] == plain["loop_edges"] == 4
    er, ep = cases.truth_error(g, robust["poses"]), cases.truth_error(g, plain["poses"])
    print("worst distance to the truth: %.3f m with loop_closure_huber = 1, %.3f m with 0, ratio %.3f" % (er, ep, er / ep), robust["report"])
    assert er < 0.6 * ep
    pairs = [tuple(int(x) for x in g["ij"][k]) for k in g["loops"]]
    assert [(t, s) for t, s, _, _ in robust["report"]] == pairs == [(t, s) for t, s, _, _ in plain["report"]]
    bad = [tuple(int(x) for x in g["ij"][k]) for k in g["bad"]]
    assert [(t, s) for t, s, _, w in robust["report"] if w < 1.0] == bad             # exactly the corrupted edge is flagged
    assert all(w < 0.1 for t, s, _, w in robust["report"] if (t, s) in bad)
    assert all(w == 1.0 for _, _, _, w in plain["report"])                           # without a threshold nothing is down-weighted ...
    assert [nrm > 1.0 for _, _, nrm, _ in plain["report"]].count(True) >= 1          # ... though the norm shows the strain
    assert np.abs(robust["poses"][0] - g["poses"][0]).max() == 0.0


def test_isam_optimizer_survives_a_wrong_loop_edge_through_the_solver_hook(tmp_path):
    """robust16 frame by frame: the three good loops arrive with frames 12, 13 and 14, the corrupted one with frame 15.  The final
    batch solve starts from the incremental estimate instead of the chained odometry, and ends in the same minimum: no factor other
    than the issue's 0.6 is needed."""
    g = cases.graph("robust16")
    robust, plain = run_isam("host", tmp_path, g, 1.0), run_isam("host", tmp_path, g, 0.0)
    check_isam(g, robust, plain)
    _, want, _, _ = cases.reference("robust16")
    dt, dr = base.pose_difference(robust["poses"], want)
    print("incremental against the batch restatement", dt, dr)
    assert dt < 1e-6                                                                 # the same minimum, approached from another start
