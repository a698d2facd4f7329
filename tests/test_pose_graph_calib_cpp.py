"""The odometry calibration factor without a GPU: tests/cpp/test_pose_graph_calib.cc `host` checks that PoseGraph emits the arrays it
always did while no calibration vertex exists, where the vertex, its prior and the HANDEYE factors go when one does, and which entry
Optimize takes; its `solve` mode runs the kernel's own loop (csrc/pose_graph_kernel.h), compiled for the CPU as one thread, over the
graphs of tests/pose_graph_calib_cases.py against tests/pose_graph_calib_ref.py -- the same code the device runs; its `isam host` mode
feeds IsamOptimizer with use_odom a ring frame by frame through AddDetected."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import pose_graph_calib_cases as cases
import pose_graph_calib_ref as calib
import pose_graph_cases as base
import pose_graph_ref as ref
import pose_graph_robust_cases as robust_cases
from test_pose_graph_robust_cpp import _pack12

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_pose_graph_calib.cc")


def _build_exe():
    from staticmapping_amd import build
    lib = build.build()
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "test_pose_graph_calib")
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


def test_todays_arrays_the_new_vertex_and_the_choice_of_entry_on_the_host():
    out = subprocess.run([_build_exe(), "host"], text=True, capture_output=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout


def host_solve(g, tmp_path, v, huber, max_iterations=50):
    """the kernel's loop on the CPU: (poses [N, 4, 4], stats dict, the report at them, the first linearisation with its weights, the
    output's bytes); test_pose_graph_robust_cpp.host_solve's file format"""
    n, m = len(g["poses"]), len(g["kinds"])
    Z, sinv = np.zeros((m, 12)), np.zeros((m, 6))
    for k in range(m):
        if g["kinds"][k] == calib.POINT:
            Z[k, :6], sinv[k, :3] = g["data"][k, :6], 1.0 / g["sigmas"][k, :3]
        else:
            Z[k], sinv[k] = _pack12(g["data"][k].reshape(1, 4, 4).transpose(0, 2, 1))[0], 1.0 / g["sigmas"][k]
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as fh:
        fh.write(struct.pack("<ii", n, m))
        for a in (_pack12(g["poses"]), Z, sinv, np.asarray(v)):
            fh.write(a.astype("<f8").tobytes())
        for a in (np.asarray(g["fixed"]), g["ij"], g["kinds"]):
            fh.write(a.astype("<i4").tobytes())
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


@pytest.mark.parametrize("name", cases.names())
def test_the_kernels_loop_on_the_cpu_agrees_with_the_restatement(name, tmp_path):
    """First-linearisation parity (cases.check_stage_parity), then the result: poses within 1e-9 m and 1e-9 of the restatement's direct
    solve, the same stop reason, counts and damping, every solve below its cap; then the report at the result."""
    g, want, st = cases.reference(name)
    _, _, sp = cases.reference(name, "pcg")
    v = base.probe_vector(len(g["poses"]))
    poses, stats, report, lin, _ = host_solve(g, tmp_path, v, g["huber"])
    cases.check_stage_parity(g, lin, v)
    dt, dr = base.pose_difference(poses, want)
    print(name, "difference", dt, dr, stats, "restatement", st["stop"], st["accepted"], st["rejected"], "longest solve", stats["pcg_max_iterations"], "restatement", sp["pcg_max"])
    assert dt < 1e-9 and dr < 1e-9
    base.check_costs(stats, st)
    assert (stats["stop_reason"], stats["accepted_steps"], stats["rejected_steps"], stats["damping"]) == (st["stop"], st["accepted"], st["rejected"], st["damping"])
    assert stats["pcg_max_iterations"] < 12 * calib.non_chain_edges(g) + 64
    assert abs(stats["pcg_max_iterations"] - sp["pcg_max"]) <= max(2, 0.1 * sp["pcg_max"])
    fx = np.asarray(g["fixed"]).astype(bool)
    assert (poses[fx] == g["poses"][fx]).all()
    robust_cases.check_report_parity(g, report, calib.report(g, want))
    assert abs(report[2].sum() - stats["final_cost"]) <= 1e-12 * max(stats["final_cost"], 1e-300)


# ---- IsamOptimizer ----------------------------------------------------------------------------------------------------------------

def write_drive(path, g, use_odom, free, huber, tf, has=None):
    """a ring of pose_graph_calib_cases as IsamOptimizer is fed it: the first pose, every chain factor as the matched transform from
    the previous frame, every frame's odometer pose, the loop factors as detector results"""
    n = len(g["truth"])
    between = [k for k in range(len(g["kinds"])) if g["kinds"][k] == calib.BETWEEN]
    chain, loops = between[:n - 1], between[n - 1:]
    row = lambda M: " ".join("%.17g" % x for x in np.asarray(M).ravel())
    with open(path, "w") as fh:
        fh.write("%d %d %.17g\n%s\n%d\n" % (use_odom, free, huber, row(tf), n))
        for k in range(n):
            if k:
                assert tuple(g["ij"][chain[k - 1]]) == (k - 1, k)
            step = g["poses"][0] if k == 0 else g["data"][chain[k - 1]].reshape(4, 4).T
            fh.write("%d %s %s\n" % (1 if has is None or has[k] else 0, row(step), row(g["odom"][k])))
        fh.write("%d\n" % len(loops))
        for k in loops:
            fh.write("%d %d " % tuple(g["ij"][k]) + row(g["data"][k].reshape(4, 4).T) + "\n")


def run_isam(where, tmp_path, g, use_odom, free, huber=1.0, tf=None, has=None):
    tf = ref.inv(g["poses"][g["calib_node"]]) if tf is None else tf
    src = tmp_path / ("drive_%d_%d.txt" % (use_odom, free))
    write_drive(src, g, use_odom, free, huber, tf, has)
    out = subprocess.run([_build_exe(), "isam", where, str(src)], text=True, capture_output=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    res = json.loads(out.stdout.strip().splitlines()[-1])
    res["poses"] = np.array(res["poses"]).reshape(-1, 4, 4)
    res["tf"] = np.array(res["tf"]).reshape(4, 4)
    return res


def check_isam(g_held, g_free, held, free, plain, device=False):
    """what both the CPU and the device run of the AddDetected sequence must show"""
    n = len(g_held["truth"])
    assert held["ok"] and free["ok"] and plain["ok"] and all(r["stop_reason"] in (1, 2) for r in (held, free, plain))
    assert held["odom_factors"] == free["odom_factors"] == n and plain["odom_factors"] == 0
    assert held["has_calib"] and held["held"] and free["has_calib"] and not free["held"] and not plain["has_calib"]
    assert held["tf_untouched_before_final"] and free["tf_untouched_before_final"]
    if device:                                                                                   # (the Solver hook makes no entry call)
        assert plain["entries"][3] == 0 and held["entries"][3] > 0 and free["entries"][3] > 0   # the calib entry only with a HANDEYE
    assert np.abs(held["tf"] - ref.inv(cases.T_TRUE)).max() <= 1e-15                             # held: written back as it was, up to the two inversions
    r0, _ = cases.calib_errors(cases.T_START)
    r1, t1 = cases.calib_errors(ref.inv(free["tf"]))
    e_plain, e_held, e_free = (cases.truth_error(g_held, r["poses"]) for r in (plain, held, free))
    print("worst distance to the truth: plain %.3f m, held %.3f m, free %.3f m; calibration rotation error %.4f -> %.4f rad, translation %.4f m" % (e_plain, e_held, e_free, r0, r1, t1))
    assert r1 < r0 / 5.0
    assert e_held < e_plain
    assert np.abs(held["poses"][0] - g_held["poses"][0]).max() == 0.0


def test_isam_optimizer_with_use_odom_through_the_solver_hook(tmp_path):
    """ring64 frame by frame: the final batch solve starts from the incremental estimate and ends in the restatement's minimum"""
    g_held, g_free = cases.graph("ring64_held"), cases.graph("ring64_free")
    held = run_isam("host", tmp_path, g_held, 1, 0)
    free = run_isam("host", tmp_path, g_free, 1, 1)
    plain = run_isam("host", tmp_path, g_held, 0, 0)
    check_isam(g_held, g_free, held, free, plain)
    for name, res in (("ring64_held", held), ("ring64_free", free)):
        _, want, _ = cases.reference(name)
        dt, dr = base.pose_difference(res["poses"], want[:len(res["poses"])])
        print(name, "incremental against the batch restatement", dt, dr)
        assert dt < 1e-6
    _, want, _ = cases.reference("ring64_free")
    assert np.abs(ref.inv(free["tf"]) - want[g_free["calib_node"]]).max() < 1e-6


def test_frames_without_a_reading_get_no_factor(tmp_path):
    g = cases.graph("ring16_held")
    has = [k % 3 != 1 for k in range(16)]
    res = run_isam("host", tmp_path, g, 1, 0, has=has)
    assert res["ok"] and res["odom_factors"] == sum(has)
