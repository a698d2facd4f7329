"""The BETWEEN factor with a full square-root information without a GPU: tests/cpp/test_pose_graph_info.cc runs the kernel's own loop
(csrc/pose_graph_kernel.h), compiled for the CPU as one thread, over the graphs of tests/pose_graph_info_cases.py against
tests/pose_graph_info_ref.py -- the same code the device runs."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pose_graph_calib_cases as calib_cases
import pose_graph_calib_ref as calib
import pose_graph_cases as base
import pose_graph_info_cases as cases
import pose_graph_info_ref as pgi
import pose_graph_robust_cases as robust_cases
from test_pose_graph_robust_cpp import _pack12

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_pose_graph_info.cc")


def _build_exe():
    from staticmapping_amd import build
    lib = build.build()
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "test_pose_graph_info")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = [os.path.join(ROOT, "include", "smhip", h) for h in ("pose_graph.h", "edge_information.h", "submap.h", "back_end.h", "m2dp.h", "registrator.h", "filters.h")]
    deps += [SRC, os.path.join(ROOT, "include", "smhip.h"), os.path.join(ROOT, "staticmapping_amd", "csrc", "pose_graph_kernel.h"),
             os.path.join(ROOT, "staticmapping_amd", "csrc", "pose_graph_plan.h"), lib]
    if (not os.path.exists(exe)) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                               "-L", os.path.dirname(lib), "-lsmhip", "-ldl", "-Wl,-rpath," + os.path.dirname(lib),
                               "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def host_solve(g, tmp_path, v, info="graph", max_iterations=50):
    """the kernel's loop on the CPU: (poses [N, 4, 4], stats dict, the report at them, the first linearisation with its weights, the
    output's bytes).  info: "graph" = the graph's own L, None = no arrays at all, "none" = arrays that name no L (all -1)"""
    n, m = len(g["poses"]), len(g["kinds"])
    Z, sinv = np.zeros((m, 12)), np.zeros((m, 6))
    for k in range(m):
        if g["kinds"][k] == calib.POINT:
            Z[k, :6], sinv[k, :3] = g["data"][k, :6], 1.0 / g["sigmas"][k, :3]
        else:
            Z[k], sinv[k] = _pack12(g["data"][k].reshape(1, 4, 4).transpose(0, 2, 1))[0], 1.0 / g["sigmas"][k]
    huber = g.get("huber")
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
        fh.write(struct.pack("<i", 0 if info is None else 1))
        if info is not None:
            index, rows = cases.abi_arrays(g) if info == "graph" else (np.full(m, -1, np.int32), np.zeros((0, 36)))
            fh.write(index.astype("<i4").tobytes())
            fh.write(struct.pack("<i", len(rows)))
            fh.write(rows.astype("<f8").tobytes())
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


def test_the_source_compiles_without_a_gpu():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), SRC])


def test_the_graphs_arrays_and_isam_optimizers_option_on_the_host():
    out = subprocess.run([_build_exe(), "host"], text=True, capture_output=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout


@pytest.mark.parametrize("name", cases.NAMES)
def test_the_kernels_loop_on_the_cpu_agrees_with_the_restatement(name, tmp_path):
    """test_pose_graph_calib_cpp's comparison: the first linearisation, then the result -- poses within 1e-9 m and 1e-9 of the
    restatement's direct solve, the same stop reason, counts and damping -- then the report at the result"""
    g, want, st = cases.reference(name)
    v = base.probe_vector(len(g["poses"]))
    poses, stats, report, lin, _ = host_solve(g, tmp_path, v)
    cases.check_stage_parity(g, lin)
    dt, dr = base.pose_difference(poses, want)
    print(name, "difference", dt, dr, stats, "restatement", st["stop"], st["accepted"], st["rejected"])
    assert dt < 1e-9 and dr < 1e-9
    base.check_costs(stats, st)
    assert (stats["stop_reason"], stats["accepted_steps"], stats["rejected_steps"], stats["damping"]) == (st["stop"], st["accepted"], st["rejected"], st["damping"])
    assert stats["pcg_max_iterations"] < 12 * calib.non_chain_edges(g) + 64
    fx = np.asarray(g["fixed"]).astype(bool)
    assert (poses[fx] == g["poses"][fx]).all()
    robust_cases.check_report_parity(g, report, pgi.report(g, want))
    assert abs(report[2].sum() - stats["final_cost"]) <= 1e-12 * max(stats["final_cost"], 1e-300)


def test_edges_that_do_not_see_x_let_the_points_decide_it(tmp_path):
    """the case that shows the point: with sigma edges the nodes end between the chain and their POINT targets, with edges that are
    weak along x within 5 cm of the targets"""
    v = np.zeros((6, 6))
    plain = host_solve(cases.graph("chain6_sigma"), tmp_path, v)[0]
    weak = host_solve(cases.graph("chain6_weak_x"), tmp_path, v)[0]
    print("distance from the POINT targets along x: sigma edges", cases.x_miss(plain), "weak-x edges", cases.x_miss(weak))
    assert cases.x_miss(weak).max() < 0.05
    assert cases.x_miss(plain).max() > 0.05
    assert np.abs(weak[:, 1:3, 3]).max() < 1e-9 and np.abs(plain[:, 1:3, 3]).max() < 1e-9      # nothing pulls across


def test_arrays_that_name_no_information_change_no_bit(tmp_path):
    """info_index all -1, and no arrays at all: the bytes of test_pose_graph_calib's solve of the same graph"""
    from test_pose_graph_calib_cpp import host_solve as calib_solve
    g = calib_cases.graph("ring16_free")
    v = base.probe_vector(len(g["poses"]))
    want = calib_solve(g, tmp_path, v, g["huber"])[4]
    gi = pgi.with_information(g, [None] * len(g["kinds"]))
    assert host_solve(gi, tmp_path, v, info="none")[4] == want
    assert host_solve(gi, tmp_path, v, info=None)[4] == want


def test_a_diagonal_information_is_the_sigma_form(tmp_path):
    g = cases.graph("ring16_diag")
    v = base.probe_vector(len(g["poses"]))
    sigma_form = host_solve(g, tmp_path, v, info=None)
    info_form = host_solve(g, tmp_path, v)
    dt, dr = base.pose_difference(sigma_form[0], info_form[0])
    print("sigma form against L = diag(1 / sigma):", dt, dr)
    assert dt <= 1e-12 and dr <= 1e-12
    assert sigma_form[1]["stop_reason"] == info_form[1]["stop_reason"] and sigma_form[1]["accepted_steps"] == info_form[1]["accepted_steps"]
