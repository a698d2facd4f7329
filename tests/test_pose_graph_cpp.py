"""The pose-graph optimiser without a GPU: include/smhip/pose_graph.h compiles alone; tests/cpp/test_pose_graph.cc `host` checks
every refusal of smhip_pose_graph_optimize's host half (directly and through smhip_pose_graph_plan), the CSR order,
Submap::UpdateInnerFramePose and IsamOptimizer::AddFrame's bookkeeping on hand-made detector results; its `solve` mode runs the
kernel's own loop (csrc/pose_graph_kernel.h), compiled for the CPU as one thread, over the graphs the device is tested on and
is compared with tests/pose_graph_ref.py -- the same code the device runs, checked where a debugger can reach it."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pose_graph_cases as cases
import pose_graph_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_pose_graph.cc")


def _build_exe():
    from staticmapping_amd import build
    lib = build.build()
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "test_pose_graph")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = [os.path.join(ROOT, "include", "smhip", h) for h in ("pose_graph.h", "submap.h", "back_end.h", "m2dp.h", "registrator.h", "filters.h")]
    deps += [os.path.join(ROOT, "include", "smhip.h"), os.path.join(ROOT, "staticmapping_amd", "csrc", "pose_graph_kernel.h"),
             os.path.join(ROOT, "staticmapping_amd", "csrc", "pose_graph_plan.h"), SRC, lib]
    if (not os.path.exists(exe)) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                               "-L", os.path.dirname(lib), "-lsmhip", "-Wl,-rpath," + os.path.dirname(lib),
                               "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_headers_compile_without_a_gpu(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), SRC])
    alone = tmp_path / "pose_graph_alone.cc"
    alone.write_text('#include "smhip/pose_graph.h"\nint main() { smhip::back_end::PoseGraph g; return g.VertexCount(); }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(alone)])


def test_refusals_csr_inner_frame_poses_and_bookkeeping_on_the_host():
    out = subprocess.run([_build_exe(), "host"], text=True, capture_output=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout


def _pack12(X):
    return np.concatenate([X[:, :3, :3].reshape(len(X), 9), X[:, :3, 3]], axis=1)


def host_solve(g, tmp_path, v, max_iterations=50):
    """the kernel's loop on the CPU: (poses [N, 4, 4], stats dict, the first linearisation as staticmapping_amd.pose_graph.last gives it)"""
    n, m = len(g["poses"]), len(g["edges"])
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as fh:
        fh.write(struct.pack("<ii", n, m))
        fh.write(_pack12(g["poses"]).astype("<f8").tobytes())
        fh.write(_pack12(g["Z"]).astype("<f8").tobytes())
        fh.write(np.tile(1.0 / ref.DEFAULT_SIGMAS, (m, 1)).astype("<f8").tobytes())
        fh.write(np.asarray(v, "<f8").tobytes())
        fh.write(g["fixed"].astype("<i4").tobytes())
        fh.write(g["edges"].astype("<i4").tobytes())
        fh.write(struct.pack("<i", max_iterations))
    out = subprocess.run([_build_exe(), "solve", str(src), str(dst)], text=True, capture_output=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    a = np.fromfile(dst, "<f8")
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
    stats = dict(initial_cost=od[0], final_cost=od[1], stop_reason=oi[0], iterations=oi[1], accepted_steps=oi[2], rejected_steps=oi[3],
                 pcg_iterations=oi[4], pcg_max_iterations=oi[5])
    lin = dict(r=take(m, 6), A=take(m, 6, 6), B=take(m, 6, 6), g=take(n, 6), minv_v=take(n, 6))
    assert at[0] == len(a)
    return poses, stats, lin


ALL = sorted({**cases.stage_cases(), **cases.angle_cases(), **cases.circle_cases()})


@pytest.mark.parametrize("name", ALL)
def test_the_kernels_loop_on_the_cpu_agrees_with_the_restatement(name, tmp_path):
    """Stage by stage (cases.check_stage_parity), then the result: poses within 1e-9 m and 1e-9 of the restatement's direct solve
    (the bound the device is held to before a difference counts as a finding), the restatement's gradient at them below 1e-9 of the
    one at the start, the same stop reason, every count below its cap."""
    g, want, st = cases.reference(name)
    v = cases.probe_vector(len(g["poses"]))
    poses, stats, lin = host_solve(g, tmp_path, v)
    cases.check_stage_parity(g, lin, v)
    dt, dr = cases.pose_difference(poses, want)
    ratio = cases.gradient_ratio(g, poses)
    print(name, "difference", dt, dr, "gradient ratio", ratio, stats, "restatement", st["stop"], st["accepted"], st["rejected"])
    assert dt < 1e-9 and dr < 1e-9
    if name not in cases.angle_cases():         # (near_zero starts at its minimum: noise over noise.  near_pi and triangle keep a large
        assert ratio < 1e-9                     # residual, where Gauss-Newton converges linearly and the cost criterion stops it first.)
    cases.check_costs(stats, st)
    assert stats["stop_reason"] == st["stop"] and stats["accepted_steps"] == st["accepted"] and stats["rejected_steps"] == st["rejected"]
    assert stats["iterations"] == stats["accepted_steps"] + stats["rejected_steps"] < 50
    assert stats["pcg_max_iterations"] < 12 * ref.non_chain_edges(g["edges"]) + 64
    assert (poses[g["fixed"].astype(bool)] == g["poses"][g["fixed"].astype(bool)]).all()
