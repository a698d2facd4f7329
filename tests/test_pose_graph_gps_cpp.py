"""The GPS factors without a GPU: the headers compile alone; tests/cpp/test_pose_graph_gps.cc `host` checks PoseGraph's arrays with the
frame vertex last, the plan's counts and Submap's ENU; its `solve` mode runs the kernel's own loop (csrc/pose_graph_kernel.h), compiled
for the CPU as one thread, over the GPS graphs the device is tested on, against tests/pose_graph_gps_ref.py -- the same code the device
runs; its `isam host` mode runs IsamOptimizer's GPS bookkeeping through the Solver hook on hand-made frames, compared with the
restated rule (pose_graph_gps_ref.gps_rule)."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import pose_graph_cases as base
import pose_graph_gps_cases as cases
import pose_graph_gps_ref as gps
import pose_graph_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_pose_graph_gps.cc")


def _build_exe():
    from staticmapping_amd import build
    lib = build.build()
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "test_pose_graph_gps")
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
    for header, body in (("smhip/pose_graph.h", "smhip::back_end::PoseGraph g; g.SetFrameVertex(smhip::back_end::Matrix4d::Identity(), smhip::back_end::GpsCoordPriorSigmas()); return g.NodeCount();"),
                         ("smhip/submap.h", "smhip::builder::Submap s{smhip::builder::SubmapOptions()}; return s.HasGps();"),
                         ("smhip/back_end.h", "smhip::back_end::LoopFrame f; return f.has_enu;")):
        alone = tmp_path / "alone.cc"
        alone.write_text('#include "%s"\nint main() { %s }\n' % (header, body))
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(alone)])


def test_graph_arrays_plan_counts_and_submap_enu_on_the_host():
    out = subprocess.run([_build_exe(), "host"], text=True, capture_output=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout


def _pack12(X):
    return np.concatenate([X[:, :3, :3].reshape(len(X), 9), X[:, :3, 3]], axis=1)


def host_solve(g, tmp_path, v, max_iterations=50):
    """the kernel's loop on the CPU: (poses [N, 4, 4], stats dict, the first linearisation as staticmapping_amd.pose_graph.last gives it)"""
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
    stats = dict(initial_cost=od[0], final_cost=od[1], damping=od[2], stop_reason=oi[0], iterations=oi[1], accepted_steps=oi[2], rejected_steps=oi[3],
                 pcg_iterations=oi[4], pcg_max_iterations=oi[5])
    lin = dict(r=take(m, 6), A=take(m, 6, 6), B=take(m, 6, 6), g=take(n, 6), minv_v=take(n, 6))
    assert at[0] == len(a)
    return poses, stats, lin


GRAPHS = ["alone", "drive240", "chain1_all", "chain2_last", "chain4_second", "chain23_all", "chain62_second", "chain63_all", "chain64_last", "chain64_all"]


@pytest.mark.parametrize("name", GRAPHS)
def test_the_kernels_loop_on_the_cpu_agrees_with_the_restatement(name, tmp_path):
    """Stage by stage (cases.check_stage_parity), then the result: poses within 1e-9 m and 1e-9 of the restatement's direct solve, the
    same stop reason, counts and damping, every iteration count below its cap."""
    g, want, st = cases.reference(name)
    v = base.probe_vector(len(g["poses"]))
    poses, stats, lin = host_solve(g, tmp_path, v, max_iterations=100 if name == "alone" else 50)
    cases.check_stage_parity(g, lin, v)
    dt, dr = base.pose_difference(poses, want)
    print(name, "difference", dt, dr, "gradient ratio", cases.gradient_ratio(g, poses), stats, "restatement", st["stop"], st["accepted"], st["rejected"])
    assert dt < 1e-9 and dr < 1e-9
    base.check_costs(stats, st)
    assert (stats["stop_reason"], stats["accepted_steps"], stats["rejected_steps"], stats["damping"]) == (st["stop"], st["accepted"], st["rejected"], st["damping"])
    assert 0 < stats["pcg_max_iterations"] < 12 * gps.non_chain_edges(g) + 64
    fx = np.asarray(g["fixed"]).astype(bool)
    assert (poses[fx] == g["poses"][fx]).all()


# ---- IsamOptimizer's bookkeeping --------------------------------------------------------------------------------------------------

def quarter_drive(n=40, turn=0.75 * 2 * np.pi, radius=120.0, drift_from=None, seed=11):
    """n submaps on three quarters of a circle that never returns (neighbours 14 m apart, no frame within 25 m of one 15 older).
    Returns (truth [n, 4, 4], fed [n, 4, 4]: the truth, from drift_from on moved by 0.5 m / 0.5 degrees)."""
    truth = np.stack([ref.make_pose((0.0, 0.0, a + 0.5 * np.pi), (radius * np.cos(a), radius * np.sin(a), 0.0)) for a in np.linspace(0.0, turn, n)])
    fed = truth.copy()
    if drift_from is not None:
        drift = ref.make_pose((0.0, 0.0, np.deg2rad(0.5)), (0.3, 0.4, 0.0))
        fed[drift_from:] = drift @ truth[drift_from:]
    return truth, fed


def write_isam_input(path, fed, enu, has, use_gps=1, init_num=25, sample_step=1, init_angle=1.6, extrinsic=0, lever=cases.LEVER):
    with open(path, "w") as fh:
        fh.write("%d %d %d %.17g %d\n%.17g %.17g %.17g\n%d\n" % (use_gps, init_num, sample_step, init_angle, extrinsic, *lever, len(fed)))
        for P, e, h in zip(fed, enu, has):
            fh.write(" ".join("%.17g" % x for x in P.ravel()) + " %d %.17g %.17g %.17g\n" % (int(h), *e))


def run_isam(where, tmp_path, fed, enu, has, **options):
    src = tmp_path / "isam.txt"
    write_isam_input(src, fed, enu, has, **options)
    out = subprocess.run([_build_exe(), "isam", where, str(src)], text=True, capture_output=True, timeout=300)
    if out.returncode != 0:
        return out.returncode, out.stderr
    return 0, json.loads(out.stdout.strip().splitlines()[-1])


def check_against_the_rule(res, has, **rule):
    want = gps.gps_rule(has, res["angles"], **rule)
    assert res["factor_indices"] == want["factors"], (res["factor_indices"], want)
    assert res["gps_factors"] == len(want["factors"])
    assert res["cached"] == len(want["cached"])
    return want


def test_isam_optimizer_gps_bookkeeping_through_the_solver_hook(tmp_path):
    truth, fed = quarter_drive()
    enu = cases.enu_of(truth, 11)
    every = [True] * len(fed)
    # the turn passes 1.6 rad at frame 14 (0.121 rad a frame)
    code, res = run_isam("host", tmp_path, fed, enu, every, init_num=60)                    # below init_num: everything cached, no factor
    assert code == 0 and res["ok"]
    want = check_against_the_rule(res, every, init_num=60)
    assert want["trigger"] is None and res["gps_factors"] == 0 and res["cached"] == 40 and np.abs(np.array(res["gps_coord"]).reshape(4, 4) - np.eye(4)).max() == 0.0
    code, res = run_isam("host", tmp_path, fed[:12], enu[:12], every[:12], init_num=5)      # enough frames, but below the angle
    assert code == 0 and res["ok"]
    want = check_against_the_rule(res, every[:12], init_num=5)
    assert want["trigger"] is None and max(res["angles"]) < 1.6 and res["cached"] == 12
    code, res = run_isam("host", tmp_path, fed, enu, every)                                 # the defaults: 25 cached, the trigger frame skipped
    assert code == 0 and res["ok"]
    want = check_against_the_rule(res, every)
    assert want["trigger"] == 25 and 25 not in res["factor_indices"] and res["factor_indices"] == list(range(25)) + list(range(26, 40))
    assert res["nodes"] == 41
    G = np.array(res["gps_coord"]).reshape(4, 4)
    assert np.linalg.norm(G[:3, 3] - cases.G[:3, 3]) < 0.30 and np.linalg.norm(ref.log_so3(cases.G[:3, :3].T @ G[:3, :3])) < 0.014
    assert np.abs(G[:3, :3].T @ G[:3, :3] - np.eye(3)).max() < 1e-12
    code, res = run_isam("host", tmp_path, fed, enu, every, init_num=10, sample_step=2)     # the angle decides (frame 14), then every second frame
    assert code == 0 and res["ok"]
    want = check_against_the_rule(res, every, init_num=10, sample_step=2)
    assert 10 < want["trigger"] < 25 and all(k % 2 == 0 for k in want["sampled"]) and len(want["sampled"]) > 5
    has = [k % 3 != 1 and k != 25 for k in range(40)]                                       # frames without a fix, the would-be trigger among them
    code, res = run_isam("host", tmp_path, fed, enu, has, init_num=10)
    assert code == 0 and res["ok"]
    want = check_against_the_rule(res, has, init_num=10)
    assert all(has[k] for k in res["factor_indices"]) and want["trigger"] is not None and has[want["trigger"]]
    code, res = run_isam("host", tmp_path, fed, enu, every, use_gps=0)                      # without use_gps nothing happens
    assert code == 0 and res["gps_factors"] == 0 and res["cached"] == 0 and res["nodes"] == 40
    code, text = run_isam("host", tmp_path, fed, enu, every, extrinsic=1)                   # refused with a message
    assert code == 4 and "enable_extrinsic_calib" in text
