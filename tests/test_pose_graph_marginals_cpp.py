"""The marginal covariances without a GPU: tests/cpp/test_pose_graph_marginals.cc runs the kernel header's own per-query routine
(csrc/pose_graph_kernel.h, marginal_query), compiled for the CPU as one thread, over the graphs of tests/pose_graph_marginals_cases.py
against tests/pose_graph_marginals_ref.py -- the same code the device runs; its `host` mode checks the refusals (the NUMERIC flag among
them), probe 3's NUMERIC ending and the dealing of queries to workgroups."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pose_graph_calib_ref as calib
import pose_graph_info_cases as info_cases
import pose_graph_marginals_cases as cases
import pose_graph_marginals_ref as mref
from test_pose_graph_robust_cpp import _pack12

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_pose_graph_marginals.cc")
# The worst difference of the routine's cov and blocks to pcg_columns', relative to the largest entry of the query's covariances, over
# every graph of the cases file, all nodes queried: 1.24e-10 (n63, cond(H) 9.0e8; 1.0e-10 on missing_chain_edge, 2.6e-11 on n64, 4.8e-13
# on circle240, 3.2e-13 on gps_chain23; 2e-14 and below elsewhere), measured by test_the_routine_on_the_cpu_agrees_with_the_restatement, which prints every
# graph's figure.  Both sides run the same iteration with the same operators in f64; they differ in the order of their sums, which
# cond(H) amplifies, and -- on the three graphs that lead -- by up to one iteration in where a column stops.  The bound is ten times the
# figure on every graph.
WORST_MEASURED = 1.24e-10


def bound(H):
    return 10.0 * WORST_MEASURED


def _build_exe():
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "test_pose_graph_marginals")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "include", "smhip.h"), os.path.join(ROOT, "staticmapping_amd", "csrc", "pose_graph_kernel.h"),
            os.path.join(ROOT, "staticmapping_amd", "csrc", "pose_graph_plan.h")]
    if (not os.path.exists(exe)) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe])
    return exe


def kernel_arrays(g, poses):
    """the graph as the kernel's arrays: dict(cur [n, 12], Z [m, 12], sinv [m, 6], huber [m] | None, fixed, ij, kind | None, info_index | None,
    sqrt_info [K, 36] | None)"""
    if "kinds" not in g:
        m = len(g["edges"])
        sig = np.broadcast_to(np.asarray(g.get("sigmas", mref.ref.DEFAULT_SIGMAS), np.float64), (m, 6))
        return dict(cur=_pack12(np.asarray(poses)), Z=_pack12(g["Z"]), sinv=1.0 / sig, huber=None, fixed=np.asarray(g["fixed"]), ij=g["edges"], kind=None,
                    info_index=None, sqrt_info=None)
    m = len(g["kinds"])
    Z, sinv = np.zeros((m, 12)), np.zeros((m, 6))
    for k in range(m):
        if g["kinds"][k] == calib.POINT:
            Z[k, :6], sinv[k, :3] = g["data"][k, :6], 1.0 / g["sigmas"][k, :3]
        else:
            Z[k], sinv[k] = _pack12(g["data"][k].reshape(1, 4, 4).transpose(0, 2, 1))[0], 1.0 / g["sigmas"][k]
    index, rows = info_cases.abi_arrays(g) if g.get("L") is not None else (None, None)
    return dict(cur=_pack12(np.asarray(poses)), Z=Z, sinv=sinv, huber=g.get("huber"), fixed=np.asarray(g["fixed"]), ij=g["ij"], kind=g["kinds"],
                info_index=index, sqrt_info=rows)


def host_marginals(g, poses, query, rows, tmp_path, workgroups=1, cap=None):
    """the kernel's routine on the CPU: (ok, cov [Q, 6, 6], blocks [Q, R, 6, 6], info [Q, 3]: iterations, longest, capped)"""
    a = kernel_arrays(g, poses)
    n, m, Q, R = len(a["cur"]), len(a["Z"]), len(query), len(rows)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as fh:
        fh.write(struct.pack("<9i", n, m, Q, R, mref.pcg_cap(g) if cap is None else cap, workgroups, 0 if a["kind"] is None else 1,
                             0 if a["huber"] is None else 1, -1 if a["info_index"] is None else len(a["sqrt_info"])))
        for key in ("cur", "Z", "sinv", "huber", "sqrt_info"):
            if a[key] is not None:
                fh.write(np.asarray(a[key]).astype("<f8").tobytes())
        for key in ("fixed", "ij", "kind", "info_index"):
            if a[key] is not None:
                fh.write(np.asarray(a[key]).astype("<i4").tobytes())
        fh.write(np.asarray(query, "<i4").tobytes())
        fh.write(np.asarray(rows, "<i4").tobytes())
    out = subprocess.run([_build_exe(), "solve", str(src), str(dst)], text=True, capture_output=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(dst, "<f8")
    if raw[0] == 0.0:
        return False, None, None, None
    assert len(raw) == 1 + 36 * Q + 36 * Q * R + 3 * Q
    return True, raw[1:1 + 36 * Q].reshape(Q, 6, 6), raw[1 + 36 * Q:1 + 36 * Q * (1 + R)].reshape(Q, R, 6, 6), raw[1 + 36 * Q * (1 + R):].reshape(Q, 3).astype(int)


def test_the_source_compiles_without_a_gpu():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), SRC])


def test_refusals_the_numeric_flag_and_the_dealing_on_the_host():
    out = subprocess.run([_build_exe(), "host"], text=True, capture_output=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout


@pytest.mark.parametrize("which", ["two_nodes", "prior_alone"])
def test_the_analytic_cases(which, tmp_path):
    g = cases.two_nodes() if which == "two_nodes" else cases.prior_alone()
    k = len(g["poses"]) - 1
    ok, cov, _, info = host_marginals(g, g["poses"], [k], [], tmp_path)
    want = np.diag(cases.ANALYTIC_SIGMAS ** 2)
    print(which, np.abs(cov[0] - want).max(), info)
    assert ok and (np.abs(cov[0] - want) <= 1e-12 * np.abs(want).max()).all() and (np.abs(np.diag(cov[0]) - np.diag(want)) <= 1e-12 * np.diag(want)).all()


@pytest.mark.parametrize("name", cases.ALL)
def test_the_routine_on_the_cpu_agrees_with_the_restatement(name, tmp_path):
    """every node queried, every node a row, over two workgroups: cov and blocks within ten times the recorded worst case of
    pcg_columns' and within the CPU bound of the dense inverse; no column capped, every count below the cap; the longest column
    within one iteration of the restatement's longest and the total within one per column of its total"""
    g, poses = cases.optimised(name)
    n = len(poses)
    q = list(range(n))
    H, fixed, cap, want, D = cases.restated(name)
    wcov, wblocks = mref.covariances(want["x"], fixed, q, q)
    dcov, dblocks = mref.covariances(D, fixed, q, q)
    ok, cov, blocks, info = host_marginals(g, poses, q, q, tmp_path, workgroups=2)
    assert ok
    scale = np.abs(wcov).max()
    rel = max(np.abs(cov - wcov).max(), np.abs(blocks - wblocks).max()) / scale
    rel_dense = max(np.abs(cov - dcov).max(), np.abs(blocks - dblocks).max()) / scale
    its = want["iterations"].sum(axis=1)
    print(name, "cond %.3g" % np.linalg.cond(H), "against pcg_columns %.3g" % rel, "bound %.3g" % bound(H), "against dense %.3g" % rel_dense, "bound %.3g" % mref.bound(H),
          "iterations", info[:, 0].sum(), "restatement", its.sum())
    assert rel <= bound(H) and rel_dense <= mref.bound(H)
    worst = np.abs(info[:, 1] - want["iterations"].max(axis=1)).max()
    print(name, "longest column against the restatement's: largest difference", worst)
    assert (info[:, 2] == 0).all() and (info[fixed] == 0).all() and (info[~fixed, 1] >= 1).all() and info[:, 1].max() < cap
    assert abs(info[:, 1].max() - want["iterations"].max()) <= 1 and abs(info[:, 0].sum() - its.sum()) <= 6 * int((~fixed).sum())
    assert (cov[fixed] == 0.0).all() and (blocks[fixed] == 0.0).all() and (blocks[:, fixed] == 0.0).all()
    assert (cov == cov.transpose(0, 2, 1)).all()


def test_a_cap_below_what_the_columns_need_raises_the_flag(tmp_path):
    g, poses = cases.optimised("circle64")
    ok, _, _, info = host_marginals(g, poses, [0, 10], [], tmp_path, cap=5)
    assert ok and info.tolist() == [[0, 0, 0], [30, 5, 1]]


def test_isam_optimizers_marginal_calls_on_the_host():
    """tests/cpp/test_pose_graph_marginals_api.cc: IsamOptimizer::MarginalCovariance, JointMarginalCovariance, CalibCovariance and
    GpsCoordCovariance with SetSolver / SetMarginalizer in place of the device, and PoseGraph::WorldPositionCovariance"""
    from staticmapping_amd import build
    lib = build.build()
    src = os.path.join(ROOT, "tests", "cpp", "test_pose_graph_marginals_api.cc")
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "test_pose_graph_marginals_api")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = [src, lib, os.path.join(ROOT, "include", "smhip.h")] + [os.path.join(ROOT, "include", "smhip", h) for h in ("pose_graph.h", "back_end.h", "edge_information.h", "submap.h")]
    if (not os.path.exists(exe)) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", os.path.dirname(lib), "-lsmhip", "-ldl",
                               "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    out = subprocess.run([exe], text=True, capture_output=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
