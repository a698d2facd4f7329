"""The device's marginal covariances (smhip_pose_graph_marginals: one launch that linearises and factors, one multi-workgroup launch
that solves six columns per queried node) against tests/pose_graph_marginals_ref.py, on the graphs of
tests/pose_graph_marginals_cases.py, each after its own optimise entry -- all five entries are covered.  The restatement linearises at
the poses the device returned, which are the poses the device linearises at, so what is compared is the solve and not the optimiser."""
import ctypes

import numpy as np
import pytest

import pose_graph_cases as base
import pose_graph_marginals_cases as cases
import pose_graph_marginals_ref as mref
import pose_graph_ref as ref
from staticmapping_amd import IcpFastHip, SmhipError, _capi, pose_graph

pytestmark = pytest.mark.gpu

NOT_READY, INVALID, NO_MATCH, CAPACITY = 4, 1, 6, 7
# The worst difference of the device's cov and blocks to pcg_columns', relative to the largest entry of the call's covariances, on the
# first run on the MI355X over every graph below: 1.18e-10, on n63 (cond(H) 9.0e8; next 4.0e-11 on missing_chain_edge and 2.1e-11 on
# n64 -- the three graphs on which a column may stop one iteration apart -- then 3.7e-13 on gps_chain23 and 2.7e-13 on circle240; 1e-14
# and below elsewhere).  The bound is ten times that on every graph (the same routine on the CPU: 1.24e-10 on the same graph).
DEVICE_MEASURED = 1.18e-10


# ... and of the 1 500-node graph's 300 queries to scipy's sparse LU on that run: 3.98e-7 (cond(H) 3.7e12); asserted within ten times
# that, beside the formula's 8e-2, which at this cond is only an upper limit
LARGE_MEASURED = 3.98e-7


def device_bound(H):
    return 10.0 * DEVICE_MEASURED


@pytest.fixture(scope="module")
def handle():
    m = IcpFastHip(device=0, max_source_points=1024, max_target_points=1024)
    yield m
    m.close()


def optimise(handle, name, g):
    """the graph through the entry of its kind: (poses, stats)"""
    if "kinds" not in g:
        return pose_graph.optimize(handle, g["poses"], g["edges"], g["Z"], fixed=g["fixed"], sigmas=g.get("sigmas"))
    args = (handle, g["poses"], g["kinds"], g["ij"], g["data"])
    kw = dict(fixed=g["fixed"], sigmas=g["sigmas"])
    if name == "info_ring16":
        return pose_graph.optimize_info(*args, **kw, huber=g.get("huber"), sqrt_information=g["L"])
    if name == "calib_ring16":
        return pose_graph.optimize_calib(*args, **kw, huber=g.get("huber"))
    if name == "robust16":
        return pose_graph.optimize_robust(*args, **kw, huber=g["huber"])
    return pose_graph.optimize_factors(*args, **kw)


def _queries(n):
    """every node of a small graph; of a large one every tenth node, the first three and the last three"""
    return list(range(n)) if n <= 65 else sorted(set(range(0, n, 10)) | {1, 2, n - 3, n - 2, n - 1})


@pytest.mark.parametrize("which", ["two_nodes", "prior_alone"])
def test_the_analytic_cases(handle, which):
    """Sigma = diag(sigma^2) to 1e-12 relative (tests/test_pose_graph_marginals_ref.py says why)"""
    g = cases.two_nodes() if which == "two_nodes" else cases.prior_alone()
    n = len(g["poses"])
    poses, _ = optimise(handle, which, g)
    assert np.abs(poses - g["poses"]).max() < 1e-12                      # it starts at its minimum
    cov, blocks, stats = pose_graph.marginals(handle, n, [n - 1], rows=[n - 1])
    want = np.diag(cases.ANALYTIC_SIGMAS ** 2)
    print(which, "worst difference", np.abs(cov[0] - want).max(), stats)
    assert (np.abs(cov[0] - want) <= 1e-12 * np.abs(want).max()).all() and (np.abs(np.diag(cov[0]) - np.diag(want)) <= 1e-12 * np.diag(want)).all()
    assert (np.abs(blocks[0, 0] - want) <= 1e-12 * np.abs(want).max()).all()
    assert stats["workgroups"] == 1 and 0 < stats["pcg_max_iterations"] < stats["pcg_cap"]


_SOLVED = {}


def solved(handle, name):
    """the graph optimised and queried on the device, and the restatement at the device's poses: computed once per graph"""
    if name not in _SOLVED:
        g, _ = cases.optimised(name)
        poses, ostats = optimise(handle, name, g)
        q = _queries(len(poses))
        cov, blocks, stats = pose_graph.marginals(handle, len(poses), q, rows=q)
        H, fixed, cap = mref.system(g, poses)
        _SOLVED[name] = dict(q=q, cov=cov, blocks=blocks, stats=stats, ostats=ostats, H=H, fixed=fixed, cap=cap, want=mref.pcg_columns(H, fixed, q, cap))
    return _SOLVED[name]


@pytest.mark.parametrize("name", cases.ALL)
def test_covariances_and_cross_blocks_against_the_restatement(handle, name):
    """cov and blocks within ten times the first run's worst difference of pcg_columns' (device_bound) and within the CPU bound of the
    dense inverse (pose_graph_marginals_ref.bound), both relative to the largest entry of the covariances; no column capped; zeros for
    fixed nodes, exact symmetry, positive definite."""
    s = solved(handle, name)
    q, cov, blocks, stats, H, fixed, want = s["q"], s["cov"], s["blocks"], s["stats"], s["H"], s["fixed"], s["want"]
    wcov, wblocks = mref.covariances(want["x"], fixed, q, q)
    dcov, dblocks = mref.covariances(mref.dense_columns(mref.dense(H, fixed), q), fixed, q, q)
    scale = np.abs(wcov).max()
    rel = max(np.abs(cov - wcov).max(), np.abs(blocks - wblocks).max()) / scale
    rel_dense = max(np.abs(cov - dcov).max(), np.abs(blocks - dblocks).max()) / scale
    print(name, "nodes", len(fixed), "queries", len(q), "cond %.3g" % np.linalg.cond(H), "against pcg_columns %.3g" % rel, "bound %.3g" % device_bound(H),
          "against dense %.3g" % rel_dense, "bound %.3g" % mref.bound(H), stats)
    assert rel <= device_bound(H)
    assert rel_dense <= mref.bound(H)
    assert stats["pcg_cap"] == s["cap"] == s["ostats"]["pcg_cap"] and 0 < stats["pcg_max_iterations"] < s["cap"] and 1 <= stats["workgroups"] <= len(q)
    fq = fixed[q]
    assert (cov[fq] == 0.0).all() and (blocks[fq] == 0.0).all() and (blocks[:, fq] == 0.0).all()
    assert (cov == cov.transpose(0, 2, 1)).all()
    assert all((np.linalg.eigvalsh(c) > 0.0).all() for c in cov[~fq])


@pytest.mark.parametrize("name", cases.ALL)
def test_iteration_counts_equal_the_restatements(handle, name):
    """The longest column's count within one of the restatement's longest, the call's total within one per column of its total.

    Measured on the MI355X: eleven of the fifteen graphs take exactly the restatement's counts; on the other four, whose columns run
    17 to 37 iterations at cond(H) 5e7 .. 6e9 -- past what exact arithmetic would need, so that rounding decides the last iteration or
    two -- device against restatement, longest column / total: missing_chain_edge 36 / 7 815 against 37 / 8 007 (234 columns), n63
    17 / 5 458 against 17 / 5 553 (372), n64 26 / 9 423 against 26 / 9 436 (378), gps_chain23 19 / 2 357 against 19 / 2 376 (138).  That
    holds because the restatement uses the definition's own operators; through the assembled H and LAPACK's M^-1 it takes 40, 20, 32
    and 23 (tests/test_pose_graph_marginals_ref.py, test_what_the_kernels_operators_do_to_the_iteration_counts)."""
    s = solved(handle, name)
    stats, want = s["stats"], s["want"]
    free_columns = 6 * int((~s["fixed"][s["q"]]).sum())
    print(name, "device: longest", stats["pcg_max_iterations"], "total", stats["pcg_iterations"], "restatement: longest", want["iterations"].max(), "total",
          want["iterations"].sum(), "columns", free_columns)
    assert abs(stats["pcg_max_iterations"] - want["iterations"].max()) <= 1
    assert abs(stats["pcg_iterations"] - want["iterations"].sum()) <= free_columns


def test_fixed_nodes_and_transposed_cross_blocks(handle):
    g, _ = cases.optimised("fixed_in_the_middle")
    poses, _ = optimise(handle, "fixed_in_the_middle", g)
    n = len(poses)
    H, fixed, _ = mref.system(g, poses)
    assert fixed[0] and fixed[9]
    q = [9, 3, 20, 0, 12]
    cov, blocks, _ = pose_graph.marginals(handle, n, q, rows=q)
    assert (cov[0] == 0.0).all() and (cov[3] == 0.0).all()                               # a fixed node queried
    assert (blocks[:, 0] == 0.0).all() and (blocks[:, 3] == 0.0).all()                   # a fixed row
    assert (blocks[0] == 0.0).all() and (blocks[3] == 0.0).all()
    scale = np.abs(cov).max()
    for a in (1, 2, 4):
        for b in (1, 2, 4):                                                              # block(i | query j) = block(j | query i)^T
            assert np.abs(blocks[a, b] - blocks[b, a].T).max() <= mref.bound(H) * scale
        assert np.abs(blocks[a, a] - cov[a]).max() <= mref.bound(H) * scale              # the diagonal cross block is the unsymmetrised X


def test_the_same_bits_whatever_the_grid_and_whatever_else_is_queried(handle):
    g, _ = cases.optimised("circle64")
    optimise(handle, "circle64", g)
    n = len(g["poses"])
    every = list(range(n))
    rows = [0, 7, 63]
    cov, blocks, stats = pose_graph.marginals(handle, n, every, rows=rows)
    again = pose_graph.marginals(handle, n, every, rows=rows)
    assert again[0].tobytes() == cov.tobytes() and again[1].tobytes() == blocks.tobytes() and again[2] == stats
    assert stats["workgroups"] == 64
    for wg in (1, 2, 3):
        c, b, s = pose_graph.marginals(handle, n, every, rows=rows, max_workgroups=wg)
        assert s["workgroups"] == wg and c.tobytes() == cov.tobytes() and b.tobytes() == blocks.tobytes()
        assert (s["pcg_iterations"], s["pcg_max_iterations"]) == (stats["pcg_iterations"], stats["pcg_max_iterations"])
    for k in (1, 40, 63):                                                                # a node queried alone
        c, b, _ = pose_graph.marginals(handle, n, [k], rows=rows)
        assert c[0].tobytes() == cov[k].tobytes() and b[0].tobytes() == blocks[k].tobytes()
    five = [62, 5, 5, 0, 33]                                                             # the grid stride with a remainder, a repeat, the held node
    c, b, s = pose_graph.marginals(handle, n, five, rows=rows, max_workgroups=2)
    assert s["workgroups"] == 2
    for at, k in enumerate(five):
        assert c[at].tobytes() == cov[k].tobytes() and b[at].tobytes() == blocks[k].tobytes()
    c, b, _ = pose_graph.marginals(handle, n, five)                                      # no rows at all
    assert b is None and all(c[at].tobytes() == cov[k].tobytes() for at, k in enumerate(five))


def test_more_nodes_than_threads_and_more_queries_than_workgroups(handle):
    """pose_graph_cases.large_circle: 1 500 nodes, so every strided loop of a solve takes a second round, and 300 queries, more than
    the device has CUs, so workgroups take a second query.  Against scipy's sparse LU of the same H, column by column: the bound is
    pose_graph_marginals_ref.bound's with cond(H) from the extreme eigenvalues (H is symmetric positive definite)."""
    import scipy.sparse.linalg as spl
    g, _, _ = base.large_circle()
    poses, _ = optimise(handle, "large", g)
    n = len(poses)
    q = [int(k) for k in np.linspace(0, n - 1, 300).round()]
    rows = [1, 750, n - 1]
    cov, blocks, stats = pose_graph.marginals(handle, n, q, rows=rows)
    edges = [(int(i), int(j)) for i, j in g["edges"]]
    fixed = g["fixed"].astype(bool)
    H, _ = ref.assemble_sparse(n, fixed, edges, *ref.linearize(poses, edges, g["Z"]))
    lu = spl.splu(H.tocsc())
    big = float(spl.eigsh(H, k=1, which="LA", return_eigenvectors=False)[0])
    small = float(spl.eigsh(H, k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0])
    cond = big / small
    rhs = np.zeros((6 * n, 6 * len(q)))
    for at, k in enumerate(q):
        if not fixed[k]:
            rhs[6 * k:6 * k + 6, 6 * at:6 * at + 6] = np.eye(6)
    X = lu.solve(rhs)
    x = np.stack([X[:, 6 * at:6 * at + 6] for at in range(len(q))])
    wcov, wblocks = mref.covariances(x, fixed, q, rows)
    scale = np.abs(wcov).max()
    rel = max(np.abs(cov - wcov).max(), np.abs(blocks - wblocks).max()) / scale
    bound = 100.0 * mref.EPS * cond + 10.0 * mref.TRUNCATION_MEASURED
    print("1 500 nodes, 300 queries: cond %.3g" % cond, "relative difference %.3g" % rel, "bound %.3g" % bound, stats)
    assert rel <= bound
    assert rel <= 10.0 * LARGE_MEASURED
    assert stats["workgroups"] < 300 and 0 < stats["pcg_max_iterations"] < stats["pcg_cap"] == 12 * 6 + 64
    assert (cov[0] == 0.0).all() and (cov == cov.transpose(0, 2, 1)).all()


def test_a_marginals_call_leaves_the_poses_and_the_hooks_alone(handle):
    g, _ = cases.optimised("robust16")
    poses, _ = optimise(handle, "robust16", g)
    n, m = len(poses), len(g["kinds"])
    v = base.probe_vector(n)
    before, report = pose_graph.last(handle, n, m, v), pose_graph.last_robust(handle, m)
    cov, _, _ = pose_graph.marginals(handle, n, list(range(n)), rows=[1, 2])
    after, report2 = pose_graph.last(handle, n, m, v), pose_graph.last_robust(handle, m)
    assert all(before[key].tobytes() == after[key].tobytes() for key in before)
    assert all(report[key].tobytes() == report2[key].tobytes() for key in report)        # the report is at cur: cur has its bits
    assert (report["weight"] < 1.0).any()
    assert pose_graph.marginals(handle, n, list(range(n)))[0].tobytes() == cov.tobytes() # ... and after the hooks the same marginals
    again, _ = optimise(handle, "robust16", g)
    assert again.tobytes() == poses.tobytes()


def _raw(handle, n_nodes, query, cov, rows=None, blocks=None, n_query=None, n_rows=None, max_workgroups=0):
    """the ABI itself, on the caller's arrays: (status, stats)"""
    o = _capi.PoseGraphMarginalsOptions()
    o.max_workgroups = max_workgroups
    st = _capi.PoseGraphMarginalsStats(-7, -7, -7, -7)
    ptr = lambda a, kind: None if a is None else a.ctypes.data_as(kind)
    s = handle._lib.smhip_pose_graph_marginals(handle._h, n_nodes, len(query) if n_query is None else n_query, ptr(query, _capi.c_int32_p), ptr(cov, _capi.c_double_p),
                                               (0 if rows is None else len(rows)) if n_rows is None else n_rows, ptr(rows, _capi.c_int32_p), ptr(blocks, _capi.c_double_p),
                                               ctypes.byref(o), ctypes.byref(st))
    return s, (st.workgroups, st.pcg_iterations, st.pcg_max_iterations, st.pcg_cap)


def test_refusals_write_nothing_and_leave_the_handle():
    fresh = IcpFastHip(device=0, max_source_points=1024, max_target_points=1024)
    try:
        q, rows = np.array([1, 2, 3], np.int32), np.array([0, 5], np.int32)
        cov, blocks = np.full((3, 36), 7.5), np.full((3, 2, 36), 7.5)

        def refused(want, *a, **kw):
            s, st = _raw(fresh, *a, **kw)
            assert s == want, (s, want, fresh._lib.smhip_last_error(fresh._h))
            assert st == (-7, -7, -7, -7) and (cov == 7.5).all() and (blocks == 7.5).all()
        refused(NOT_READY, 64, q, cov)                                                   # no optimise call yet
        g, _ = cases.optimised("circle64")
        poses, stats = optimise(fresh, "circle64", g)
        assert stats["pcg_cap"] == 100
        refused(INVALID, 63, q, cov)                                                     # not the last call's node count
        refused(INVALID, 64, q, cov, n_query=0)
        refused(INVALID, 64, None, cov, n_query=3)
        refused(INVALID, 64, q, None)
        refused(INVALID, 64, np.array([1, 64, 3], np.int32), cov)
        refused(INVALID, 64, np.array([1, -1, 3], np.int32), cov)
        refused(INVALID, 64, q, cov, rows=np.array([0, 64], np.int32), blocks=blocks)
        refused(INVALID, 64, q, cov, rows=None, blocks=blocks, n_rows=2)
        refused(INVALID, 64, q, cov, rows=rows, blocks=None)
        refused(INVALID, 64, q, cov, max_workgroups=-1)
        many = np.ones(334, np.int32)                                                    # one workgroup: 334 x 6 x 100 = 200 400 > 200 000
        room = np.full((334, 36), 7.5)
        s, st = _raw(fresh, 64, many, room, max_workgroups=1)
        assert s == CAPACITY and st == (-7, -7, -7, -7) and (room == 7.5).all()
        s, st = _raw(fresh, 64, many, room, max_workgroups=2)                            # 167 x 6 x 100: accepted (the edge itself: the host test)
        assert s == 0 and st[0] == 2 and st[3] == 100 and (room != 7.5).all()
        with pytest.raises(SmhipError):
            pose_graph.marginals(fresh, 63, [1])
        again, stats2 = optimise(fresh, "circle64", g)                                   # the next optimise call is unaffected
        assert again.tobytes() == poses.tobytes() and stats2 == stats
        s, _ = _raw(fresh, 64, q, cov, rows=rows, blocks=blocks)
        assert s == 0 and (cov != 7.5).all()
    finally:
        fresh.close()
