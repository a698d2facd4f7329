"""The marginal covariances' restatement (tests/pose_graph_marginals_ref.py) against what is known without it: the two analytic cases,
numpy's dense inverse of the same H on every graph of tests/pose_graph_marginals_cases.py, and the conditions the device tests
lean on -- every column converges below the cap, an active Huber weight reaches H."""
import numpy as np
import pytest

import pose_graph_marginals_cases as cases
import pose_graph_marginals_ref as mref
import pose_graph_robust_ref as robust


def _relative(have, want):
    return float(np.abs(have - want).max() / np.abs(want).max())


@pytest.mark.parametrize("which", ["two_nodes", "prior_alone"])
def test_the_analytic_cases_give_the_sigmas_squared(which):
    """Node 0 held and one BETWEEN measured exactly, or one node held by a PRIOR around its own pose: the residual is zero, the free
    node's Jacobian is I / sigma, H = diag(1 / sigma^2) and Sigma = diag(sigma^2), to 1e-12 relative by both solvers."""
    g = cases.two_nodes() if which == "two_nodes" else cases.prior_alone()
    k = len(g["poses"]) - 1
    H, fixed, cap = mref.system(g, g["poses"])
    want = np.diag(cases.ANALYTIC_SIGMAS ** 2)
    out = mref.pcg_columns(H, fixed, [k], cap)
    cov, _ = mref.covariances(out["x"], fixed, [k])
    dcov, _ = mref.covariances(mref.dense_columns(mref.dense(H, fixed), [k]), fixed, [k])
    print(which, "pcg", np.abs(cov[0] - want).max(), "dense", np.abs(dcov[0] - want).max(), "iterations", out["iterations"])
    for have in (cov[0], dcov[0]):
        assert (np.abs(have - want) <= 1e-12 * np.abs(want).max()).all()
        assert (np.abs(np.diag(have) - np.diag(want)) <= 1e-12 * np.diag(want)).all()
    assert out["converged"].all() and out["iterations"].max() < cap


@pytest.fixture(scope="module")
def solved():
    """name -> (H, fixed, cap, pcg_columns of every node, dense columns of every node): computed once"""
    return {name: cases.restated(name) for name in cases.ALL}


@pytest.mark.parametrize("name", cases.ALL)
def test_pcg_columns_against_the_dense_inverse(solved, name):
    """Every column of every node within 100 eps cond(H) + 10 x the measured truncation of numpy.linalg.inv(H), relative to the largest
    entry; every column converged, in fewer iterations than the cap (the condition the device's counts are compared under); a fixed
    node's columns are zero."""
    H, fixed, cap, out, D = solved[name]
    rel = _relative(out["x"], D)
    its = out["iterations"][~fixed]
    print(name, "nodes", len(fixed), "cond %.3g" % np.linalg.cond(H), "iterations", its.min(), "..", its.max(), "of", cap, "relative difference %.3g" % rel,
          "bound %.3g" % mref.bound(H))
    assert rel <= mref.bound(H)
    assert out["converged"].all() and its.max() < cap and its.min() >= 1
    assert (out["x"][fixed] == 0.0).all() and (out["iterations"][fixed] == 0).all()
    assert (out["x"][:, np.repeat(fixed, 6), :] == 0.0).all()


def test_the_truncation_that_the_bound_carries(solved):
    """TRUNCATION_MEASURED is the worst difference to the dense inverse over the graphs with cond(H) < 1e7 (where 100 eps cond is below
    2.3e-7 and the dense inverse's own floor, eps cond, below 2.3e-9 -- in fact far lower), rounded up: not below what is measured here and
    not more than twice it."""
    worst = 0.0
    for name in cases.ALL:
        H, fixed, cap, out, D = solved[name]
        if np.linalg.cond(H) < 1e7:
            rel = _relative(out["x"], D)
            print(name, "relative difference %.3g" % rel)
            worst = max(worst, rel)
    print("worst %.3g" % worst, "recorded %.3g" % mref.TRUNCATION_MEASURED)
    assert worst <= mref.TRUNCATION_MEASURED <= 2.0 * worst


def test_the_optimisers_own_tolerance_is_looser(solved):
    """at 1e-8 the same columns end a hundred times further from the dense inverse: the tolerance is what sets the truncation"""
    H, fixed, cap, out, D = solved["circle64"]
    q = list(range(len(fixed)))
    loose = mref.pcg_columns(H, fixed, q, cap, tol=1e-8)
    print("1e-10: %.3g" % _relative(out["x"], D), "1e-8: %.3g" % _relative(loose["x"], D), "iterations", loose["iterations"][~fixed].max(), out["iterations"][~fixed].max())
    assert _relative(loose["x"], D) > 10.0 * _relative(out["x"], D)
    assert loose["iterations"].max() < out["iterations"].max()


def test_what_the_kernels_operators_do_to_the_iteration_counts(solved):
    """The definition names the optimiser's own operators: H p factor by factor and M^-1 by the cyclic reduction.  A solve of the same
    columns through the assembled H and LAPACK's LU of M ends at the same answer -- inside the bound of the dense inverse -- but on n64
    (cond 5.9e9, two loop edges between free nodes: 25 iterations in exact arithmetic) its longest column takes 32 where the
    definition's takes 26, because A^T A formed once squares what rounding sees and delays convergence.  Measured: 26 and 9 436 in all
    against 32 and 10 797."""
    H, fixed, cap, out, D = solved["n64"]
    q = list(range(len(fixed)))
    other = mref.pcg_columns(H, fixed, q, cap, operators="dense")
    print("kernel operators: longest", out["iterations"].max(), "total", out["iterations"].sum(), "dense operators: longest", other["iterations"].max(), "total",
          other["iterations"].sum(), "difference of the answers %.3g" % _relative(other["x"], out["x"]))
    assert _relative(other["x"], D) <= mref.bound(H) and other["converged"].all()
    assert other["iterations"].max() >= out["iterations"].max() + 3 and other["iterations"].sum() > out["iterations"].sum()
    assert out["iterations"].max() <= 12 * 2 + 1 + 1


def test_an_active_huber_weight_reaches_h():
    """robust16's wrong loop edge ends with a weight below 1; with the thresholds taken away, at the same poses, the covariances differ by
    far more than the bound"""
    g, poses = cases.optimised("robust16")
    _, _, _, w = robust.linearize(g, poses)
    assert (w < 1.0).any()
    H, fixed, cap = mref.system(g, poses)
    H1, _, _ = mref.system(cases.without_thresholds(g), poses)
    q = list(range(len(poses)))
    a, _ = mref.covariances(mref.pcg_columns(H, fixed, q, cap)["x"], fixed, q)
    b, _ = mref.covariances(mref.pcg_columns(H1, fixed, q, cap)["x"], fixed, q)
    print("weights below 1:", int((w < 1.0).sum()), "smallest", w.min(), "relative change of the covariances", _relative(a, b), "bound", mref.bound(H))
    assert _relative(a, b) > 1e3 * max(mref.bound(H), mref.bound(H1))


def test_cross_blocks_are_each_others_transposes_and_fixed_rows_are_zero():
    g, poses = cases.optimised("fixed_in_the_middle")
    H, fixed, cap = mref.system(g, poses)
    rows = [0, 3, 9, 20]
    out = mref.pcg_columns(H, fixed, rows, cap)
    cov, blocks = mref.covariances(out["x"], fixed, rows, rows)
    assert fixed[0] and fixed[9]
    assert (cov[0] == 0.0).all() and (cov[2] == 0.0).all() and (blocks[:, 0] == 0.0).all() and (blocks[:, 2] == 0.0).all() and (blocks[0] == 0.0).all()
    assert np.abs(blocks[1, 3] - blocks[3, 1].T).max() <= mref.bound(H) * np.abs(out["x"]).max()
    assert (np.linalg.eigvalsh(cov[1]) > 0.0).all() and (np.linalg.eigvalsh(cov[3]) > 0.0).all()
    assert (cov[1] == cov[1].T).all()
    W = mref.world_position_covariance(poses[3], cov[1])
    assert np.allclose(np.linalg.eigvalsh(W), np.linalg.eigvalsh(cov[1][3:, 3:]), rtol=1e-12)
