"""What tests/pose_graph_calib_ref.py alone must satisfy for the C++ and device tests against it to mean anything (DESIGN.md section 6,
"Odometry calibration factor"): the HANDEYE Jacobians and the Huber gradient against central differences, a graph without a HANDEYE
solved as pose_graph_robust_ref solves it bit for bit, every case of tests/pose_graph_calib_cases.py ending by a stop rule and
qualifying, and what the factor is for: a held calibration pulls a drifted ring back, a free one finds its rotation."""
import numpy as np
import pytest

import pose_graph_calib_cases as cases
import pose_graph_calib_ref as calib
import pose_graph_cases as base
import pose_graph_ref as ref
import pose_graph_robust_cases as robust_cases
import pose_graph_robust_ref as robust


def test_the_jacobians_against_central_differences():
    """A and B column by column on random poses with rotations of 0.5 rad and translations of about 5 m, h = 1e-6: the bound is the 1e-6
    of the existing restatements' tests"""
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(20):
        X, T, Z = ref.random_pose(rng, 0.5), ref.random_pose(rng, 0.5), ref.random_pose(rng, 0.5)
        e, A, B = calib.handeye_jacobians(X, T, Z)
        assert (e == calib.handeye_residual(X, T, Z)).all() and (A[:3, 3:] == 0.0).all() and (B[:3, 3:] == 0.0).all()
        for J, which in ((A, 0), (B, 1)):
            for c in range(6):
                d = np.zeros(6)
                d[c] = 1e-6
                up, dn = [X, T], [X, T]
                up[which], dn[which] = ref.retract(up[which], d), ref.retract(dn[which], -d)
                fd = (calib.handeye_residual(up[0], up[1], Z) - calib.handeye_residual(dn[0], dn[1], Z)) / 2e-6
                worst = max(worst, float(np.abs(fd - J[:, c]).max()))
    print("worst difference", worst)
    assert worst <= 1e-6


def test_b_vanishes_where_h_is_the_identity():
    T = ref.random_pose(np.random.default_rng(1), 0.5)
    _, A, B = calib.handeye_jacobians(np.eye(4), T, np.eye(4))
    assert np.abs(B).max() <= 1e-15 and np.linalg.matrix_rank(A) == 6


@pytest.mark.parametrize("name", ["ring16_free", "gps24_free"])
def test_the_gradient_is_that_of_half_the_cost(name):
    """J^T r against a central difference of cost / 2 along every free coordinate at the start of a _free case, where some HANDEYE
    factors are above their threshold and some below (asserted), none within 1e-3 of it.  h = 1e-6."""
    g = cases.graph(name)
    at = g["poses"]
    s, w, _ = calib.report(g, at)
    he = g["kinds"] == calib.HANDEYE
    print(name, "HANDEYE factors above the threshold", int((w[he] < 1.0).sum()), "of", int(he.sum()))
    assert (w[he] < 1.0).any() and (w[he] == 1.0).any() and (np.abs(s[he] - 1.0) > 1e-3).all()
    _, grad = calib.assemble(g, at)
    h = 1e-6
    fd = np.zeros_like(grad)
    for k in range(len(at)):
        if g["fixed"][k]:
            continue
        for a in range(6):
            d = np.zeros(6)
            d[a] = h
            up, dn = at.copy(), at.copy()
            up[k], dn[k] = ref.retract(at[k], d), ref.retract(at[k], -d)
            fd[6 * k + a] = 0.5 * (calib.cost(g, up) - calib.cost(g, dn)) / (2.0 * h)
    print(name, "largest |g|", np.abs(grad).max(), "largest difference", np.abs(fd - grad).max())
    assert np.abs(fd - grad).max() <= 1e-6 * np.abs(grad).max()


def test_without_a_handeye_it_is_the_robust_restatement_bit_for_bit():
    for name in ("robust16", "robust_point"):
        g = robust_cases.graph(name)
        want, sw = robust.optimize(g)
        got, sg = calib.optimize(g)
        assert got.tobytes() == want.tobytes() and all(sg[key] == sw[key] for key in sw)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(calib.linearize(g, g["poses"]), robust.linearize(g, g["poses"])))


@pytest.mark.parametrize("name", cases.names())
def test_the_cases_stop_by_a_rule_and_qualify(name):
    g, poses, st = cases.reference(name)
    same, diff, ratio = cases.qualifies(name)
    print(name, "stop", st["stop"], "steps", st["accepted"], st["rejected"], "direct against pcg", diff, "gradient ratio", ratio)
    assert st["stop"] in (ref.STOP_STEP, ref.STOP_COST)
    assert same and diff < 1e-10 and ratio < 1e-9
    j = g["calib_node"]
    assert (g["ij"][g["kinds"] == calib.HANDEYE, 1] == j).all() and bool(g["fixed"][j]) == name.endswith("_held")
    n = len(g["truth"])
    assert calib.non_chain_edges(g) == sum(1 for k, (a, b) in zip(g["kinds"], g["ij"]) if k != calib.PRIOR and abs(int(a) - int(b)) != 1)
    assert any(k == calib.HANDEYE and a == n - 1 and b == n for k, (a, b) in zip(g["kinds"], g["ij"]))      # the adjacent one: a chain block


def test_a_held_calibration_pulls_the_ring_back():
    """the 64-node ring, calibration held, Huber 1: the worst position error falls (the prototype behind the definition: 2.71 m to 0.07 m
    in 5 steps on its own drive)"""
    g, poses, st = cases.reference("ring64_held")
    before, after = cases.truth_error(g, g["poses"]), cases.truth_error(g, poses)
    print("worst position error", before, "->", after, "steps", st["accepted"], st["rejected"])
    assert after < before
    assert (poses[g["calib_node"]] == cases.T_TRUE).all()


@pytest.mark.parametrize("name", ["ring16_free", "ring64_free"])
def test_a_free_calibration_finds_its_rotation(name):
    """from a start 0.10 rad / 0.077 m off the rotation error of T ends below a fifth of its start.  The translation is not asserted: the
    0.1 m prior outweighs factors with sigmas of 1.5 - 2 m (printed)."""
    g, poses, st = cases.reference(name)
    r0, t0 = cases.calib_errors(g["poses"][g["calib_node"]])
    r1, t1 = cases.calib_errors(poses[g["calib_node"]])
    print(name, "rotation error", r0, "->", r1, "translation error", t0, "->", t1)
    assert abs(r0 - 0.10) < 1e-9 and abs(t0 - 0.077) < 1e-3
    assert r1 < r0 / 5.0
    assert cases.truth_error(g, poses) < cases.truth_error(g, g["poses"])
