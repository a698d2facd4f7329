"""tests/pose_graph_info_ref.py checked against its own definition, without a GPU: the whitened Jacobians are the derivatives of the
whitened residual, a graph without an L is pose_graph_calib_ref's, L = diag(1 / sigma) is the sigma form, and the case that shows
the point -- edges that do not see x let the POINT factors decide it."""
import numpy as np

import pose_graph_calib_cases as calib_cases
import pose_graph_calib_ref as calib
import pose_graph_cases as base
import pose_graph_info_cases as cases
import pose_graph_info_ref as pgi
import pose_graph_ref as ref


def test_the_whitened_jacobians_are_the_residuals_derivatives():
    g = cases.graph("ring16_full")
    r, A, B, w = pgi.linearize(g, g["poses"])
    step = 1e-6
    worst = 0.0
    for k in np.flatnonzero([L is not None for L in g["L"]])[:6]:
        assert w[k] == 1.0
        i, j = g["ij"][k]
        L = g["L"][k]
        for which, J in ((i, A[k]), (j, B[k])):
            fd = np.zeros((6, 6))
            for a in range(6):
                xi = np.zeros(6)
                xi[a] = step
                plus, minus = g["poses"].copy(), g["poses"].copy()
                plus[which], minus[which] = ref.retract(plus[which], xi), ref.retract(minus[which], -xi)
                fd[:, a] = (L @ calib.factor_residual(calib.BETWEEN, plus[i], plus[j], g["data"][k])
                            - L @ calib.factor_residual(calib.BETWEEN, minus[i], minus[j], g["data"][k])) / (2 * step)
            worst = max(worst, np.abs(fd - J).max() / np.abs(J).max())
    print("worst |J - fd| / |J|:", worst)
    assert worst <= 1e-7


def test_a_graph_without_an_information_is_the_calib_restatements():
    g = calib_cases.graph("ring16_free")
    gi = pgi.with_information(g, [None] * len(g["kinds"]))
    assert pgi.cost(gi, g["poses"]) == calib.cost(g, g["poses"])
    want, st = calib.optimize(g)
    got, si = pgi.optimize(gi)
    assert got.tobytes() == want.tobytes() and (si["stop"], si["accepted"], si["rejected"]) == (st["stop"], st["accepted"], st["rejected"])


def test_a_diagonal_information_is_the_sigma_form():
    _, got, _ = cases.reference("ring16_diag")
    _, want, _ = calib_cases.reference("ring16_free")
    dt, dr = base.pose_difference(got, want)
    print("L = diag(1 / sigma) against the sigma form:", dt, dr)
    assert dt <= 1e-12 and dr <= 1e-12


def test_edges_that_do_not_see_x_let_the_points_decide_it():
    _, plain, _ = cases.reference("chain6_sigma")
    _, weak, _ = cases.reference("chain6_weak_x")
    print("distance from the POINT targets along x: sigma edges", cases.x_miss(plain), "weak-x edges", cases.x_miss(weak))
    assert cases.x_miss(weak).max() < 0.05 and cases.x_miss(plain).max() > 0.05
    L = cases.weak_x_information()
    info_edge = L.T @ L
    assert np.isclose(info_edge[3, 3], 1.0 / 15.0 ** 2, rtol=1e-9) and np.isclose(info_edge[4, 4], 1.0 / 0.15 ** 2, rtol=1e-3)


def test_the_restatements_own_two_solves_agree():
    for name in cases.NAMES:
        _, a, sa = cases.reference(name)
        _, b, sb = cases.reference(name, "pcg")
        assert (sa["accepted"], sa["rejected"], sa["stop"]) == (sb["accepted"], sb["rejected"], sb["stop"]), name
        assert max(base.pose_difference(a, b)) < 1e-10, name
