"""tests/icp_information_ref.py checked against its own definition, without a GPU: every row J is the derivative of the
point-to-plane residual under T <- T * [Exp(phi), rho]; that tangent is the one tests/pose_graph_ref.py's BETWEEN residual uses; a
plane's information has rank 3 with the null space geometry says it has; a corridor's weakest direction is the translation along it."""
import numpy as np

import icp_information_ref as info
import pose_graph_ref as ref


def _perturbed(T, xi):
    return ref.retract(T, xi)                      # R Exp(phi), t + R rho: T * [Exp(phi), rho]


def test_every_row_is_the_derivative_of_its_residual():
    src, tgt, nrm, T = info.surface_pair(info.CORRIDOR, 257, 600, seed=3)
    s = src[:, :3].astype(np.float64)
    got = info.information(s, tgt, nrm, T, 0.7)
    k = got["rows"]
    assert got["kept"] == len(k) > 150
    q, n = tgt[got["ids"][k]], nrm[got["ids"][k]]
    step = 1e-6
    fd = np.zeros_like(got["J"])
    for a in range(6):
        xi = np.zeros(6)
        xi[a] = step
        Tp, Tm = _perturbed(T, xi), _perturbed(T, -xi)
        fd[:, a] = (info.rows(s[k], q, n, Tp[:3, :3], Tp[:3, 3])[1] - info.rows(s[k], q, n, Tm[:3, :3], Tm[:3, 3])[1]) / (2 * step)
    err = np.linalg.norm(fd - got["J"], axis=1) / np.linalg.norm(got["J"], axis=1)
    print("worst |J - fd| / |J|:", err.max())
    assert err.max() <= 1e-7
    assert np.allclose(got["H"], got["J"].T @ got["J"]) and np.isclose(got["sum_r2"], got["r"] @ got["r"])


def test_the_tangent_is_the_between_residuals():
    """Z = T measured, relative pose T * [Exp(xi)]: the BETWEEN residual of X_i = I, X_j = T * [Exp(xi)] is xi to second order"""
    T = info.surface_pair(info.PLANE, 8, 8, seed=1)[3]
    rng = np.random.default_rng(5)
    for scale in (1e-3, 1e-4):
        xi = rng.normal(size=6) * scale
        e = ref.residual(np.eye(4), _perturbed(T, xi), T)
        assert np.linalg.norm(e - xi) <= 2.0 * np.linalg.norm(xi) ** 2, (scale, e, xi)


def test_a_planes_information_has_rank_three():
    src, tgt, nrm, T = info.surface_pair(info.PLANE, 1999, 2000, seed=2)
    got = info.information(src[:, :3].astype(np.float64), tgt, nrm, T, 0.7)
    sv = np.linalg.svd(got["H"], compute_uv=False)
    print("singular values:", sv)
    assert sv[2] > 1e-3 * sv[0] and sv[3] < 1e-10 * sv[0]
    m = T[:3, :3].T @ np.array([0.0, 0.0, 1.0])                  # the plane's normal in the source frame
    a = np.cross(m, [1.0, 0.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(m, a)
    for null in (np.concatenate([m, np.zeros(3)]), np.concatenate([np.zeros(3), a]), np.concatenate([np.zeros(3), b])):
        assert np.linalg.norm(got["H"] @ null) <= 1e-10 * sv[0]


def test_a_corridors_weakest_direction_is_the_translation_along_it():
    src, tgt, nrm, T = info.surface_pair(info.CORRIDOR, 2000, 2000, seed=4)
    got = info.information(src[:, :3].astype(np.float64), tgt, nrm, T, 0.7)
    edge = info.edge_information(got["H"], got["sum_r2"], got["kept"])
    axis = np.concatenate([np.zeros(3), T[:3, :3].T @ np.array([1.0, 0.0, 0.0])])       # rho along the corridor, source frame
    print("strength:", edge["strength"], "weakest:", edge["weakest"])
    assert abs(edge["weakest"] @ axis) > 0.99
    assert edge["strength"][0] < 1e-6 and edge["strength"][1] > 10.0
    # L^T L: the floor across the corridor, the floor inflated a hundred times along it
    info_edge = edge["L"].T @ edge["L"]
    assert np.isclose(axis @ info_edge @ axis, 1.0 / (100.0 * 0.15) ** 2, rtol=1e-3)


def test_the_gpu_fixtures_have_no_near_ties():
    """the property the GPU test relies on (and asserts again on the device's values), on the CPU's own centring of the target"""
    import icp_information_cases as cases
    for name in cases.REGULAR:
        c = cases.cases()[name]
        mu = c["tgt"].mean(axis=0)
        centred = (c["tgt"] - mu).astype(np.float32).astype(np.float64)
        margin = cases.near_tie_margin(cases.moved_f32(c["src"], c["T"], mu), centred)[0]
        print(name, "runner-up margin:", margin)
        assert margin > 1e-4, name
