"""The constructed GICP inputs and their float64 reference (tests/gicp_ref.py) on their own: every condition the device tests
rely on is asserted here, on the CPU, for the clouds and seeds that are committed."""
import numpy as np
import pytest

from oracle import ndt_gicp as ong
from tests import gicp_ref as gr


@pytest.mark.parametrize("name", gr.LATTICE_CLOUDS)
def test_lattice_clouds_are_exact(name):
    pts = gr.cloud(name)
    assert gr.check_lattice(pts)
    n = gr.cloud_size(name) if name.startswith("n") else 2048 if name != "plane" else 1024
    assert len(pts) == n
    if name == "dups":
        u, c = np.unique(pts, axis=0, return_counts=True)
        assert (c == 2).all()
    else:
        assert len(np.unique(pts, axis=0)) == n
    # index order is unrelated to position: neighbouring indices are not neighbouring points
    if n >= 127:
        assert np.median(np.linalg.norm(np.diff(pts.astype(np.float64), axis=0), axis=1)) > 1.0


def test_check_lattice_refuses_inexact_clouds():
    pts = gr.cloud("ties").copy()
    with pytest.raises(AssertionError):
        gr.check_lattice(pts[:-1])                       # 2047 points, no longer symmetric: the mean is not a binary fraction
    pts[0, 0] += np.float32(2.0 ** -7)
    with pytest.raises(AssertionError):
        gr.check_lattice(pts)
    with pytest.raises(AssertionError):
        gr.check_lattice(gr.cloud("generic"))


@pytest.mark.parametrize("k", gr.cloud_ks("ties"))
def test_ties_cloud_ties_and_tie_sensitivity(k):
    pts = gr.cloud("ties")
    idx, d2 = gr.cloud_order("ties")
    idl, _ = gr.cloud_order("ties", largest=True)
    share = gr.tied(d2, k).mean()
    C, lam = gr.covariances(pts, idx[:, :k])
    Cl, _ = gr.covariances(pts, idl[:, :k])
    sensitive = int((np.abs(C - Cl).max(axis=(1, 2)) > 1e-3).sum())
    gap = gr.eigen_gap(lam).min()
    print(f"[ties k={k}] tied {share:.3f} sensitive {sensitive} smallest eigen gap {gap:.3f}")
    assert share >= 0.30
    assert sensitive >= 200
    assert gap > 1e-2


def test_every_compared_lattice_point_has_an_eigen_gap():
    for name, k in gr.COV_CASES:
        if gr.is_lattice(name):
            C, scale, checked = gr.cov_reference(name, k)
            assert checked.all()
            assert np.isfinite(scale).all() and (gr.U53 / scale).min() > 1e-2, (name, k)


def test_k3_is_degenerate_on_the_square_lattice():
    """Why k = 3 is not used with the lattice height fields: collinear triples, two zero eigenvalues."""
    idx, _ = gr.cloud_order("ties")
    _, lam = gr.covariances(gr.cloud("ties"), idx[:, :3])
    assert (lam[:, 1] == 0).sum() > 100


def test_reference_set_is_the_k_smallest_by_distance_then_index():
    pts = gr.cloud("dups")
    idx, d2 = gr.cloud_order("dups")
    p = pts.astype(np.float64)
    for i in (0, 17, 2047):
        d = ((p - p[i]) ** 2).sum(axis=1)
        want = sorted(range(len(p)), key=lambda j: (d[j], j))[:33]
        assert list(idx[i]) == want
    twin = np.array([np.flatnonzero((pts == pts[i]).all(axis=1)) for i in range(len(pts))])
    assert (idx[:, 0] == twin.min(axis=1)).all() and (idx[:, 1] == twin.max(axis=1)).all() and (d2[:, 1] == 0).all()


def test_reference_covariance_is_the_oracles_on_a_tie_free_cloud():
    pts = gr.cloud("generic")
    idx, d2 = gr.cloud_order("generic")
    assert not gr.tied(d2, 20).any()
    want, nn = ong.gicp_covariances(pts, return_nn=True)
    assert (np.sort(nn, axis=1) == np.sort(idx[:, :20], axis=1)).all()
    got, _, _ = gr.cov_reference("generic", 20)
    assert np.abs(got - want).max() < 1e-9


def test_plane_covariance_is_diag_1_1_eps():
    for k in gr.cloud_ks("plane"):
        C, scale, _ = gr.cov_reference("plane", k)
        want = np.diag([1.0, 1.0, gr.EPS])
        assert np.abs(C - want).max() <= gr.K_COV * scale.max()


def test_generic_cloud_excuses_at_most_two_percent():
    pts = gr.cloud("generic")
    _, d2 = gr.cloud_order("generic")
    far = np.linalg.norm(pts.astype(np.float64), axis=1) > 25
    assert far.sum() == 9
    for k in gr.KS:
        share = gr.generic_excused(pts, d2, k).mean()
        print(f"[generic k={k}] excused {share:.4f}")
        assert share <= gr.GENERIC_CAP


def test_measured_rho_cov():
    rho = gr.measure_rho_cov()
    print(f"[measured] RHO_COV {rho:.4g} (recorded {gr.RHO_COV}), K_COV {gr.k_from_rho(rho)} (recorded {gr.K_COV})")
    assert rho <= gr.RHO_COV
    assert gr.K_COV == gr.k_from_rho(gr.RHO_COV)


def _case(name):
    return gr.lazy_case(name.endswith("second")) if name.startswith("lazy") else gr.functor_case(name)


@pytest.mark.parametrize("name", gr.RHO_F_CASES + ("big",))
def test_functor_case_inputs(name):
    case = _case(name)
    assert gr.check_lattice(case.tgt) and gr.check_lattice(case.src)
    q = gr.transform_f32(case.src, case.guess)
    for mode in ("fma", "blas"):                          # the guess is exact on the lattice
        assert np.array_equal(q, gr.transform_f32(case.src, case.guess, mode))
    ref = gr.FunctorRef(case)
    assert ref.gap.min() >= gr.NEAREST_MARGIN             # one nearest target, by a margin
    at_gate = int((ref.d2 == 0.25).sum())
    inside = ref.d2[ref.keep]
    print(f"[{name}] ns {len(case.src)} kept {ref.m} exactly at the gate {at_gate} nearest-target margin {ref.gap.min():.4f}")
    assert not ref.keep[ref.d2 == 0.25].any()             # strict: d2 = thr2 is dropped
    pattern = name.split("/")[1] if "/" in name else "mix"
    if pattern in ("mix", "blocks", "four", "none"):
        assert at_gate > 0
    if pattern in ("mix", "blocks"):
        assert ref.m > 0 and inside.max() >= 0.25 - 2 * 0.5 * gr.Q      # some kept one lattice step inside the gate
    if pattern == "all":
        assert ref.m >= len(case.src) - 3
    if pattern == "four":
        assert ref.m == 4
    if pattern == "none":
        assert ref.m == 0
    if name.startswith("lazy"):
        _, cnt = np.unique(ref.j[ref.keep], return_counts=True)
        assert cnt.max() == 3 and len(case.src) % 64 != 0 and len(case.src) > 128 and ref.m == len(case.src)
    if name == "big":
        assert len(case.src) == 262145 and (case.tgt[:, 2] == 0).all() and (case.src[:, 1] == 0).all()
        assert -(-len(case.src) // 256) == 1025


def test_second_lazy_batch_needs_old_and_new_targets():
    a, b = gr.FunctorRef(gr.lazy_case(False)), gr.FunctorRef(gr.lazy_case(True))
    first, second = set(a.j[a.keep].tolist()), set(b.j[b.keep].tolist())
    assert len(second & first) > 20 and len(second - first) > 20


def test_functor_reference_is_the_oracles_functor():
    case = gr.functor_case("ns257/mix/r")
    ref = gr.FunctorRef(case)
    fn = ong.GicpFunctor(case.guess, ref.src, ref.tgt, ref.maha, transform_mode="nofma")
    for x in gr.XS:
        vals, S = ref.reference(x)
        f, g = fn.fdf(x)
        assert gr.functor_ratio(np.concatenate([[f], g]), vals, S)[0] <= gr.K_F
        assert (S > 0).all()


def test_transposed_rotation_and_open_gate_move_the_reference():
    """What the device tests must be able to see: R^T for R in the Mahalanobis product, and <= for < at the gate."""
    case = gr.functor_case("ns257/mix/r")
    ref = gr.FunctorRef(case)
    vals, S = ref.reference(gr.XS[0])
    wrong = gr.FunctorRef(case)
    R = case.guess[:3, :3].astype(np.float64).T
    Cs, Ct = gr.case_covariances(case)
    wrong.maha = np.linalg.inv(R[None] @ Cs[ref.keep] @ R.T[None] + Ct[ref.j[ref.keep]])
    assert gr.functor_ratio(wrong.evaluate(gr.XS[0])[0], vals, S)[0] > 1e6
    assert int((ref.d2 <= 0.25).sum()) > ref.m


def test_measured_rho_f():
    rho = gr.measure_rho_f(gr.RHO_F_CASES)
    print(f"[measured] RHO_F {rho:.4g} (recorded {gr.RHO_F}), K_F {gr.k_from_rho(rho)} (recorded {gr.K_F})")
    assert rho <= gr.RHO_F
    assert gr.K_F == gr.k_from_rho(gr.RHO_F)
