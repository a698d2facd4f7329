"""The GICP kernels (csrc/gicp_kernels.hip: gicp_knn_cov, gicp_need / gicp_knn_cov_listed, gicp_corr, gicp_fdf) against the
float64 reference of tests/gicp_ref.py on constructed clouds: neighbour sets under ties, the strict distance gate, the
Mahalanobis product with R != R^T, the functor's fold at the source sizes where it changes shape, covariances on demand.
Every test prints its worst |device - reference| / scale; the bounds K_COV and K_F are measured on the CPU (gicp_ref.py)."""
import numpy as np
import pytest

import staticmapping_amd as sm
from tests import gicp_ref as gr

pytestmark = pytest.mark.gpu

COV_GUESS = np.eye(4)
COV_GUESS[0, 3] = gr.Q                      # the run behind the hooks: one outer iteration from a lattice step away


@pytest.fixture(scope="module")
def matcher():
    m = sm.NdtGicpHip(max_source_points=8192, max_target_points=8192)
    yield m
    m.close()


def _covariances(m, name, k, cell=0.0):
    """The cloud as source (which = 0: the scratch slot's grid) and as target (which = 1: the job slot's) of one run."""
    pts = gr.cloud(name)
    m.set_gicp_options(gicp_k_correspondences=k, gicp_max_iterations=1, gicp_search_cell=cell, gicp_corr_dist_threshold=5.0)
    m.gicp_only(pts, pts, COV_GUESS)
    return m.get_covariances(0, len(pts)), m.get_covariances(1, len(pts))


def _check_covariances(m, name, k, cell=0.0):
    src, tgt = _covariances(m, name, k, cell)
    out = []
    for which, got in (("source", src), ("target", tgt)):
        assert np.isfinite(got).all()
        r, i = gr.cov_ratio(got, name, k)
        out.append((which, r, i))
    print(f"[cov {name} k={k} cell={cell or 'default'}] worst ratio source {out[0][1]:.3g} target {out[1][1]:.3g} (allowed {gr.K_COV:g})")
    for which, r, i in out:
        assert r <= gr.K_COV, (name, k, cell, which, r, i)


@pytest.mark.parametrize("name,k", gr.COV_CASES, ids=[f"{n}-k{k}" for n, k in gr.COV_CASES])
def test_neighbour_sets_and_covariances(matcher, name, k):
    """Both clouds of a run, every constructed cloud: the set is the k smallest by (float distance, caller index)."""
    _check_covariances(matcher, name, k)


@pytest.mark.parametrize("k", gr.cloud_ks("ties"))
@pytest.mark.parametrize("cell", [0.1, 0.5, 8.0])
def test_ties_cloud_across_search_cells(matcher, cell, k):
    """0.1: a cell below the point spacing, mostly empty shells.  0.5: cell faces on lattice planes, so that neighbours sit
    exactly on the face of an unexplored cell, straight along an axis, when a shell ends.  8.0: the whole cloud in a few cells."""
    _check_covariances(matcher, "ties", k, cell)
    g = matcher.debug_get_grid(0)                        # the job slot's grid, as get_covariances(1) built it
    assert abs(float(g["h"]) - cell) < 1e-6
    if cell == 0.5:
        rel = (g["tq"][:, :3].astype(np.float64) - g["origin"].astype(np.float64)) / float(g["h"])
        on_face = rel == np.round(rel)
        print(f"[grid cell=0.5] origin {g['origin']} points on a cell face: x {on_face[:, 0].mean():.2f} y {on_face[:, 1].mean():.2f} z {on_face[:, 2].mean():.2f}")
        assert on_face[:, 0].mean() > 0.4 and on_face[:, 1].mean() > 0.4 and on_face[:, 2].mean() > 0.1
    if cell == 8.0:
        assert g["nocc"] <= 27 and g["nt"] / g["nocc"] > 4 * k


def test_plane_is_diag_1_1_eps(matcher):
    src, tgt = _covariances(matcher, "plane", 20)
    want = np.diag([1.0, 1.0, gr.EPS])
    _, scale, _ = gr.cov_reference("plane", 20)
    worst = max(np.abs(src - want).max(), np.abs(tgt - want).max())
    print(f"[plane] largest |C - diag(1, 1, eps)| {worst:.3g}")
    assert worst <= gr.K_COV * scale.max()


# ---- correspondences, Mahalanobis matrices, functor ------------------------------------------------------------------------
def _check_functor(m, case, label, evaluate_only=False):
    ref = gr.FunctorRef(case)
    guess = case.guess.astype(np.float64)
    if not evaluate_only:
        m.set_gicp_options(gicp_k_correspondences=case.k, gicp_max_iterations=1, gicp_search_cell=0.0, gicp_corr_dist_threshold=case.threshold)
        m.gicp_only(case.src, case.tgt, guess)
        assert m.last_gicp_stats["gicp_correspondences"] == ref.m, (label, m.last_gicp_stats, ref.m)
    if ref.m == 0:
        return None
    worst = (-1.0, None)
    for n, x in enumerate(gr.XS):
        f, g = m.gicp_evaluate(guess, x)
        assert np.isfinite(f) and np.isfinite(g).all()
        vals, S = ref.reference(x)
        r, c = gr.functor_ratio(np.concatenate([[f], g]), vals, S)
        if r > worst[0]:
            worst = (r, (n, c))
    print(f"[functor {label}] ns {len(case.src)} kept {ref.m} worst ratio {worst[0]:.3g} at (x, component) {worst[1]} (allowed {gr.K_F:g})")
    assert worst[0] <= gr.K_F, (label, worst)
    return ref


@pytest.mark.parametrize("name", [c[0] for c in gr.FUNCTOR_CASES if c[3] != "none"])
def test_gate_mahalanobis_and_functor(matcher, name):
    """gicp_corr's strict gate (points at d2 = thr2 exactly are dropped: the kept count is the reference's), R C1 R^T + C2 with
    a rotation that is not symmetric, sym_inverse, and gicp_fdf's sums and fold at 1, 2 and 17 workgroups."""
    case = gr.functor_case(name)
    ref = _check_functor(matcher, case, name)
    if "/blocks/" in name:
        # whole workgroups of gicp_fdf with nothing kept (their partial sums are all zero), in the order the device holds the source
        _, caller = matcher.get_source(0)
        kept = ref.keep[caller]
        per_group = [int(kept[a:a + 256].sum()) for a in range(0, len(kept), 256)]
        print(f"[functor {name}] kept per workgroup {per_group}")
        assert len(per_group) == 17 and min(per_group[:-1]) == 0 and max(per_group) > 0


def test_evaluate_without_a_kept_correspondence_is_an_error(matcher):
    """Every source point at or beyond the gate: the run ends at once, and the functor -- sums divided by the kept count -- has no
    value: a status and a message, not SMHIP_OK with NaN."""
    case = gr.functor_case("ns4097/none/r")
    assert _check_functor(matcher, case, case.name) is None
    with pytest.raises(sm.SmhipError) as e:
        matcher.gicp_evaluate(case.guess.astype(np.float64), np.zeros(6))
    assert "no correspondence" in str(e.value)


def test_functor_fold_with_capped_workgroups():
    """ns = 262 145: ceil(ns / 256) = 1025 > 1024, so nblk is capped and the grid-stride loop takes a second trip.  Both clouds
    are flat, so every covariance is diag(1, 1, eps) in its plane whatever the neighbour set."""
    case = gr.functor_case("big")
    m = sm.NdtGicpHip(max_source_points=1 << 19, max_target_points=1 << 19)
    try:
        _check_functor(m, case, "big")
    finally:
        m.close()


# ---- covariances on demand -------------------------------------------------------------------------------------------------
def test_covariances_on_demand():
    """A batch of four estimates a target's covariances where source points are matched (gicp_need: the atomicExch that lets one
    of three askers list a point, the ballot compaction across waves; gicp_knn_cov_listed on tied target points).  A second
    batch on the kept targets under a shifted guess needs some covariances that carry the epoch and some that are new."""
    first, second = gr.lazy_case(False), gr.lazy_case(True)
    others = [gr.small_pair(61 + j) for j in range(3)]
    m = sm.NdtGicpHip(max_source_points=4096, max_target_points=4096, jobs=4)
    try:
        m.set_gicp_options(use_ndt=0, using_voxel_filter=0, gicp_max_iterations=1, gicp_k_correspondences=20, gicp_corr_dist_threshold=0.5)
        m.set_input_source(first.src, slot=0); m.set_input_target(first.tgt, slot=0)
        for j, (s, t, g) in enumerate(others):
            m.set_input_source(s, slot=j + 1); m.set_input_target(t, slot=j + 1)
        had = set()                                          # job 0's target points whose covariance carries the epoch
        for case in (first, second):
            guesses = [case.guess.astype(np.float64)] + [g.astype(np.float64) for _, _, g in others]
            _, _, st = m.align_batch(4, guesses)
            ref = gr.FunctorRef(case)
            assert st[0]["gicp_correspondences"] == ref.m and st[0]["n_source"] == len(case.src) and st[0]["n_target"] == len(case.tgt)
            # every matched target point is listed once, whoever asks (three source points share one), and only if it is new
            matched = set(ref.j[ref.keep].tolist())
            print(f"[{case.name}] matched target points {len(matched)} of {ref.m} correspondences, new {len(matched - had)}, "
                  f"estimated on demand {st[0]['gicp_covariances_on_demand']}")
            assert st[0]["gicp_covariances_on_demand"] == len(matched - had)
            for j in range(3):
                assert st[j + 1]["gicp_correspondences"] == 256
                assert st[j + 1]["gicp_covariances_on_demand"] == (0 if had else 256)
            had |= matched
            _check_functor(m, case, case.name, evaluate_only=True)
    finally:
        m.close()
