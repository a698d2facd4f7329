"""The CPU reference of the device CalculateNormals (tests/normals_ref.py) against the two oracle restatements of
builder/data/cloud_types.cc:73-144, 347-368 and against the product's host smhip_calculate_normals_f64; its own pieces on
hand-built leaves; and three deliberately WRONG statements of the split rule, which the same comparisons must reject.  No GPU."""
import ctypes
import functools

import numpy as np
import pytest

import normals_ref as nr
from oracle import cref
from oracle import icp_fast as onp
from staticmapping_amd import synth

F = np.float32


def tie_free(p32):
    """the cloud with every repeated coordinate value of a column moved up by float32 steps until the column has no ties
    (std::nth_element's choice among equal cut coordinates is open, so only tie-free clouds pin the oracles' partition)"""
    p = np.array(p32, dtype=F)
    for c in range(3):
        col = p[:, c]
        while True:
            o = np.argsort(col, kind="stable")
            dup = np.zeros(len(col), dtype=bool)
            dup[o[1:]] = col[o[1:]] == col[o[:-1]]
            if not dup.any():
                break
            col[dup] = np.nextafter(col[dup], F(np.inf))
    return p


@functools.lru_cache(maxsize=None)
def cloud(name):
    if name == "planes5000":
        a = synth.three_planes_pair(5000, seed=1)[0]
    else:
        a = synth.scan_pair("cfg2", n_points=int(name[4:]))[0]
    return np.ascontiguousarray(a[:, :3].astype(F))


@functools.lru_cache(maxsize=None)
def quantised(n):
    p = cloud(f"cfg2{n}")
    return np.ascontiguousarray((np.round(p / F(0.02)) * F(0.02)).astype(F))


def _sets(perm, ranges):
    return sorted(tuple(sorted(int(i) for i in perm[f:l])) for f, l in ranges)


def compare_with_oracle(p32, oracle, **rule):
    """same leaf index sets as the oracle's partition; the oracle's kept means are, in order, the means of reference leaves
    (1e-12), and no reference leaf the oracle has dropped is one the reference keeps by rank"""
    p64 = p32.astype(np.float64)
    perm, ranges = oracle.normals_partition(p64)
    L = nr.leaves(p32, **rule)
    assert _sets(perm, [tuple(r) for r in ranges]) == sorted(tuple(int(i) for i in ids) for ids in L)
    q, nrm, sz = oracle.calculate_normals(p64)
    mean = np.array([sum(p64[i] for i in ids) / len(ids) for ids in L])
    j = 0
    skipped = []
    for k in range(len(L)):
        if j < len(q) and len(L[k]) == sz[j] and np.abs(mean[k] - q[j]).max() < 1e-12:
            j += 1
        else:
            skipped.append(k)
    assert j == len(q), (j, len(q))
    if skipped:                                   # (the oracle keeps NaN normals: only the rank test drops a leaf there)
        dec = nr.rank_decision(p32, [L[k] for k in skipped])
        assert (dec != nr.KEEP).all(), (skipped[:5], dec[:5])


def partition_checks(which, **rule):
    """every comparison that pins the split rule; `which` selects one so that the time is spread over test cases"""
    if which == "numpy-oracle-5000":
        compare_with_oracle(tie_free(cloud("cfg25000")), onp, **rule)
    elif which == "c-oracle-20000":
        compare_with_oracle(tie_free(cloud("cfg220000")), cref, **rule)
    elif which == "c-oracle-120000":
        compare_with_oracle(tie_free(cloud("cfg2120000")), cref, **rule)
    elif which == "planes-5000":
        compare_with_oracle(tie_free(cloud("planes5000")), cref, **rule)
    elif which == "rule-on-ties-20000":
        p = quantised(20000)
        perm, ranges, _ = nr.tree(p, **rule)
        nr.check_legal_partition(p, perm, ranges, tie_rule=True)
    else:
        raise KeyError(which)


CHECKS = ["numpy-oracle-5000", "c-oracle-20000", "c-oracle-120000", "planes-5000", "rule-on-ties-20000"]


@pytest.mark.parametrize("which", CHECKS)
def test_partition_matches_the_oracles_and_the_stated_rule(which):
    partition_checks(which)


WRONG = {"left = count / 2": dict(left_of=lambda c: c // 2),
         "ties to the largest index": dict(tie_sign=-1),
         "cut value from rank left - 1": dict(cut_rank=-1)}


@pytest.mark.parametrize("name", list(WRONG))
def test_a_wrong_statement_of_the_rule_is_caught(name):
    """The comparison can fail.  `left = count / 2` and the cut value from rank left - 1 differ from the oracle on a tie-free
    cloud.  Ties to the largest index cannot differ from an oracle there (no ties), and on tied input the oracles' outcome is only
    ONE legal one: that variant is caught by the statement of the rule itself on the 2 cm-quantised scan."""
    caught = []
    for which in ("c-oracle-20000", "rule-on-ties-20000"):
        try:
            partition_checks(which, **WRONG[name])
        except AssertionError:
            caught.append(which)
    print(name, "caught by", caught)
    assert caught
    if name != "ties to the largest index":
        assert "c-oracle-20000" in caught


def test_oracle_outcomes_on_tied_input_are_legal():
    """cfg2 quantised to 2 cm (thousands of ties per cut): what the oracles' nth_element did is one legal outcome"""
    p = quantised(20000)
    assert len(p) - len(np.unique(p[:, 0])) > 10_000
    perm, ranges = cref.normals_partition(p.astype(np.float64))
    nr.check_legal_partition(p, perm, [tuple(r) for r in ranges])
    p5 = quantised(5000)
    perm5, ranges5 = onp.normals_partition(p5.astype(np.float64))
    nr.check_legal_partition(p5, perm5, [tuple(r) for r in ranges5])
    # and the checker can fail: two points swapped across the root's cut
    x = p[perm, 0]
    half = len(p) - len(p) // 2
    a, b = int(np.argmin(x[:half])), half + int(np.argmax(x[half:]))
    perm[a], perm[b] = perm[b], perm[a]
    with pytest.raises(AssertionError):
        nr.check_legal_partition(p, perm, [tuple(r) for r in ranges])


@pytest.mark.parametrize("name", ["cfg25000", "cfg220000"])
def test_host_calculate_normals_against_the_reference(name):
    """smhip_calculate_normals_f64 (the product's host path): its finite-normal rows are reference leaves -- every one the
    reference keeps, none it drops -- with means to 1e-12 and normals within FACTOR * sigma (+ 2^-51: the normalisation's own
    square root and division, which the draws do not perturb) on the informative leaves."""
    from scipy.spatial import cKDTree
    import staticmapping_amd as sm
    p32 = tie_free(cloud(name))
    p = np.ascontiguousarray(p32.astype(np.float64))
    lib = sm._capi.load_library()
    op = np.zeros_like(p); on = np.zeros_like(p); m = ctypes.c_int32()
    assert lib.smhip_calculate_normals_f64(p.ctypes.data_as(sm._capi.c_double_p), len(p), op.ctypes.data_as(sm._capi.c_double_p),
                                           on.ctypes.data_as(sm._capi.c_double_p), ctypes.byref(m)) == 0
    q, n = op[:m.value], on[:m.value]
    fin = np.isfinite(n).all(axis=1)
    q, n = q[fin], n[fin]
    R = nr.LeafReference(p32)
    mean = np.array([sum(p[i] for i in ids) / len(ids) for ids in R.leaves])
    d, j = cKDTree(mean).query(q)
    assert d.max() < 1e-12 and len(np.unique(j)) == len(j)
    got = np.zeros(len(R.leaves), dtype=bool); got[j] = True
    assert not (got & (R.decision == nr.DROP)).any() and not (~got & (R.decision == nr.KEEP)).any()
    assert (R.decision == nr.UNDECIDABLE).mean() <= 1e-3
    info = R.informative[j]
    err = np.abs(n - R.exact[j]).max(axis=1)
    ratio = err[info] / (R.tol64[j][info] + 2.0 ** -51)
    print(name, "host: informative", int(info.sum()), "of", len(j), "worst |n - n_exact| / tol", ratio.max())
    assert ratio.max() <= 1.0
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-12


def test_keeps_on_hand_built_leaves():
    line = np.array([[0.25 * i, 2, 3] for i in range(7)], F)                   # 7 points on a line: rank 1
    assert nr.keeps(line, np.arange(7)) == nr.DROP
    tri = np.array([[1, 0, 1], [0, 1, 1], [0, 0, 1]], F)                       # 3 points, not collinear, plane z = 1 misses the origin
    assert nr.keeps(tri, np.arange(3)) == nr.KEEP
    flat = np.array([[1, 0, 0], [0, 1, 0], [1, 1, 0], [2, 1, 0]], F)           # in the plane z = 0: det(M) == 0, no finite normal
    assert nr.keeps(flat, np.arange(4)) == nr.DROP
    assert nr.leaf_normal_exact(flat, np.arange(4)) is None
    assert nr.keeps(np.array([[1, 2, 3]], F), [0]) == nr.DROP                  # one point: rank 0
    assert nr.keeps(np.array([[1, 2, 3], [1, 2, 5]], F), [0, 1]) == nr.DROP    # two points: rank 1
    n = nr.leaf_normal_exact(tri, np.arange(3))
    assert np.array_equal(n, [0.0, 0.0, 1.0])                                  # M^-1 b of points with n.p = 1 is n
    assert np.array_equal(nr.leaf_mean(tri, [2, 0, 1]), (np.array([1, 1, 3], np.float64) / 3).astype(F))


def test_leaf_mean_is_the_double_sum_in_index_order():
    p = cloud("cfg25000")
    L = nr.leaves(p)
    all_means = nr.leaf_means(p, L)
    for k in range(0, len(L), 37):
        assert np.array_equal(all_means[k], nr.leaf_mean(p, L[k]))
    assert sorted(int(i) for ids in L for i in ids) == list(range(len(p)))     # a partition
    assert [int(ids[0]) for ids in L] == sorted(int(ids[0]) for ids in L)       # in emit order
    assert max(len(ids) for ids in L) <= 7 and min(len(ids) for ids in L) >= 4


@pytest.mark.parametrize("name,n_leaves,cap", [("planes5000", 1024, 0.0), ("cfg220000", 4096, 0.03), ("cfg2120000", 21696, 0.10)])
def test_the_tolerance_table_is_reproduced_within_its_caps(name, n_leaves, cap):
    R = nr.LeafReference(cloud(name))
    share = 1.0 - R.informative.mean()
    tol = np.nan_to_num(R.tol, nan=np.inf)
    print(name, "leaves", len(R.leaves), "uninformative", share, "median tol", np.median(tol), "95 % tol", np.quantile(tol, 0.95),
          "undecidable", (R.decision == nr.UNDECIDABLE).mean())
    assert len(R.leaves) == n_leaves
    assert share <= cap
    assert np.median(tol) < 1.2e-7
    assert (R.decision == nr.UNDECIDABLE).mean() <= 1e-3
    # a held-out 17th draw stays inside the tolerance on every informative leaf
    rng = np.random.default_rng(nr.SEED)
    for _ in range(nr.DRAWS + 1):
        d = nr.leaf_normal_f64(R.p32, R.leaves, rng)
    err = np.abs(d - R.exact).max(axis=1)
    assert (err[R.informative] <= R.tol64[R.informative]).all()
