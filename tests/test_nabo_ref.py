"""tests/nabo_ref.py and tests/nabo_cases.py on their own: every condition tests/test_nabo_exact_gpu.py relies on is asserted
here, on the CPU -- the reference equals both restatements of libnabo where the library defines the answer, the rule check tells
right trees from wrong ones, the lattice fixtures are exact, the off-lattice ones are decidable but for a share under their cap,
and the queries are sharp enough that six wrong walks each change an answer."""
import inspect
import math

import numpy as np
import pytest

from oracle import cref, nabo
from tests import nabo_cases as nc
from tests import nabo_ref as nr

UNDECIDABLE_CAP = 1.0e-3          # per off-lattice fixture


def _mutant(func, *swaps):
    """a copy of `func` with pieces of its text replaced (every piece must be there exactly once)"""
    src = inspect.getsource(func)
    for old, new in swaps:
        assert src.count(old) == 1, old
        src = src.replace(old, new)
    scope = dict(vars(nr))
    exec(compile(src, f"<{func.__name__} mutant>", "exec"), scope)
    return scope[func.__name__]


def _tie_free_cloud(n, seed):
    rng = np.random.default_rng(seed)
    return nc.untie((rng.normal(0, 5, (n, 3)) * [4, 3, 0.3]).astype(np.float32))


def _same_tree(a, b):
    """two (nodes, order) in the reference's layout: the same tree up to the order inside buckets?"""
    (na, oa), (nb, ob) = a, b
    if not np.array_equal(na, nb):
        return False
    for x, y in na[(na[:, 1] & 3) == 3]:
        f, c = int(x), int(y) >> 2
        if sorted(oa[f:f + c]) != sorted(ob[f:f + c]):
            return False
    return True


@pytest.mark.parametrize("n,seed", [(1, 1), (8, 2), (9, 3), (700, 4), (4097, 5)])
def test_build_is_both_restatements_on_tie_free_clouds(n, seed):
    tgt = _tie_free_cloud(n, seed)
    assert nc.tie_free(tgt)
    qry = _tie_free_cloud(300, seed + 100)
    mine = nr.build(tgt)
    theirs = nabo.NaboTree(tgt.astype(np.float64))
    assert nr.legal(*mine, tgt) == []
    assert _same_tree(mine, nr.from_oracle(theirs))
    tree = nr.Tree(mine[0], tgt[mine[1]], mine[1])
    for eps in (0.0, 0.5, 3.16):
        ids_c, d2_c, leaves_c = cref.nn_nabo(tgt.astype(np.float64), qry.astype(np.float64), eps)
        leaves = 0
        for k, q in enumerate(qry):
            w = nr.walk(tree, q, eps)
            j, d2, lv = theirs.knn1(q.astype(np.float64), eps)
            leaves += len(w.leaves)
            if not w.decidable:      # (1 + eps)^2 is a float32 here and a float64 there: only a comparison within roundings can differ
                continue
            assert (w.id, len(w.leaves)) == (j, lv) and w.id == ids_c[k], (eps, k)
            assert abs(w.d2 - d2) <= 4 * 2.0 ** -53 * d2 and abs(w.d2 - d2_c[k]) <= 4 * 2.0 ** -53 * d2
        # the library returns the leaf TOTAL alone, so it can only be compared when every query is decidable: the seeds are such
        assert sum(not nr.walk(tree, q, eps).decidable for q in qry) == 0
        assert leaves == leaves_c


@pytest.mark.parametrize("name", nc.LATTICE_CLOUDS)
@pytest.mark.parametrize("n", [9, 65, 1025])
def test_legal_accepts_both_builds_of_tied_clouds(name, n):
    """oracle.nabo.NaboTree leaves equal keys where numpy's argpartition puts them, build where its rule does: both are libnabo
    trees.  (The C restatement keeps its tree to itself; its ANSWERS are compared above.)"""
    tgt = (nc.LATTICE_CLOUDS[name](n).astype(np.float64) - nc.OFFSET).astype(np.float32)
    assert nr.legal(*nr.build(tgt), tgt) == []
    assert nr.legal(*nr.from_oracle(nabo.NaboTree(tgt.astype(np.float64))), tgt) == []


WRONG_BUILDERS = {
    "left = count / 2": [("left = count - count // 2", "left = count // 2")],
    "cut dimension from the segment's own bounds": [("cd = _arg_max(mx - mn)",
                                                     "cd = _arg_max(pts[order[first:first + count]].max(axis=0) - pts[order[first:first + count]].min(axis=0))")],
    "cutVal from rank left - 1": [("cut = pts[seg[left], cd]", "cut = pts[seg[left - 1], cd]")],
}


@pytest.mark.parametrize("what", WRONG_BUILDERS)
def test_legal_rejects_wrong_builders(what):
    wrong = _mutant(nr.build, *WRONG_BUILDERS[what])
    caught = 0
    for name in ("latin", "coarse"):
        tgt = (nc.LATTICE_CLOUDS[name](1025).astype(np.float64) - nc.OFFSET).astype(np.float32)
        assert nr.legal(*nr.build(tgt), tgt) == []
        caught += bool(nr.legal(*wrong(tgt), tgt))
    tgt = _tie_free_cloud(1025, 9)
    caught += bool(nr.legal(*wrong(tgt), tgt))
    assert caught == 3, what            # on tied and on tie-free clouds alike


def test_legal_rejects_a_lost_point_and_a_fat_leaf():
    tgt = _tie_free_cloud(100, 6)
    nodes, order = nr.build(tgt)
    o2 = order.copy(); o2[3] = o2[4]
    assert nr.legal(nodes, o2, tgt)
    n2 = nodes.copy()
    leaf = np.flatnonzero((n2[:, 1] & 3) == 3)[0]
    n2[leaf, 1] = (9 << 2) | 3
    assert nr.legal(n2, order, tgt)


@pytest.mark.parametrize("name,n", nc.tree_stage_cases())
def test_tree_stage_lattice_clouds_are_lattices(name, n):
    t = nc.LATTICE_CLOUDS[name](n)
    assert len(t) == n
    for eps in nc.LATTICE_EPS:
        assert nr.check_lattice(t, t, nc.OFFSET, nc.Q, eps)
    assert nc.tie_free(t) == (name == "latin" or n == 1)


def test_walk_stage_fixtures_are_lattices_and_hold_the_named_queries():
    for name, t, q in nc.walk_fixtures():
        for eps in nc.LATTICE_EPS:
            assert nr.check_lattice(t, q, nc.OFFSET, nc.Q, eps), name
        assert (~np.isfinite(q[:3])).any(axis=1).all() and np.isfinite(q[3:]).all()
        assert np.linalg.norm(q[3].astype(np.float64) - nc.OFFSET) == 1000.0
    name, t, q = nc.walk_fixtures()[0]
    assert name == "latin1025" and len(q) == 1025 and max(nc.QUERY_COUNTS) == 1025


def test_check_lattice_refuses_inexact_fixtures():
    t = nc.latin(1025)
    q = nc.lattice_queries(t)
    with pytest.raises(AssertionError):
        nr.check_lattice(t[:-1], q, nc.OFFSET, nc.Q, 0.0)                 # no longer symmetric: OFFSET is not the mean
    with pytest.raises(AssertionError):
        nr.check_lattice(t, q, nc.OFFSET, nc.Q, 3.16)                     # (1 + eps)^2 no power of two
    with pytest.raises(AssertionError):
        nr.check_lattice(t, q + np.float32(0.125), nc.OFFSET, nc.Q, 0.0)  # queries off the lattice
    with pytest.raises(AssertionError):
        nr.check_lattice(nc.latin(4097), q, nc.OFFSET, nc.Q, 0.0)         # distances beyond 2^24 quanta^2
    far = q.copy(); far[3, 0] += 3000.0
    with pytest.raises(AssertionError):
        nr.check_lattice(t, far, nc.OFFSET, nc.Q, 0.0)


def test_lattice_walks_are_decidable_and_u_free():
    """on a lattice the roundings are zero: the walk with u = 2^-24 may call a tie undecidable, never change an answer"""
    name, t, q = nc.walk_fixtures()[1]
    tree = nr.tree_of_build((t.astype(np.float64) - nc.OFFSET).astype(np.float32))
    qq, firm = nr.queries(q, np.eye(4), nc.OFFSET)
    assert firm.all()
    ties = 0
    for eps in nc.LATTICE_EPS:
        for a, b in zip(nr.walk_all(tree, qq, eps, u=0.0), nr.walk_all(tree, qq, eps)):
            assert a.decidable and (a.id, a.d2, a.leaves, a.slack) == (b.id, b.d2, b.leaves, b.slack)
            ties += not b.decidable
    assert ties > 0


# the six wrong walks of the issue, as replacements in walk's own text
WRONG_WALKERS = {
    "off[cd] not restored after the far side": [("            off[cd] = old_off\n", "")],
    "rd = new_off^2 without the old_off^2 term": [("rd = rd + (-old_off * old_off + new_off * new_off)", "rd = rd + new_off * new_off")],
    "prune with <=": [("        if x < best:\n            off[cd] = new_off", "        if x <= best:\n            off[cd] = new_off")],
    "far child first": [("(arg[n] + 1, arg[n]) if new_off > 0 else (arg[n], arg[n] + 1)",
                         "(arg[n], arg[n] + 1) if new_off > 0 else (arg[n] + 1, arg[n])")],
    "E2 left out": [("x, best = rd * E2, st[0]", "x, best = rd, st[0]")],
    "new_off >= 0 goes right": [("if new_off > 0 else", "if new_off >= 0 else")],
}


@pytest.fixture(scope="module")
def lattice_walks():
    out = []
    for name, t, q in nc.walk_fixtures():
        tree = nr.tree_of_build((t.astype(np.float64) - nc.OFFSET).astype(np.float32))
        qq, _ = nr.queries(q, np.eye(4), nc.OFFSET)
        out.append((name, tree, qq, {eps: nr.walk_all(tree, qq, eps, u=0.0) for eps in nc.LATTICE_EPS}))
    return out


@pytest.mark.parametrize("what", WRONG_WALKERS)
def test_the_lattice_queries_catch_wrong_walkers(what, lattice_walks):
    """Power of the cases: each wrong walk changes an id or a leaf count on a (decidable) query of the lattice fixtures."""
    wrong = _mutant(nr.walk, *WRONG_WALKERS[what])
    caught = []
    for name, tree, qq, right in lattice_walks:
        for eps in nc.LATTICE_EPS:
            if what == "E2 left out" and eps == 0.0:
                continue                                        # (1 + 0)^2 = 1: nothing is left out
            for k, q in enumerate(qq):
                w, r = wrong(tree, q, eps, 0.0), right[eps][k]
                assert r.decidable
                if (w.id, len(w.leaves)) != (r.id, len(r.leaves)):
                    caught.append((name, eps, k))
    assert caught, what
    if what == "new_off >= 0 goes right":                        # what the cut-plane queries are there for
        assert any(name == "latin1025" for name, _, _ in caught)


def _undecidable_share(target_f32_raw, src_f32, pose, eps, take=None):
    t = np.asarray(target_f32_raw, dtype=np.float32)
    mu = t.astype(np.float64).mean(axis=0)
    tree = nr.tree_of_build((t.astype(np.float64) - mu).astype(np.float32))
    q, firm = nr.queries(src_f32, pose, mu)
    if take is not None:
        q, firm = q[take], firm[take]
    walks = nr.walk_all(tree, q, eps)
    bad = sum((not w.decidable) or (not f) for w, f in zip(walks, firm))
    return bad / len(q), walks


@pytest.mark.parametrize("eps", [3.16, 0.5, 0.0])
def test_velo20k_undecidable_share_is_under_its_cap(velo20k, eps, capsys):
    share, walks = _undecidable_share(velo20k["q"].astype(np.float32), velo20k["src"], velo20k["guess"], eps, take=nc.VELO_TAKE)
    with capsys.disabled():
        print(f"\n[velo20k eps {eps}] undecidable share {share:.5f} of {len(walks)} queries, "
              f"{np.mean([len(w.leaves) for w in walks]):.1f} leaves per query")
    assert share < UNDECIDABLE_CAP


@pytest.mark.parametrize("n", nc.DEEP_SIZES)
def test_deep_targets_undecidable_share_is_under_its_cap(n, capsys):
    share, walks = _undecidable_share(nc.normal_cloud(n), nc.normal_queries(), np.eye(4), 3.16)
    with capsys.disabled():
        print(f"\n[normal cloud {n}] undecidable share {share:.5f} of {len(walks)} queries")
    assert share < UNDECIDABLE_CAP


@pytest.mark.parametrize("shift", [0.0, nc.STRIDED_SHIFT])
@pytest.mark.parametrize("nt", [nc.SHALLOW_MAX, nc.SHALLOW_MAX + 1])
def test_align_fixture_undecidable_share_is_under_its_cap(nt, shift):
    """at the guesses of the checked slots, every query (the second search's pose is the device's own: asserted there)"""
    t, _, src, guesses = nc.batch_case(nt, shift)
    # the sizes tests/cpp/test_icp_plan.cc (nabo_exact_cases) pins the launch shapes for
    assert (len(src), len(guesses), nc.SHALLOW_MAX) == (7700, 32, 8 << 12) and nc.BATCH_NS == 7700 and nc.BATCH_SLOTS == 32
    for s in nc.BATCH_CHECKED:
        share, _ = _undecidable_share(t, src, guesses[s], 3.16)
        assert share < UNDECIDABLE_CAP, (s, share)


def test_the_segment_threshold_is_the_headers():
    """nc.SEGMENT_THRESHOLD: the smallest cloud one of whose levels has more segments than kd_median_tree.h's LDS histogram
    words hold pairs of fill counters for (2 S <= kKdHistWords)."""
    words = nc.kd_hist_words()
    assert words == 16384

    def most_segments(n):
        level, most = [n], 1
        while any(c > nr.BUCKET for c in level):
            level = [h for c in level if c > nr.BUCKET for h in (c - c // 2, c // 2)]
            most = max(most, len(level))
        return most

    assert 2 * most_segments(nc.SEGMENT_THRESHOLD) > words >= 2 * most_segments(nc.SEGMENT_THRESHOLD - 1)


def test_certificate_displacement_keeps_the_reference_walk():
    """The slack the reference reports is sound in its own arithmetic: a query moved by 0.9 x slack (less two ulp of its largest
    coordinate) along the directions the GPU test uses names the same point through the same leaves."""
    name, t, q = nc.walk_fixtures()[0]
    tree = nr.tree_of_build((t.astype(np.float64) - nc.OFFSET).astype(np.float32))
    qq, _ = nr.queries(q[4:260], np.eye(4), nc.OFFSET)
    rng = np.random.default_rng(5)
    moved = 0
    for q0 in qq:
        w = nr.walk(tree, q0, 3.0, u=0.0)
        for q1 in nr.displaced(tree, q0, w, w.slack, rng):
            v = nr.walk(tree, q1, 3.0, u=0.0)
            assert (v.id, v.leaves) == (w.id, w.leaves)
            moved += 1
    assert moved > 500
