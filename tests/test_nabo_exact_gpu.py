"""nn_mode = NN_NABO decision by decision: the tree kd_build leaves, the walk nn_nabo makes of it and the certificate it stores,
read back through smhip_icp_debug_get_kd_tree and compared with tests/nabo_ref.py -- libnabo's buildNodes with one definite tie
rule, its recurseKnn in float64, recursive, with nothing of the device's stack scheme.

Tree stage: the device's tree obeys every rule of a libnabo tree (nabo_ref.legal) and, where the fixture is a lattice or tie-free,
is nabo_ref.build's node for node.  Walk stage: the reference walks the DEVICE's arrays, so the walk is tested whatever the build
did.  On the lattice fixtures (tests/nabo_cases.py; nabo_ref.check_lattice is asserted on the CPU, tests/test_nabo_ref.py) float32
and float64 coincide: every query must agree in id, in d2 bit for bit and in the leaves visited.  Off the lattice a query is
compared when the reference calls it decidable: when no comparison of its walk lies within the roundings of the device's own
float32 expressions, (r + 1) u A from the operation count, no fitted constant.  Cap on the undecidable share: 0.1 % per fixture."""
import numpy as np
import pytest

from tests import nabo_cases as nc
from tests import nabo_ref as nr

pytestmark = pytest.mark.gpu

U = nr.U
UNDECIDABLE_CAP = 1.0e-3


def _up(n):
    return np.tile([0.0, 0.0, 1.0], (n, 1))


def _handle(ns, nt, eps, **kw):
    import staticmapping_amd as sm
    return sm.IcpFastHip(max_source_points=ns, max_target_points=nt, nn_mode=sm.NN_NABO, nn_epsilon=eps, **kw)


def _find(m, tgt, qry, pose=None):
    m.set_input_source(np.ascontiguousarray(qry, dtype=np.float32))
    m.set_input_target(tgt, _up(len(tgt)))
    ids, d2 = m.find_closests(np.eye(4) if pose is None else pose, len(qry))
    return ids, d2, m.debug_get_kd_tree(0)


def _check_tree(g, tgt_f32, exact_mean, same_as_build, tag=""):
    """What always holds of the device's tree -- and, with same_as_build, its equality with nabo_ref.build node for node: the
    dimension, the cut value's bits and the child layout (the node words), bucket membership and order (the caller indices)."""
    tgt = np.asarray(tgt_f32, dtype=np.float32).astype(np.float64)
    n = len(tgt)
    assert g["nt"] == n, tag
    w = g["tq"][:, 3].copy().view(np.int32)
    assert np.array_equal(np.sort(w), np.arange(n)), tag                            # a permutation of the caller's indices
    mean = tgt.mean(axis=0)
    if exact_mean:
        assert np.array_equal(g["mu"], mean) and np.array_equal(g["mu"], nc.OFFSET), (tag, g["mu"])
    else:                                                                           # n float64 additions, in the device's order
        assert (np.abs(g["mu"] - mean) <= n * 2.0 ** -53 * np.abs(tgt).max(axis=0)).all(), (tag, g["mu"], mean)
    centred = (tgt - g["mu"]).astype(np.float32)
    assert np.array_equal(g["tq"][:, :3], centred[w]), tag
    assert nr.legal(g["nodes"], w, centred) == [], tag
    nodes = g["nodes"]
    leaf = (nodes[:, 1] & 3) == 3
    first, count = nodes[leaf, 0].astype(np.int64), (nodes[leaf, 1] >> 2).astype(np.int64)
    if n > nr.BUCKET:
        assert count.min() >= 4, tag                                                # so that block first >> 2 belongs to one bucket
    at = first[:, None] + np.arange(8)                                              # [leaves, 8] positions, real where below the count
    real = np.arange(8) < count[:, None]
    at = np.where(real, at, 0)
    want = np.where(real[:, None, :], g["tq"][at, :3].transpose(0, 2, 1), np.float32(np.inf))
    assert np.array_equal(g["leaf"][first >> 2], want), tag                         # the x[8] y[8] z[8] blocks, +inf beyond the count
    assert (np.diff(w[at], axis=1) > 0)[real[:, 1:]].all(), tag                     # a bucket's entries by caller index
    if same_as_build:
        ref_nodes, ref_order = nr.build(centred)
        assert np.array_equal(nodes, ref_nodes), (tag, int((nodes != ref_nodes).any(axis=1).argmax()))
        assert np.array_equal(w, ref_order), tag
    return centred, w


def _compare(g, ids, d2, q32, firm, eps, u, lb_check=True, take=slice(None), tag=""):
    """The reference's walk of the device's own arrays against what the device answered.  -> (walks, compared mask, worst d2
    deviation in units of u d2, undecidable count)"""
    w = g["tq"][:, 3].copy().view(np.int32)
    tree = nr.Tree(g["nodes"], g["tq"][:, :3], w)
    assert float(g["max_error2"]) == nr.max_error2(eps), tag
    pos_of = np.empty(len(w), np.int64); pos_of[w] = np.arange(len(w))
    rows = np.arange(len(q32))[take]
    walks, worst, undecided = {}, 0.0, 0
    for k in rows:
        r = nr.walk(tree, q32[k], eps, u)
        walks[k] = r
        if r.id < 0:                                                                # NaN / Inf rows
            assert ids[k] == -1 and d2[k] == np.inf and g["work"][k] == 0 and g["lb"][k] == 0.0, (tag, k)
            continue
        if r.decidable and firm[k]:
            assert ids[k] == r.id, (tag, k, ids[k], r.id)
            assert g["work"][k] == min(len(r.leaves), 255), (tag, k, g["work"][k], len(r.leaves))
            if u == 0.0:
                assert np.float32(r.d2) == d2[k] and float(np.float32(r.d2)) == r.d2, (tag, k, d2[k], r.d2)
            else:
                assert abs(float(d2[k]) - r.d2) <= 4 * u * r.d2, (tag, k, d2[k], r.d2)
                worst = max(worst, abs(float(d2[k]) - r.d2) / (u * r.d2) if r.d2 > 0 else 0.0)
            if lb_check:
                assert 0.0 <= g["lb"][k] <= r.slack, (tag, k, g["lb"][k], r.slack, r.slack_by)   # sound against the formula
        else:                                       # whichever way the rounding fell, the distance belongs to the point named
            undecided += 1
            e = pos_of[ids[k]]
            named = sum((float(q32[k][d]) - (tree.x, tree.y, tree.z)[d][e]) ** 2 for d in range(3))
            assert abs(float(d2[k]) - named) <= 4 * U * named, (tag, k)
    return walks, worst, undecided


# ----------------------------------------------------------------------------------------------------------------------
# tree stage
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nc.LATTICE_CLOUDS)
def test_tree_of_lattice_clouds_is_the_reference_build(name):
    """1 .. 4 097 points (the build's 1 024 threads either side; a root that is a leaf; one split): the tie-free lattice, the coarse
    one with every median tied, exact duplicates, a plane and a line (zero extent on the arg-max's other dimensions)."""
    m = _handle(8, max(nc.TREE_SIZES), 0.0)
    for cloud, n in nc.tree_stage_cases():
        if cloud != name:
            continue
        t = nc.LATTICE_CLOUDS[name](n)
        ids, d2, g = _find(m, t, t[:1])
        _check_tree(g, t, exact_mean=True, same_as_build=True, tag=(name, n))
        assert d2[0] == 0.0 and np.array_equal(t[ids[0]], t[0])
    m.close()


@pytest.mark.parametrize("n", [1025, 4097, nc.SHALLOW_MAX, nc.SHALLOW_MAX + 1, nc.SEGMENT_THRESHOLD, 150_000, nc.TWO_BIT_SIZE])
def test_tree_of_seeded_clouds_is_the_reference_build(n):
    """Tie-free seeded clouds: either side of the shallow / deep switch of the search (8 << 12 points); the smallest cloud one of
    whose levels has more segments than the build's LDS words hold fill counters for (tests/test_nabo_ref.py derives it -- that
    level's segments are leaves, though, and the levels above it rank by counting); 150 000 points, where a level of 2 048
    segments of 73 points is the first to take the radix select with 4-bit digits, in two groups of segments; and 8 192 x 64 + 1
    points, the smallest cloud with a level of 8 192 segments too large to rank by counting: 2-bit digits, two groups."""
    t = nc.normal_cloud(n)
    m = _handle(8, n, 3.16)
    ids, d2, g = _find(m, t, t[:1])
    m.close()
    _check_tree(g, t, exact_mean=False, same_as_build=True, tag=n)
    assert ids[0] == 0 and d2[0] == 0.0


def test_tree_of_a_million_points_is_a_libnabo_tree_and_walks_like_one(capsys):
    """16 384 x 64 + 1 points: a level of 16 384 segments of which one holds 65 points, so that level takes the radix select with
    1-bit digits in two groups of segments and its partition keeps the fill counters in global memory -- forms no smaller cloud
    reaches.  The reference's own build of such a cloud takes ten seconds, so the device's tree is held to the rules (legal: cut
    dimension, left count, both sides of every cut, every point once; the draw has tied coordinates), its blocks to its points,
    and 1 024 queries are walked on it."""
    n = nc.ONE_BIT_SIZE
    t, q = nc.normal_cloud_with_ties(n), nc.normal_queries(1024)
    m = _handle(len(q), n, 3.16)
    ids, d2, g = _find(m, t, q)
    m.close()
    _check_tree(g, t, exact_mean=False, same_as_build=False, tag=n)
    assert g["n_nodes"] == 2 * 131073 - 1                                          # 2^17 - 1 leaves of 8 points, one of 5 and one of 4
    q32, firm = nr.queries(q, np.eye(4), g["mu"])
    walks, worst, undecided = _compare(g, ids, d2, q32, firm, 3.16, U, tag=n)
    with capsys.disabled():
        print(f"\n[normal cloud {n}] {len(walks)} queries: {undecided} undecidable, worst d2 deviation {worst:.2f} u")
    assert undecided < UNDECIDABLE_CAP * len(walks)


# ----------------------------------------------------------------------------------------------------------------------
# walk stage
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", nc.LATTICE_EPS)
def test_lattice_walks_are_the_reference_walks(eps):
    """Every query of every lattice fixture: id, d2 bit for bit, nabo_work == leaves visited -- on cut planes, on target points,
    equidistant from two bucket entries, outside the root box on each face, 1 km away; NaN / Inf rows give -1 and +inf.  The
    stored certificate never exceeds the reference's slack (0 on a cut plane and between two equidistant entries)."""
    m = _handle(1025, 1025, eps)
    for name, t, q in nc.walk_fixtures():
        ids, d2, g = _find(m, t, q)
        _check_tree(g, t, exact_mean=True, same_as_build=True, tag=name)
        q32, firm = nr.queries(q, np.eye(4), g["mu"])
        assert firm.all()
        walks, _, undecided = _compare(g, ids, d2, q32, firm, eps, 0.0, tag=(name, eps))
        assert undecided == 0 and len(walks) == len(q)
    m.close()


def test_query_counts_either_side_of_a_wave_and_a_workgroup():
    name, t, q = nc.walk_fixtures()[0]
    assert len(t) == 1025 and len(q) == 1025
    m = _handle(1025, 1025, 3.0)
    for count in nc.QUERY_COUNTS:
        ids, d2, g = _find(m, t, q[:count])
        q32, firm = nr.queries(q[:count], np.eye(4), g["mu"])
        walks, _, undecided = _compare(g, ids, d2, q32, firm, 3.0, 0.0, tag=count)
        assert undecided == 0 and len(walks) == count and len(g["work"]) == count
    m.close()


@pytest.mark.parametrize("eps", [3.16, 0.5, 0.0])
def test_velo20k_decidable_queries_are_the_reference_walks(velo20k, eps, capsys):
    t = velo20k["q"].astype(np.float32)
    m = _handle(len(velo20k["src"]), len(t), eps)
    ids, d2, g = _find(m, t, velo20k["src"], velo20k["guess"])
    m.close()
    _check_tree(g, t, exact_mean=False, same_as_build=True, tag="velo20k")   # (ties or not: the rule is the documented one)
    q32, firm = nr.queries(velo20k["src"], velo20k["guess"], g["mu"])
    walks, worst, undecided = _compare(g, ids, d2, q32, firm, eps, U, take=nc.VELO_TAKE, tag=("velo20k", eps))
    with capsys.disabled():
        print(f"\n[velo20k eps {eps}] {len(walks)} queries walked by the reference: {undecided} undecidable, worst d2 deviation {worst:.2f} u")
    assert undecided < UNDECIDABLE_CAP * len(walks)


@pytest.mark.parametrize("n", nc.DEEP_SIZES)
def test_deep_targets_decidable_queries_are_the_reference_walks(n, capsys):
    t, q = nc.normal_cloud(n), nc.normal_queries()
    m = _handle(len(q), n, 3.16)
    ids, d2, g = _find(m, t, q)
    m.close()
    q32, firm = nr.queries(q, np.eye(4), g["mu"])
    walks, worst, undecided = _compare(g, ids, d2, q32, firm, 3.16, U, tag=n)
    with capsys.disabled():
        print(f"\n[normal cloud {n}] {len(walks)} queries: {undecided} undecidable, worst d2 deviation {worst:.2f} u")
    assert undecided < UNDECIDABLE_CAP * len(walks)


# ----------------------------------------------------------------------------------------------------------------------
# launch shapes
# ----------------------------------------------------------------------------------------------------------------------
# Which kernels a call launches is the host-only plan's decision (csrc/icp_plan.h); tests/cpp/test_icp_plan.cc (nabo_exact_cases)
# pins it on the CPU for exactly these sizes:
#   find_closests (every test above)         nn_nabo<4, false, .>: four rounds per workgroup, whatever the size
#   one_pair   an Align of one pair          nn_nabo<1, false, .>: one round; then nn_certify<1, true> and the list walk on 31 workgroups
#   two_parts  32 pairs, default overlap     two parts of 16 pairs = 256 workgroups each: the same small forms, batched
#   one_part   32 pairs, no_overlap = 1      512 workgroups, the plan's threshold: nn_nabo<4, false, .> inside an Align, then
#                                            nn_certify<kCertifyItems, true> and the list walk on 96 workgroups per pair
#   strided    the same with SMHIP_NABO_LISTED_BLOCKS = 8: a trip of the list walk covers 8 x 256 queries, so a pair's list of
#              more than 2 048 queries (asserted) takes every workgroup round its stride loop more than once
SLOTS, NS, CHECKED = nc.BATCH_SLOTS, nc.BATCH_NS, nc.BATCH_CHECKED
FORMS = dict(one_pair=(1, {}, None), two_parts=(SLOTS, {}, None), one_part=(SLOTS, dict(no_overlap=1), None),
             strided=(SLOTS, dict(no_overlap=1), 8))


def _align(nt, slots, opts, max_iteration, t, nrm, src, guesses):
    m = _handle(NS, nt, 3.16, pair_slots=slots, max_iteration=max_iteration, early_exit=0, **opts)
    for s in range(slots):
        m.set_input_source(src, slot=s); m.set_input_target(t, nrm, slot=s)
    R, _, stats = m.align_batch(slots, guesses[:slots])
    out = {s: (m.get_matches(NS, slot=s), m.debug_get_kd_tree(s)) for s in (CHECKED if slots > 1 else (0,))}
    m.close()
    return R, stats, out


@pytest.mark.parametrize("nt", [nc.SHALLOW_MAX, nc.SHALLOW_MAX + 1])
@pytest.mark.parametrize("form", FORMS)
def test_align_searches_are_the_reference_walks(form, nt, monkeypatch, capsys):
    """One iteration, then two from the same guess, on a 12-level and an 18-level target.  After the first run get_matches is the
    search at the guess: the full walk in the form's shape.  The first run's result is the pose of the second run's last search,
    in which a query either kept its match by its certificate or was listed and walked again; either way get_matches must be the
    reference's walk of EVERY query at that pose -- a certified query by the certificate's soundness, a listed one by the list walk
    -- and every query of the checked slots (0 / 13 / 31 of a batch) is walked.  From the stats: some queries were certified and
    some walked again.  (The stored word is no longer the bare slack here -- the pair's motion potential is in it -- so it is not
    compared.)"""
    slots, opts, listed_blocks = FORMS[form]
    if listed_blocks:
        monkeypatch.setenv("SMHIP_NABO_LISTED_BLOCKS", str(listed_blocks))      # read when the handle is made
    t, nrm, src, guesses = nc.batch_case(nt, shift=nc.STRIDED_SHIFT if form == "strided" else 0.0)
    R1, _, first = _align(nt, slots, opts, 1, t, nrm, src, guesses)
    R2, stats, second = _align(nt, slots, opts, 2, t, nrm, src, guesses)
    again = []
    for s in first:
        for out, pose in ((first, guesses[s]), (second, R1[s])):
            (ids, d2), g = out[s]
            q32, firm = nr.queries(src, pose, g["mu"])
            walks, _, undecided = _compare(g, ids, d2, q32, firm, 3.16, U, lb_check=False, tag=(form, nt, s))
            assert len(walks) == NS and undecided < UNDECIDABLE_CAP * NS
        assert stats[s]["iterations"] == 2
        again.append(stats[s]["searched_queries"] - NS)
        assert 0 < again[-1] < NS, stats[s]                                       # some certified, some walked again
        if listed_blocks:
            assert again[-1] > listed_blocks * 256, stats[s]                      # more than one trip of the stride loop
    with capsys.disabled():
        print(f"\n[{form}, {nt} points] queries walked again in the second search: {again} of {NS}")


# ----------------------------------------------------------------------------------------------------------------------
# certificates
# ----------------------------------------------------------------------------------------------------------------------
def _displacements_hold(g, q32, walks, eps, u, seed):
    """Soundness directly: a query with lb > 0, moved by 0.9 lb less two ulp of its largest coordinate along five directions and
    rounded to float32, is walked by the reference to the same id through the same leaves in the same order."""
    tree = nr.Tree(g["nodes"], g["tq"][:, :3], g["tq"][:, 3].copy().view(np.int32))
    rng = np.random.default_rng(seed)
    moved = 0
    for k, r in walks.items():
        if r.id < 0 or not g["lb"][k] > 0.0:
            continue
        for q1 in nr.displaced(tree, q32[k], r, g["lb"][k], rng):
            v = nr.walk(tree, q1, eps, u)
            assert (v.id, v.leaves) == (r.id, r.leaves), (k, g["lb"][k], r.slack, r.slack_by)
            moved += 1
    return moved


def test_certificates_of_find_closests(velo20k, capsys):
    """After find_closests the stored word IS the slack: grid_setup / pose_setup zero the pair's motion potential (pot_a, pot_b) and
    with_pot(slack, 0) = slack (icp_kernels.hip); nothing moves the pose before the walk.  lb <= the reference's slack is asserted
    for every decidable query by _compare; here the displaced queries, and how much of the reference's slack the device keeps.
    No lower side follows from the allowances nn_nabo states (2e-5 relative in kd_sqrt_gap, the factor 1.000001, the 1e3 clamp): a
    sibling the walk drops when it is pushed is measured against the best of that moment, which the recursion's best at the
    sibling's turn may undercut by any amount.  So only this: lb == 0 among decidable queries stays under ten times the
    undecidable share."""
    eps = 3.16
    t = velo20k["q"].astype(np.float32)
    m = _handle(len(velo20k["src"]), len(t), eps)
    ids, d2, g = _find(m, t, velo20k["src"], velo20k["guess"])
    m.close()
    q32, firm = nr.queries(velo20k["src"], velo20k["guess"], g["mu"])
    walks, _, undecided = _compare(g, ids, d2, q32, firm, eps, U, take=nc.VELO_TAKE, tag="certificates")
    moved = _displacements_hold(g, q32, walks, eps, U, seed=31)
    ok = [k for k, r in walks.items() if r.id >= 0 and r.decidable and firm[k] and r.slack > 0.0]
    ratio = np.array([g["lb"][k] / walks[k].slack for k in ok])
    zero = int((ratio == 0.0).sum())
    with capsys.disabled():
        print(f"\n[certificates, velo20k eps {eps}] lb / reference slack over {len(ok)} decidable queries: median {np.median(ratio):.3f}, "
              f"1st percentile {np.percentile(ratio, 1):.3f}, lb == 0: {zero}; undecidable {undecided}; {moved} displaced walks")
    assert moved > len(ok)
    assert (ratio <= 1.0).all()
    assert zero / len(ok) <= 10 * undecided / len(walks), (zero, undecided)


def test_certificates_on_a_lattice():
    """The same two soundness checks where float32 is exact, cut-plane and equidistant queries (slack 0) included."""
    name, t, q = nc.walk_fixtures()[0]
    m = _handle(1025, 1025, 3.0)
    ids, d2, g = _find(m, t, q)
    m.close()
    q32, firm = nr.queries(q, np.eye(4), g["mu"])
    walks, _, _ = _compare(g, ids, d2, q32, firm, 3.0, 0.0, tag=name)
    on_plane = [k for k, r in walks.items() if r.id >= 0 and r.slack == 0.0]
    assert len(on_plane) >= 40 and all(g["lb"][k] == 0.0 for k in on_plane)
    assert _displacements_hold(g, q32, walks, 3.0, 0.0, seed=32) > 1000
