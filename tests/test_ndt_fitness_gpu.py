"""Ndt's fitness search query by query (ndt_fit_near / ndt_fit_mid / ndt_fit_far behind pcl::Registration::getFitnessScore) against
brute force, through smhip_ndt_debug_fitness -- getFitnessScore's own launches, then every query's distance and the pass that
settled it.  Cases and conditions: tests/ndt_fitness_cases.py; reference, tolerance and stage rules: tests/ndt_fitness_ref.py.

Lattice cases (leaf 1.0, 0.5 and 0.3): the distance of EVERY query bit-equal to the integer brute force; at leaf 1.0 the first pass
settles exactly the queries the rule names; at every leaf no stage breaks its necessary condition and the passes a case was built
for are populated; the score is the exact mean of the returned distances.  Scan cases (30 000 queries against 90 000 points at six
poses, one of them 1e7 m away): every distance inside the derived tolerance; the worst |d2 - d^2| / tolerance of each is printed and
recorded in DESIGN.md section 8.
"""
import numpy as np
import pytest

import ndt_fitness_cases as C
import ndt_fitness_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small():
    """One handle for all lattice cases (a second one for comparisons)."""
    import staticmapping_amd as sm
    ms = [sm.NdtHip(max_source_points=C.MAX_SOURCE, max_target_points=C.MAX_TARGET) for _ in range(2)]
    yield ms
    for m in ms:
        m.close()


def _caller_order(m, per_slot, slot=0):
    """(d2, stage) of a slot from device order to the order of the uploaded rows; every row exactly once."""
    d2, stage, score = per_slot
    _, idx = m.get_source(slot)
    assert len(idx) == len(d2) and sorted(idx.tolist()) == list(range(len(d2)))
    a = np.empty_like(d2); b = np.empty_like(stage)
    a[idx] = d2; b[idx] = stage
    return a, b, score, idx


def _run(m, c, leaf, pose=None):
    m.set_ndt_options(resolution=leaf)
    m.set_input_source(c.source()); m.set_input_target(c.target())
    return _caller_order(m, m.debug_fitness([c.pose() if pose is None else pose])[0])


def _check_score(score, d2):
    want = R.score_of(d2)
    assert abs(score - want) <= 1e-12 * abs(want), (score, want)


@pytest.mark.parametrize("name", C.case_names())
def test_lattice_case_every_query_bit_for_bit(name, small):
    c = C.case(name)
    int_d2, cube = C.reference(name)
    want = R.lattice_expected_d2(int_d2)
    d = np.sqrt(int_d2.astype(np.float64)) * R.UNIT
    fin = c.finite_rows()
    failures = []
    for leaf in C.LEAFS:
        d2, stage, score, idx = _run(small[0], c, leaf)
        assert len(d2) == len(fin)
        counts = [int((stage == s).sum()) for s in (-1, 0, 1, 2)]
        wrong = np.nonzero(d2[fin].view(np.uint32) != want.view(np.uint32))[0]
        print(f"{name} leaf {leaf}: {len(d2)} queries, stages -1/0/1/2 = {counts}, {len(wrong)} distances off")
        if len(wrong):
            k = wrong[0]
            failures.append((leaf, "distance", len(wrong), int(k), c.query_u[k].tolist(), float(d2[fin][k]) * 4096, int(int_d2[k]), int(stage[fin][k])))
        # rows that are not finite: +inf, stage -1, and out of the score
        if not (np.isposinf(d2[~fin]).all() and (stage[~fin] == -1).all() and (stage[fin] >= 0).all()):
            failures.append((leaf, "non-finite rows", d2[~fin].tolist(), stage[~fin].tolist()))
        _check_score(score, d2)
        st = stage[fin]
        bad = R.stage_violations(st, d, leaf, R.table_margin(c.target(), leaf))
        if len(bad):
            failures.append((leaf, "stage breaks its necessary condition", len(bad), int(bad[0]), int(st[bad[0]]), float(d[bad[0]])))
        if leaf == 1.0:
            settle = R.settles_in_the_fine_cube(cube)
            off = np.nonzero((st == 0) != settle)[0]
            if len(off):
                failures.append((leaf, "first pass settles another set", len(off), int(off[0]), int(st[off[0]]), int(cube[off[0]])))
        # the passes the case was built for
        if c.expect == "all2" and not (st == 2).all():
            failures.append((leaf, "not every query went through the sweep", counts))
        if c.expect in ("open", "all_open") and not (st >= 1).any():
            failures.append((leaf, "no query past the fine cube", counts))
        if c.expect == "all_open" and not (st >= 1).all():
            failures.append((leaf, "a query settled in the fine cube", counts))
        if c.expect == "none_open" and not (st == 0).all():
            failures.append((leaf, "a query stayed open", counts))
        if c.expect == "lane255":
            dev_stage = stage[idx]                                            # device order
            if not ((dev_stage[:255] == 0).all() and dev_stage[255] >= 1 and len(dev_stage) == 256):
                failures.append((leaf, "not exactly lane 255 open", np.nonzero(dev_stage)[0].tolist()))
    if name == "corner":
        kind = np.array(c.notes["kind"])
        d2, stage, _, _ = _run(small[0], c, 1.0)
        assert (stage[kind == "corner"] == 1).all() and (stage[kind == "bound16"] == 1).all() and (stage[kind == "bound14"] == 0).all()
    assert not failures, failures


def test_nonfinite_rows_leave_the_other_rows_as_they_are(small):
    c, twin = C.case("nonfinite"), C.case("sizes/n65")
    for leaf in C.LEAFS:
        a2, as_, ascore, _ = _run(small[0], c, leaf)
        b2, bs, bscore, _ = _run(small[1], twin, leaf)
        fin = c.finite_rows()
        assert a2[fin].tobytes() == b2.tobytes() and as_[fin].tobytes() == bs.tobytes()
        assert ascore == bscore or abs(ascore - bscore) <= 1e-12 * bscore       # the same addends, perhaps in another order


@pytest.fixture(scope="module")
def scan():
    import staticmapping_amd as sm
    src, tgt, T = C.scan_clouds()
    m = sm.NdtHip(max_source_points=len(src), max_target_points=len(tgt))
    m.set_input_source(src); m.set_input_target(tgt)
    yield m, src, tgt
    m.close()


@pytest.mark.parametrize("pose", ["on", "half_off", "40m", "turned30", "500m", "1e7m"])
def test_scan_case_every_query_inside_the_derived_tolerance(pose, scan):
    m, src, tgt = scan
    G = C.scan_poses()[pose]
    d, tol = R.scan_reference(src, tgt, G)
    d2, stage, score, _ = _caller_order(m, m.debug_fitness([G])[0])
    assert len(d2) == len(src) and np.isfinite(d2).all()
    ratio = np.abs(d2.astype(np.float64) - d * d) / tol
    k = int(np.argmax(ratio))
    counts = [int((stage == s).sum()) for s in (0, 1, 2)]
    print(f"scan {pose}: stages 0/1/2 = {counts}, worst |d2 - d^2| / tolerance = {ratio[k]:.4f} at query {k} (d = {d[k]:.6g} m, stage {stage[k]})")
    assert (ratio <= 1.0).all(), (pose, int((ratio > 1).sum()), k, float(ratio[k]), float(d2[k]), float(d[k] ** 2), int(stage[k]))
    # the rules bound the device's own float distance, which |d2 - d^2| <= tol keeps within min(tol / d, sqrt(tol)) of d
    slack = np.minimum(tol / np.maximum(d, 1e-300), np.sqrt(tol))
    marg = R.table_margin(tgt, 1.0)
    assert len(R.stage_violations(stage, np.where(stage == 2, d + slack, np.maximum(d - slack, 0.0)), 1.0, marg)) == 0
    _check_score(score, d2)
    if pose in ("500m", "1e7m"):
        assert (stage == 2).all()
    if pose == "40m":
        assert counts[2] > len(src) // 2
    if pose == "on":
        assert all(n > 0 for n in counts)


def test_hook_score_is_the_align_score_bit_for_bit(scan, small):
    """After align() -- which enqueues the search speculatively behind the predicted rounds -- the hook at the returned pose gives
    get_fitness_score()'s bits: it observes the production path."""
    m, src, tgt = scan
    G = C.scan_poses()["on"].copy(); G[0, 3] -= 0.3
    for cache in (False, True, True):
        m.set_target_cache(cache)
        ok, T = m.align(G)
        got = m.debug_fitness([T])[0][2]
        assert np.float64(got).tobytes() == np.float64(m.get_fitness_score()).tobytes(), (cache, got, m.get_fitness_score())
    m.set_target_cache(True)
    c = C.case("sizes/n257")
    s = small[0]
    s.set_ndt_options(resolution=1.0)
    s.set_input_source(c.source()); s.set_input_target(c.target())
    ok, T = s.align(c.pose())
    assert np.float64(s.debug_fitness([T])[0][2]).tobytes() == np.float64(s.get_fitness_score()).tobytes()


@pytest.mark.parametrize("cache", [True, False])
def test_no_state_left_behind(cache, small):
    """Two calls at different poses, then the first pose again: the first call's bits (lists, counters, table)."""
    m = small[0]
    m.set_target_cache(cache)
    try:
        c = C.case("walls")
        m.set_ndt_options(resolution=1.0)
        m.set_input_source(c.source()); m.set_input_target(c.target())
        A = c.pose()
        B = c.pose(); B[:3, 3] += (1.25, -2.0, 0.5)
        Z = c.pose(); Z[:3, 3] += (40.0, 0.0, 0.0)                           # everything through the sweep
        first = _caller_order(m, m.debug_fitness([A])[0])
        other = _caller_order(m, m.debug_fitness([B])[0])
        far = _caller_order(m, m.debug_fitness([Z])[0])
        again = _caller_order(m, m.debug_fitness([A])[0])
        assert (far[1] == 2).all() and (first[1] == 0).any() and (first[1] == 1).any()
        assert first[0].tobytes() != other[0].tobytes()
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes() and first[2] == again[2]
    finally:
        m.set_target_cache(True)


def test_batch_returns_the_single_calls_bits(small):
    """Three slots with different targets and source sizes (65 queries next to 1 025) at first_slot = 2 of a five-slot handle."""
    import staticmapping_amd as sm
    names = ["sizes/n65", "sizes/n1025", "runs"]
    single = []
    for n in names:
        c = C.case(n)
        d2, stage, score, _ = _run(small[0], c, 1.0)
        single.append((d2, stage, score))
    mb = sm.NdtHip(max_source_points=C.MAX_SOURCE, max_target_points=C.MAX_TARGET, pair_slots=5)
    try:
        for k, n in enumerate(names):
            c = C.case(n)
            mb.set_input_source(c.source(), slot=2 + k); mb.set_input_target(c.target(), slot=2 + k)
        for rep in range(2):                                                 # second pass: the tables are kept
            out = mb.debug_fitness([C.case(n).pose() for n in names], first_slot=2)
            for k in range(3):
                d2, stage, score, _ = _caller_order(mb, out[k], slot=2 + k)
                assert d2.tobytes() == single[k][0].tobytes() and stage.tobytes() == single[k][1].tobytes(), (rep, names[k])
                assert score == single[k][2], (rep, names[k])
    finally:
        mb.close()


def test_hook_error_conventions():
    import staticmapping_amd as sm
    from staticmapping_amd import _capi
    c = C.case("sizes/n65")
    m = sm.NdtHip(max_source_points=C.MAX_SOURCE, max_target_points=C.MAX_TARGET)
    try:
        with pytest.raises(sm.SmhipError) as e:
            m.debug_fitness([np.eye(4)])
        assert e.value.status == 4                                           # SMHIP_ERR_NOT_READY
        m.set_input_source(c.source())
        with pytest.raises(sm.SmhipError) as e:
            m.debug_fitness([np.eye(4)])
        assert e.value.status == 4
        m.set_input_target(c.target())
        g = np.ascontiguousarray(np.eye(4).reshape(-1))
        d2 = np.full(64, -7.0, np.float32); stage = np.full(64, -7, np.int32); score = np.full(1, -7.0)
        st = m._lib.smhip_ndt_debug_fitness(m._h, 0, 1, g.ctypes.data_as(_capi.c_double_p), 64, d2.ctypes.data_as(_capi.c_float_p),
                                            stage.ctypes.data_as(_capi.c_int32_p), score.ctypes.data_as(_capi.c_double_p))
        assert st == 7 and "capacity" in m._lib.smhip_last_error(m._h).decode()      # SMHIP_ERR_CAPACITY, nothing written
        assert (d2 == -7).all() and (stage == -7).all() and score[0] == -7
        d2 = np.full(70, -7.0, np.float32); stage = np.full(70, -7, np.int32)
        st = m._lib.smhip_ndt_debug_fitness(m._h, 0, 1, g.ctypes.data_as(_capi.c_double_p), 70, d2.ctypes.data_as(_capi.c_float_p),
                                            stage.ctypes.data_as(_capi.c_int32_p), score.ctypes.data_as(_capi.c_double_p))
        assert st == 0 and (d2[:65] >= 0).all() and (d2[65:] == -7).all() and (stage[65:] == -7).all()     # past ns: left alone
    finally:
        m.close()
