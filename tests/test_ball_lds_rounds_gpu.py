"""The rounds of nn_ball_lds<2, .> (ball_lds_rounds) against the brute-force search and the global-memory ball search on inputs built
for their edges: round boundaries, lanes that do not search, every staging cap missed by itself, ties, empty balls, and the merged
list of failing queries of the iterations after the first.

A batch takes the batched kernels when pairs x ceil(ns_max / 512) >= 512 for a part: 64 pair slots on one stream (no_overlap = 1: one
part) with one 4 100-point cloud among small ones; split_after = -1 keeps every iteration in the search kernel.  Two batches (the
default 0.3 m radius / 0.25 m cells, and 0.1 m / 0.5 m cells) are each aligned for one and for three iterations by the three
searches; every test below reads those runs (computed once per module)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SLOTS = 64
BIG = 4100
TABLE_CAP, ROW_CAP, POINT_CAP = 1024, 256, 512           # kLdsTableCap, kLdsRowCap, kLdsPointCap (smhip_device.h)
VARIANTS = {"lds": dict(), "brute": dict(nn_mode=0), "global": dict(no_lds_table=1)}


def _pose(t=(0.0, 0.0, 0.0), rpy=(0.0, 0.0, 0.0)):
    from staticmapping_amd import synth
    return synth.make_pose(t=t, rpy_deg=rpy)


def _poses():
    """The pose the sources of the scenes below were made with, one 1 cm / 0.03 deg from it, one 0.5 m from it."""
    true = _pose(t=(0.30, -0.20, 0.10), rpy=(1.0, -2.0, 3.0))
    return true, true @ _pose(t=(0.01, 0.0, 0.0), rpy=(0.0, 0.0, 0.03)), true @ _pose(t=(0.5, 0.0, 0.0))


def _normals(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _volume(rng, n, lo, hi):
    """n target points uniform in a box, unit normals in random directions (the point-to-plane sums then fix all six freedoms)."""
    return rng.uniform(lo, hi, size=(n, 3)), _normals(rng, n)


def _source(rng, pts, T, noise=0.005):
    """Rows (x, y, z, 0) of float32: pts + noise seen from the frame T maps into the target's."""
    p = pts + rng.normal(0.0, noise, size=pts.shape)
    s = (p - T[:3, 3]) @ T[:3, :3]                              # R^T (p - t)
    return np.concatenate([s, np.zeros((len(s), 1))], axis=1).astype(np.float32)


def _case(src, q, n, guess, **tags):
    return dict(src=np.ascontiguousarray(src, dtype=np.float32), q=np.asarray(q, dtype=np.float64), n=np.asarray(n, dtype=np.float64), guess=guess, **tags)


def _cases_default():
    """The 64 slots of the batch with the default radius and cell."""
    TRUE, NEAR, FAR = _poses()
    rng = np.random.default_rng(7)
    cases, name = [], {}

    def add(key, c):
        name[key] = len(cases)
        cases.append(c)

    # 1 200 target points in a 3 m cube (~5 per 0.3 m ball) under 4 100 queries: a round of 256 Morton-consecutive queries spans ~1.5 m,
    # its box fits the three caps.  The small clouds take their queries from a 1.5 m / 2 m corner of it for the same reason.
    q, n = _volume(rng, 1200, (0, 0, 0), (3, 3, 3))
    pick = rng.integers(0, len(q), size=BIG)
    corner = rng.choice(np.flatnonzero((q < 1.5).all(axis=1)), size=1024)
    corner2 = rng.choice(np.flatnonzero((q < 2.0).all(axis=1)), size=1500)
    add("big_near", _case(_source(rng, q[pick], TRUE), q, n, NEAR))
    for ns in (1, 255, 256, 257, 511, 512, 513):                 # round boundaries
        add(f"ns{ns}", _case(_source(rng, q[corner[:ns]], TRUE), q, n, NEAR))
    # the source IS the target: every query lies on its match (to the rounding of the source to float32), every runner-up more than
    # 1 mm away, and the poses move by that rounding -- no certificate can fail after iteration 0
    d2t = ((q[:, None, :] - q[None, :, :]) ** 2).sum(axis=2) + np.eye(len(q))
    assert d2t.min() > 1.0e-6
    add("big_true", _case(_source(rng, q[pick], TRUE, noise=0.0), q, n, TRUE))
    # 0.5 m off, and every target point twice: a query's runner-up is as near as its match, so its certificate fails whatever the
    # poses do -- every workgroup searches two full rounds in every iteration
    q2, n2 = np.concatenate([q, q]), np.concatenate([n, n])
    add("big_far", _case(_source(rng, q[pick], TRUE), q2, n2, FAR))
    add("far700", _case(_source(rng, q[corner2[:700]], TRUE), q2, n2, FAR))            # ... with a partly filled second workgroup
    # lanes that do not search in iteration 0.  A row of NaNs has Morton key 0: such rows come first in the device's order.
    s = _source(rng, q[corner2], TRUE)
    s[7, 0] = np.nan; s[100, 2] = np.inf; s[rng.integers(0, 1500, size=40), 1] = np.nan
    add("nan_scattered", _case(s, q, n, NEAR))
    for key, k in (("nan_wave", 64), ("nan_round", 256)):
        s = _source(rng, q[corner2[:1024]], TRUE)
        s[rng.choice(1024, size=k, replace=False), :3] = np.nan
        add(key, _case(s, q, n, NEAR, nan_rows=k))
    # the table cap alone: 512 queries on a 200 m line -- a round's box is ~400 cells long
    x = np.sort(rng.uniform(0, 200, size=400))
    ql = np.stack([x, rng.uniform(-0.05, 0.05, 400), rng.uniform(-0.05, 0.05, 400)], axis=1)
    add("line", _case(_source(rng, ql[rng.integers(0, 400, size=512)], TRUE), ql, _normals(rng, 400), NEAR))
    # the point cap alone: 2 000 target points in a 0.5 m cube under 512 queries
    qc, nc = _volume(rng, 2000, (0, 0, 0), (0.5, 0.5, 0.5))
    add("cube", _case(_source(rng, qc[rng.integers(0, 2000, size=512)], TRUE, noise=0.002), qc, nc, NEAR))
    # ties.  Coordinates on a 2^-6 lattice below 16 m and 4 096 target points: the mean, the centred points and -- with the identity
    # as guess -- the queries are exact in float32, so equal distances are equal bit for bit.
    lat = np.unique(rng.integers(0, 512, size=(6000, 3)), axis=0)
    lat = lat[rng.permutation(len(lat))[:4000]] / 64.0           # 4 000 distinct points in an 8 m cube
    dup = lat[:64]                                               # 64 of them twice: target rows k and 4000 + k
    k16 = np.arange(16)
    mid = np.stack([9.0 + (k16 % 4) * 1.5, 1.0 + (k16 // 4) * 1.5, np.full(16, 2.0)], axis=1)     # far from everything else
    pair_lo, pair_hi = mid - (0, 8 / 64.0, 0), mid + (0, 8 / 64.0, 0)
    qt = np.concatenate([lat, dup, pair_lo, pair_hi])            # 4 096 rows; pair rows 4064 + k and 4080 + k
    assert len(qt) == 4096
    st = np.concatenate([dup + (1 / 64.0, 2 / 64.0, 0), mid, lat[64:464] + (1 / 64.0, 0, 0)])
    li = np.rint(st[:80] * 64).astype(np.int64); ti = np.rint(qt * 64).astype(np.int64)
    d2i = np.sort(((li[:, None, :] - ti[None, :, :]) ** 2).sum(axis=2), axis=1)     # exact, in lattice units: the two nearest tie, the third is farther
    assert (d2i[:64, :2] == 5).all() and (d2i[:64, 2] > 5).all() and (d2i[64:, :2] == 64).all() and (d2i[64:, 2] > 64).all()
    add("ties", _case(np.concatenate([st, np.zeros((len(st), 1))], axis=1), qt, _normals(rng, 4096), np.eye(4)))
    # exactly 256 and exactly 257 failing queries in one workgroup: a query whose nearest target point exists twice never certifies
    # (its runner-up is as near as its match); the other queries sit 5 mm from a target point with nothing else within the radius
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 3) * 0.75      # 512 points, 0.75 m apart
    for key, k in (("fail256", 256), ("fail257", 257)):
        qf = np.concatenate([g, g[:k]])
        add(key, _case(_source(rng, g, TRUE), qf, _normals(rng, len(qf)), TRUE, fails=k))
    filler = _case(_source(rng, q[corner[:300]], TRUE), q, n, NEAR)
    while len(cases) < SLOTS:
        cases.append(filler)
    return cases, name


def _cases_small_ball():
    """The batch with ball_radius = 0.1, grid_cell = 0.5 (the existing ball_small variant): balls with nothing inside, so that the
    lower-bound / validate / refine path runs behind the rounds; and the row cap by itself, which needs a box two cells thick."""
    TRUE, NEAR, FAR = _poses()
    rng = np.random.default_rng(11)
    cases, name = [], {}

    def add(key, c):
        name[key] = len(cases)
        cases.append(c)

    q, n = _volume(rng, 1200, (0, 0, 0), (3, 3, 3))
    pick = rng.integers(0, len(q), size=BIG)
    add("big_near", _case(_source(rng, q[pick], TRUE), q, n, NEAR))
    add("big_far", _case(_source(rng, q[pick], TRUE), q, n, FAR))                   # nearly every ball is empty
    pts = q[pick[:1500]].copy()
    pts[::4] += (0.0, 0.0, 3.4)                                  # a quarter of the queries 0.4 m and more above every target point (fewer
                                                                 # than the 30 % that are trimmed: their bounds stay above the quantile)
    add("empties", _case(_source(rng, pts, TRUE), q, n, NEAR))
    # the row cap alone: a y-z sheet 9.5 m x 9.5 m, 40 mm thick -- ~21 x 21 rows, one cell (+ 1 column) in x -- under ONE round of queries
    qs = np.stack([rng.uniform(-0.02, 0.02, 3000), rng.uniform(0, 9.5, 3000), rng.uniform(0, 9.5, 3000)], axis=1)
    add("sheet", _case(_source(rng, qs[rng.integers(0, 3000, size=256)], np.eye(4), noise=0.0), qs, _normals(rng, 3000), _pose(t=(0.002, 0.0, 0.0))))
    filler = _case(_source(rng, q[pick[:300]], TRUE), q, n, NEAR)
    while len(cases) < SLOTS:
        cases.append(filler)
    return cases, name


def _round_paths(grid, pts_dev, G, radius):
    """Iteration 0 restated on the host: per round of 256 queries (device order) the box of its balls as ball_lds_rounds takes it
    -> (table entries, rows, target points inside)."""
    h = np.float32(grid["h"]); o = grid["origin"].astype(np.float32)
    dims = np.array([grid["nx"], grid["ny"], grid["nz"]])
    qd = (pts_dev.astype(np.float64) @ G[:3, :3].T + G[:3, 3] - grid["mu"]).astype(np.float32)
    rs = np.float32(radius) * np.float32(1.0001) + np.float32(1.0e-3) * h
    lo = np.maximum(np.floor((qd - rs - o) / h), 0); hi = np.minimum(np.floor((qd + rs - o) / h), dims - 1)
    tc = np.clip(np.floor((grid["tq"][:, :3] - o) / h), 0, dims - 1)
    out = []
    for r in range(0, len(qd), 256):
        ok = np.isfinite(qd[r:r + 256]).all(axis=1) & (lo[r:r + 256] <= hi[r:r + 256]).all(axis=1)
        if not ok.any():
            out.append((0, 0, 0))
            continue
        b0 = lo[r:r + 256][ok].min(axis=0); b1 = hi[r:r + 256][ok].max(axis=0)
        nxl, nyl, nzl = (b1 - b0 + (2, 1, 1)).astype(int)
        out.append((int(nxl * nyl * nzl), int(nyl * nzl), int(((tc >= b0) & (tc <= b1)).all(axis=1).sum())))
    return out


def _run_batch(sm, cases, iters, **opts):
    cap_t = max(len(c["q"]) for c in cases)
    out = {}
    for vname, vopts in VARIANTS.items():
        m = sm.IcpFastHip(pair_slots=SLOTS, max_source_points=BIG, max_target_points=cap_t, max_iteration=iters, early_exit=0, split_after=-1,
                          no_overlap=1, **opts, **vopts)
        for s_, c in enumerate(cases):
            m.set_input_source(c["src"], slot=s_); m.set_input_target(c["q"], c["n"], slot=s_)
        R, sc, st = m.align_batch(SLOTS, [c["guess"] for c in cases])
        res = dict(R=R, sc=sc, st=st, matches=[m.get_matches(len(c["src"]), slot=s_) for s_, c in enumerate(cases)])
        if vname == "lds":
            res["counts"] = [m.search_counts(s_) for s_ in range(SLOTS)]
            if iters == 1:                                       # what iteration 0 saw: the device's query order and the grids
                res["dev"] = [m.get_source(s_) for s_ in range(SLOTS)]
                res["grid"] = [m.debug_get_grid(s_) for s_ in range(SLOTS)]
        m.close()
        out[vname] = res
    return out


@pytest.fixture(scope="module")
def smhip():
    import staticmapping_amd as sm
    from staticmapping_amd import _capi
    assert _capi.load_library().smhip_device_count() >= 1, "no gfx950 device visible"
    return sm


@pytest.fixture(scope="module")
def default_batch(smhip):
    cases, name = _cases_default()
    return dict(cases=cases, name=name, radius=0.3, runs={it: _run_batch(smhip, cases, it) for it in (1, 3)})


@pytest.fixture(scope="module")
def small_ball_batch(smhip):
    cases, name = _cases_small_ball()
    return dict(cases=cases, name=name, radius=0.1, runs={it: _run_batch(smhip, cases, it, ball_radius=0.1, grid_cell=0.5) for it in (1, 3)})


def _compare(batch, iters, slot):
    """As test_wave_search_equals_the_per_query_walks compares two searches, for one slot, lds against both others."""
    runs = batch["runs"][iters]
    a = runs["lds"]
    il, dl = a["matches"][slot]
    r2cap = np.float32(batch["radius"]) * np.float32(batch["radius"])
    for other in ("global", "brute"):
        o = runs[other]
        io, do = o["matches"][slot]
        assert o["st"][slot]["iterations"] == a["st"][slot]["iterations"] == iters
        assert o["st"][slot]["kept"] == a["st"][slot]["kept"] and o["st"][slot]["limit_d2"] == a["st"][slot]["limit_d2"], (other, slot, o["st"][slot], a["st"][slot])
        assert o["R"][slot].tobytes() == a["R"][slot].tobytes() and o["sc"][slot] == a["sc"][slot], (other, slot)
        # a lower-bounded query (nothing within the radius searched) keeps a seed and the radius as its distance: everything at or
        # below the quantile is identical
        lim = a["st"][slot]["limit_d2"]
        kl, ko = dl <= lim, do <= lim
        assert np.array_equal(kl, ko), (other, slot)
        assert dl[kl].tobytes() == do[kl].tobytes() and il[kl].tobytes() == io[kl].tobytes(), (other, slot)
        if iters == 1:                                           # one search from the same state: the same distance bits everywhere
            if other == "global":
                assert dl.tobytes() == do.tobytes(), (slot, int((dl != do).sum()))
            else:
                # the brute-force search has no radius: it agrees wherever the ball search is exact, and where the ball search
                # left a lower bound (the squared radius, bit for bit) the nearest point is at least that far
                same = dl.view(np.uint32) == do.view(np.uint32)
                assert same[do <= r2cap].all(), (slot, int((~same[do <= r2cap]).sum()))
                assert (dl[~same].view(np.uint32) == r2cap.view(np.uint32)).all() and (do[~same] > r2cap).all(), slot


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("key", ["big_near", "ns1", "ns255", "ns256", "ns257", "ns511", "ns512", "ns513"])
def test_round_boundaries(default_batch, key, iters):
    """One round only, a last round with one live lane, a partly filled last wave, and the 4 100-point cloud (a last workgroup of
    4 queries) in one ragged batch."""
    if key != "ns1":                                             # these rounds do take the fully staged path
        paths = _paths(default_batch, key)
        assert all(0 < e <= TABLE_CAP and r <= ROW_CAP and p <= POINT_CAP for e, r, p in paths[:2]), paths
    _compare(default_batch, iters, default_batch["name"][key])


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("key", ["nan_scattered", "nan_wave", "nan_round"])
def test_lanes_that_do_not_search(default_batch, key, iters):
    """Non-finite rows scattered, filling the first wave of a workgroup, and filling its whole first round while the second is live:
    they get d2 = inf and no match, and the other lanes of their rounds are not disturbed."""
    b = default_batch
    slot = b["name"][key]
    c = b["cases"][slot]
    pts_dev, row = b["runs"][1]["lds"]["dev"][slot]
    bad_dev = ~np.isfinite(pts_dev).all(axis=1)
    if "nan_rows" in c:                                          # the rows of NaNs do fill the first wave / round of workgroup 0
        k = c["nan_rows"]
        assert bad_dev[:k].all() and not bad_dev[k:].any() and len(pts_dev) >= 512
    bad = ~np.isfinite(c["src"][:, :3]).all(axis=1)
    ids, d2 = b["runs"][iters]["lds"]["matches"][slot]
    assert bad.any() and np.isinf(d2[bad]).all() and (ids[bad] == -1).all() and np.isfinite(d2[~bad]).all()
    assert b["runs"][1]["lds"]["counts"][slot][0] == len(bad)                # (iteration 0 is published as the cloud's size)
    _compare(b, iters, slot)


def _paths(batch, key):
    slot = batch["name"][key]
    run = batch["runs"][1]["lds"]
    return _round_paths(run["grid"][slot], run["dev"][slot][0], batch["cases"][slot]["guess"], batch["radius"])


@pytest.mark.parametrize("iters", [1, 3])
def test_table_cap_missed_alone(default_batch, iters):
    """Queries on a 200 m line: every round's box has more than 1 024 table entries, few rows, few points -> global lookups."""
    paths = _paths(default_batch, "line")
    assert len(paths) == 2 and all(e > TABLE_CAP and r <= ROW_CAP and p <= POINT_CAP for e, r, p in paths), paths
    _compare(default_batch, iters, default_batch["name"]["line"])


@pytest.mark.parametrize("iters", [1, 3])
def test_point_cap_missed_alone(default_batch, iters):
    """A 0.5 m cube of 2 000 target points under the queries: the table and the rows fit, the points do not -> table only."""
    paths = _paths(default_batch, "cube")
    assert len(paths) == 2 and all(e <= TABLE_CAP and r <= ROW_CAP and p > POINT_CAP for e, r, p in paths), paths
    _compare(default_batch, iters, default_batch["name"]["cube"])


@pytest.mark.parametrize("iters", [1, 3])
def test_row_cap_missed_alone(small_ball_batch, iters):
    """Queries over a thin y-z sheet: more than 256 rows of two table entries each -> table only."""
    paths = _paths(small_ball_batch, "sheet")
    assert len(paths) == 1 and all(e <= TABLE_CAP and r > ROW_CAP for e, r, p in paths), paths
    _compare(small_ball_batch, iters, small_ball_batch["name"]["sheet"])


def test_the_usual_round_is_fully_staged(default_batch):
    """... and the rounds of the ordinary cloud of the batch take the fully staged path (so the cases above are the exceptions)."""
    paths = _paths(default_batch, "big_near")
    staged = [e <= TABLE_CAP and r <= ROW_CAP and p <= POINT_CAP for e, r, p in paths]
    assert len(paths) == 17 and sum(staged) >= 9, paths


@pytest.mark.parametrize("iters", [1, 3])
def test_ties_go_to_the_smallest_sorted_position(default_batch, iters):
    """A target point that exists twice, and a query exactly half way between two points (lattice coordinates: the distances are
    equal bit for bit): the match is the one that comes first in the sorted target."""
    b = default_batch
    slot = b["name"]["ties"]
    _compare(b, iters, slot)
    if iters != 1:
        return
    run = b["runs"][1]["lds"]
    caller = run["grid"][slot]["tq"][:, 3].copy().view(np.int32)            # caller index by sorted position
    pos = np.empty(len(caller), np.int64); pos[caller] = np.arange(len(caller))
    ids, d2 = run["matches"][slot]
    k = np.arange(64)
    first = np.where(pos[k] < pos[4000 + k], k, 4000 + k)
    assert np.array_equal(ids[:64], first) and (d2[:64].view(np.uint32) == np.float32(5.0 / 4096.0).view(np.uint32)).all()
    k = np.arange(16)
    first = np.where(pos[4064 + k] < pos[4080 + k], 4064 + k, 4080 + k)
    assert np.array_equal(ids[64:80], first) and (d2[64:80].view(np.uint32) == np.float32(1.0 / 64.0).view(np.uint32)).all()


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("key", ["big_near", "big_far", "empties"])
def test_empty_balls(small_ball_batch, key, iters):
    """ball_radius = 0.1 on 0.5 m cells: many queries have nothing inside their ball, so lower bounds are recorded and the
    validate / refine path runs behind the rounds."""
    b = small_ball_batch
    slot = b["name"][key]
    r2cap = np.float32(0.1) * np.float32(0.1)
    if key == "empties":                                         # lower bounds are recorded and stay (above the quantile)
        ids, d2 = b["runs"][1]["lds"]["matches"][slot]
        assert (d2.view(np.uint32) == r2cap.view(np.uint32)).mean() > 0.2
    if key == "big_far":                                         # most balls are empty: the quantile reaches the bounds, they are refined
        ids, d2 = b["runs"][1]["brute"]["matches"][slot]
        assert (d2 > r2cap).mean() > 0.5
    _compare(b, iters, slot)


def test_merged_list_empty(default_batch):
    """Three iterations from the true pose with the source on the target: no certificate fails after iteration 0."""
    b = default_batch
    slot = b["name"]["big_true"]
    counts = b["runs"][3]["lds"]["counts"][slot]
    # (finalize_tail publishes an iteration in which no query was counted as the cloud's size; that every query failed instead is
    # excluded by the construction of the case, _cases_default)
    assert counts[0] == BIG and counts[1] == BIG and counts[2] == BIG, counts[:3]
    _compare(b, 3, slot); _compare(b, 1, slot)


def test_merged_list_a_few_fail(default_batch):
    """Three iterations from 1 cm / 0.03 deg off: some certificates fail, fewer than half of a workgroup's -> one search round."""
    b = default_batch
    slot = b["name"]["big_near"]
    counts = b["runs"][3]["lds"]["counts"][slot]
    assert counts[0] == BIG and 0 < counts[1] < BIG // 2, counts[:3]
    _compare(b, 3, slot)


@pytest.mark.parametrize("key", ["big_far", "far700"])
def test_merged_list_nearly_all_fail(default_batch, key):
    """Three iterations from 0.5 m off: nearly every certificate fails -> two search rounds per workgroup."""
    b = default_batch
    slot = b["name"][key]
    ns = len(b["cases"][slot]["src"])
    counts = b["runs"][3]["lds"]["counts"][slot]
    assert counts[0] == ns and counts[1] > 0.75 * ns and counts[2] > 0.75 * ns, counts[:3]
    _compare(b, 3, slot); _compare(b, 1, slot)


@pytest.mark.parametrize("key", ["fail256", "fail257"])
def test_merged_list_of_exactly_256_and_257(default_batch, key):
    """One workgroup of 512 queries of which exactly 256 / 257 fail in every later iteration: one full search round, and a second
    one with a single live lane."""
    b = default_batch
    slot = b["name"][key]
    counts = b["runs"][3]["lds"]["counts"][slot]
    assert counts[0] == 512 and counts[1] == counts[2] == b["cases"][slot]["fails"], counts[:3]
    _compare(b, 3, slot); _compare(b, 1, slot)
