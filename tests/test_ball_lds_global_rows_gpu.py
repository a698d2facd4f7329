"""The global-lookup path of nn_ball_lds's search rounds (sweep_rows_global: a lane takes the rows of its ball four at a time, their
lookups level by level) against the brute-force search and the global-memory ball search, on inputs built for the ways that loop
can go wrong: the second word of a row, clipped and empty blocks, the remainder of the row batch, run lengths around the
four-at-a-time sweep, ties across rows and batches, empty balls, lanes that do not search.

The harness is that of test_ball_lds_rounds_gpu.py: 64 pair slots on one stream (no_overlap = 1) with one 4 096-point cloud among small
ones, so that the batched kernels run; split_after = -1 keeps every iteration in the search kernel.  Two batches -- the default
0.3 m radius (3-4 cells of 0.25 m an axis: 9-16 rows a ball) and a 0.5 m radius (5-6 cells an axis: up to 36 rows, and 5 rows once
clipped to a single slab) -- are each aligned for one and for three iterations by the three searches; every test reads those runs.
Every case sends its rounds down the global path: the box of a round of 256 queries has more than 1 024 table entries, asserted on
the host from the device's grid and query order.  (A grid has at least two cells an axis -- grid_setup_pair: floor(extent / h) + 2 --
so the flattest grid there is, a target in one z-plane, has nz = 2 and not 1.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SLOTS = 64
BIG = 4096                                                 # 64 slots x 8 workgroups: the batched kernels run; 16 full rounds
TABLE_CAP, ROW_CAP = 1024, 256                             # kLdsTableCap, kLdsRowCap (smhip_device.h)
POINT_CAP, POINT_CAP_FIRST = 512, 768                      # kLdsPointCap, and kLdsPointCapFirst: iteration 0's instantiation
ROWS_AT_A_TIME = 4                                         # sweep_rows_global's batch
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


def _source(rng, pts, T, noise=0.005):
    """Rows (x, y, z, 0) of float32: pts + noise seen from the frame T maps into the target's."""
    p = pts + rng.normal(0.0, noise, size=pts.shape)
    s = (p - T[:3, 3]) @ T[:3, :3]                              # R^T (p - t)
    return np.concatenate([s, np.zeros((len(s), 1))], axis=1).astype(np.float32)


def _case(src, q, n, guess, **tags):
    return dict(src=np.ascontiguousarray(src, dtype=np.float32), q=np.asarray(q, dtype=np.float64), n=np.asarray(n, dtype=np.float64), guess=guess, **tags)


def _line(rng, TRUE, NEAR):
    """4 096 queries along a 200 m x 1 m x 1 m beam (800 cells, 25 words a row, 6 x 6 rows): every alignment of a ball's [x0, x1] to
    the 32-cell words; a round spans ~50 cells in x."""
    x = np.sort(rng.uniform(0, 200, size=1600))
    ql = np.stack([x, rng.uniform(-0.5, 0.5, 1600), rng.uniform(-0.5, 0.5, 1600)], axis=1)
    return _case(_source(rng, ql[rng.integers(0, 1600, size=BIG)], TRUE), ql, _normals(rng, 1600), NEAR)


def _fill(cases, filler):
    while len(cases) < SLOTS:
        cases.append(filler)
    return cases


def _cases_default():
    """The 64 slots of the batch with the default radius (0.3 m) and cell (0.25 m)."""
    TRUE, NEAR, FAR = _poses()
    rng = np.random.default_rng(23)
    cases, name = [], {}

    def add(key, c):
        name[key] = len(cases)
        cases.append(c)

    add("line", _line(rng, TRUE, NEAR))
    # a 4 m cube of 700 points; queries within 0.38 m of its faces, inside and outside, and 24 queries 2 m and more outside
    qc = rng.uniform(0, 4, size=(700, 3)); nc = _normals(rng, 700)
    p = rng.uniform(-0.38, 4.38, size=(4000, 3))
    p = p[((p < 0.45) | (p > 3.55)).any(axis=1)][:232]
    far = rng.uniform(0, 4, size=(24, 3)); far[:, 0] = np.where(np.arange(24) % 2 == 0, -2.0, 6.5); far[12:, [0, 1]] = far[12:, [1, 0]]
    add("faces", _case(_source(rng, np.concatenate([p, far]), TRUE, noise=0.0), qc, nc, NEAR))
    # the flattest grid: 500 target points in the plane z = 0 over 6 m x 6 m (nz = 2), queries up to 0.28 m off it
    qf = np.concatenate([rng.uniform(0, 6, size=(500, 2)), np.zeros((500, 1))], axis=1)
    pf = qf[rng.integers(0, 500, size=256)] + np.concatenate([np.zeros((256, 2)), rng.uniform(-0.28, 0.28, size=(256, 1))], axis=1)
    add("flat", _case(_source(rng, pf, TRUE), qf, _normals(rng, 500), NEAR))
    # run lengths: 64 sites 2.5 m apart, at each a pile of 1, 2, 4, 5 or 9 points within 2 cm, at every third a second pile two rows
    # (0.5 m) up in y; four queries a site up to 0.28 m off the pile in every axis -- the pile lies in any row of their balls
    site = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), axis=-1).reshape(-1, 3) * 2.5
    piles = []
    for s_, c in enumerate(site):
        k = (1, 2, 4, 5, 9)[s_ % 5]
        piles.append(c + rng.uniform(-0.01, 0.01, size=(k, 3)))
        if s_ % 3 == 0:
            piles.append(c + (0.0, 0.5, 0.0) + rng.uniform(-0.01, 0.01, size=(k, 3)))
    qr = np.concatenate(piles)
    pr = np.repeat(site, 4, axis=0) + rng.uniform(-0.28, 0.28, size=(256, 3))
    add("runs", _case(_source(rng, pr, TRUE, noise=0.0), qr, _normals(rng, len(qr)), NEAR))
    # ties.  Coordinates on a 2^-6 lattice below 16 m, the identity as guess: the mean, the centred points and the queries are
    # exact in float32 (4 096 target points), so equal distances are equal bit for bit.  The target's least coordinate is 0 in every
    # axis, so the cells' faces lie at (16 k - 8) / 64: two points 8/64 either side of a query lie in neighbouring rows.
    lat = np.unique(rng.integers(1, 512, size=(6000, 3)), axis=0)
    lat = lat[rng.permutation(len(lat))[:3967]] / 64.0          # 3 967 distinct points in an 8 m cube
    dup = lat[:64]                                              # 64 of them twice
    k16 = np.arange(16)
    sub_y, sub_z = (k16 % 4) * 4 / 64.0, (k16 // 4) * 4 / 64.0    # every quarter of a cell: the pairs fall in different rows of the balls
    mid_y = np.stack([9.0 + (k16 % 4) * 1.5, 1.0 + (k16 // 4) * 1.5 + sub_y, 2.0 + sub_z], axis=1)     # far from everything else
    mid_z = np.stack([9.0 + (k16 % 4) * 1.5, 1.0 + (k16 // 4) * 1.5 + sub_y, 5.0 + sub_z], axis=1)
    e = 8 / 64.0
    qt = np.concatenate([lat, dup, mid_y - (0, e, 0), mid_y + (0, e, 0), mid_z - (0, 0, e), mid_z + (0, 0, e), np.zeros((1, 3))])
    assert len(qt) == 4096
    st = np.concatenate([dup + (1 / 64.0, 2 / 64.0, 0), mid_y, mid_z, lat[64:224] + (1 / 64.0, 0, 0)])
    li = np.rint(st[:96] * 64).astype(np.int64); ti = np.rint(qt * 64).astype(np.int64)
    d2i = np.sort(((li[:, None, :] - ti[None, :, :]) ** 2).sum(axis=2), axis=1)     # exact, in lattice units: the two nearest tie, the third is farther
    assert (d2i[:64, :2] == 5).all() and (d2i[:64, 2] > 5).all() and (d2i[64:, :2] == 64).all() and (d2i[64:, 2] > 64).all()
    add("ties", _case(np.concatenate([st, np.zeros((len(st), 1))], axis=1), qt, _normals(rng, 4096), np.eye(4)))
    # nothing within the radius: 400 target points in the plane z = 0 over 8 m x 8 m; of 256 queries 80 % lie 2 cm off a target point,
    # 10 % 0.35 m above one (candidates in the rows of the ball, none within the radius) and 10 % 1.5 m above (no candidate at all):
    # fewer than the 30 % that are trimmed, so their bounds stay above the quantile and are not refined
    qe = np.concatenate([rng.uniform(0, 8, size=(400, 2)), np.zeros((400, 1))], axis=1)
    pe = qe[rng.integers(0, 400, size=256)].copy()
    pe[:, 2] = np.where(np.arange(256) % 10 == 3, 0.35, np.where(np.arange(256) % 10 == 4, 1.5, 0.02))
    add("empty", _case(_source(rng, pe, TRUE, noise=0.002), qe, _normals(rng, 400), NEAR))
    # lanes that do not search.  A row of NaNs has Morton key 0: such rows come first in the device's order -- 40 of them share the
    # first wave of the first round with 24 searching lanes, 64 fill it
    inner = qc[rng.integers(0, 700, size=512)]
    for key, k in (("nan40", 40), ("nan64", 64)):
        s = _source(rng, inner, TRUE)
        bad = rng.choice(512, size=k, replace=False)
        s[bad[: k // 2], :3] = np.nan; s[bad[k // 2:], :3] = np.inf
        add(key, _case(s, qc, nc, NEAR, nan_rows=k))
    # three iterations with full lists: 0.5 m off, and every target point twice -- a query's runner-up is as near as its match, so
    # its certificate fails whatever the poses do
    qv = rng.uniform(0, 3.5, size=(1500, 3)); nv = _normals(rng, 1500)
    add("far", _case(_source(rng, qv[rng.integers(0, 1500, size=1024)], TRUE), np.concatenate([qv, qv]), np.concatenate([nv, nv]), FAR))
    # iteration 0's point cap (these two rounds are NOT global: table and rows fit).  The `cube` construction of
    # test_ball_lds_rounds_gpu.py scaled: 600 / 800 target points in a 0.5 m cube under one round of queries -- between the caps of the
    # other instantiations (512) and of iteration 0's (768): points staged; over both: row tables only
    for key, k in (("cube600", 600), ("cube800", 800)):
        qk = rng.uniform(0, 0.5, size=(k, 3))
        add(key, _case(_source(rng, qk[rng.integers(0, k, size=256)], TRUE, noise=0.002), qk, _normals(rng, k), NEAR))
    return _fill(cases, _case(_source(rng, qc[rng.integers(0, 700, size=300)], TRUE), qc, nc, NEAR)), name


def _cases_wide_ball():
    """The batch with ball_radius = 0.5 on the default 0.25 m cells: 5-6 cells an axis."""
    TRUE, NEAR, FAR = _poses()
    rng = np.random.default_rng(29)
    cases, name = [], {}

    def add(key, c):
        name[key] = len(cases)
        cases.append(c)

    add("line", _line(rng, TRUE, NEAR))
    # row counts: a 6 m x 3 m x 3 m block of 900 points; queries along its two x-edges (y, z) = (0, 0) and (3, 3), up to 0.6 m outside
    # the block and 0.8 m inside: their balls are clipped to 1-6 cells in y and in z
    qb = rng.uniform(0, 1, size=(900, 3)) * (6, 3, 3); nb = _normals(rng, 900)
    p = np.stack([rng.uniform(0, 6, 256), rng.uniform(-0.6, 0.8, 256), rng.uniform(-0.6, 0.8, 256)], axis=1)
    p[128:, 1:] = 3.0 - p[128:, 1:]
    add("rowcounts", _case(_source(rng, p, TRUE, noise=0.0), qb, nb, NEAR))
    qv = rng.uniform(0, 3.5, size=(1500, 3)); nv = _normals(rng, 1500)
    add("far", _case(_source(rng, qv[rng.integers(0, 1500, size=1024)], TRUE), np.concatenate([qv, qv]), np.concatenate([nv, nv]), FAR))
    add("near", _case(_source(rng, qv[rng.integers(0, 1500, size=1024)], TRUE), qv, nv, NEAR))
    return _fill(cases, _case(_source(rng, qb[rng.integers(0, 900, size=300)], TRUE), qb, nb, NEAR)), name


# ---- iteration 0 restated on the host from the device's grid (debug_get_grid) -----------------------------------------------------
def _balls(grid, pts, G, radius):
    """Per query (rows of pts, any order): its position in the grid's frame (float32) and its block of cells lo..hi as
    ball_lds_rounds takes it, and whether the block is non-empty."""
    h = np.float32(grid["h"]); o = grid["origin"].astype(np.float32)
    dims = np.array([grid["nx"], grid["ny"], grid["nz"]])
    qd = (pts.astype(np.float64) @ G[:3, :3].T + G[:3, 3] - grid["mu"]).astype(np.float32)
    rs = np.float32(radius) * np.float32(1.0001) + np.float32(1.0e-3) * h
    with np.errstate(invalid="ignore"):
        lo = np.maximum(np.floor((qd - rs - o) / h), 0); hi = np.minimum(np.floor((qd + rs - o) / h), dims - 1)
        ok = np.isfinite(qd).all(axis=1) & (lo <= hi).all(axis=1)
    lo = np.where(ok[:, None], lo, 0).astype(np.int64); hi = np.where(ok[:, None], hi, -1).astype(np.int64)
    return qd, lo, hi, ok


def _round_entries(lo, hi, ok):
    """Table entries of the box of every round of 256 queries (device order); 0 = no searching lane."""
    out = []
    for r in range(0, len(lo), 256):
        m = ok[r:r + 256]
        if not m.any():
            out.append(0)
            continue
        b0 = lo[r:r + 256][m].min(axis=0); b1 = hi[r:r + 256][m].max(axis=0)
        out.append(int(np.prod(b1 - b0 + (2, 1, 1))))
    return out


def _round_paths(lo, hi, ok, tc):
    """(table entries, rows, target points inside) of the box of every round of 256 queries (device order)."""
    out = []
    for r in range(0, len(lo), 256):
        m = ok[r:r + 256]
        if not m.any():
            out.append((0, 0, 0))
            continue
        b0 = lo[r:r + 256][m].min(axis=0); b1 = hi[r:r + 256][m].max(axis=0)
        nxl, nyl, nzl = (b1 - b0 + (2, 1, 1)).tolist()
        out.append((nxl * nyl * nzl, nyl * nzl, int(((tc >= b0) & (tc <= b1)).all(axis=1).sum())))
    return out


def _target_cells(grid):
    h = np.float32(grid["h"]); o = grid["origin"].astype(np.float32)
    dims = np.array([grid["nx"], grid["ny"], grid["nz"]])
    return np.clip(np.floor((grid["tq"][:, :3] - o) / h), 0, dims - 1).astype(np.int64)


def _walk(grid, tc, qd, lo, hi, radius):
    """The rows of one query's ball in the order of the walk: [(run length, or -1 for a row outside the ball)]."""
    h = np.float32(grid["h"]); o = grid["origin"].astype(np.float32)
    slack = np.float32(2.0e-3) * h; r2 = np.float32(radius) * np.float32(radius)
    inx = (tc[:, 0] >= lo[0]) & (tc[:, 0] <= hi[0])
    rows = []
    for z in range(lo[2], hi[2] + 1):
        zl = o[2] + np.float32(z) * h
        dz = max(max(zl - qd[2], qd[2] - (zl + h)) - slack, np.float32(0))
        for y in range(lo[1], hi[1] + 1):
            yl = o[1] + np.float32(y) * h
            dy = max(max(yl - qd[1], qd[1] - (yl + h)) - slack, np.float32(0))
            rows.append(-1 if dy * dy + dz * dz > r2 else int((inx & (tc[:, 1] == y) & (tc[:, 2] == z)).sum()))
    return rows


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
def wide_batch(smhip):
    cases, name = _cases_wide_ball()
    return dict(cases=cases, name=name, radius=0.5, runs={it: _run_batch(smhip, cases, it, ball_radius=0.5) for it in (1, 3)})


def _compare(batch, iters, slot):
    """As test_ball_lds_rounds_gpu._compare: one slot, the default path against both others."""
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


def _host(batch, key, device_order=True):
    """(grid, target cells, qd, lo, hi, ok) of the case's iteration 0, the queries in the device's order or the caller's."""
    slot = batch["name"][key]
    run = batch["runs"][1]["lds"]
    grid = run["grid"][slot]
    pts = run["dev"][slot][0] if device_order else batch["cases"][slot]["src"][:, :3]
    return (grid, _target_cells(grid)) + _balls(grid, pts, batch["cases"][slot]["guess"], batch["radius"])


def _assert_global(batch, key):
    """Every round of the case's iteration 0 that searches has a box over the table cap."""
    grid, tc, qd, lo, hi, ok = _host(batch, key)
    entries = _round_entries(lo, hi, ok)
    assert any(entries) and all(e == 0 or e > TABLE_CAP for e in entries), (key, entries)


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("which", ["default", "wide"])
def test_second_word_of_a_row(default_batch, wide_batch, which, iters):
    """Queries on a long line along x: balls whose x0 and x1 lie in different 32-cell words, whose x1 is the last cell of a word and
    whose x0 is the first -- the second word, wc, and both pop-count masks."""
    b = default_batch if which == "default" else wide_batch
    _assert_global(b, "line")
    grid, tc, qd, lo, hi, ok = _host(b, "line")
    x0, x1 = lo[ok, 0], hi[ok, 0]
    two = (x0 >> 5) != (x1 >> 5)
    assert grid["wx"] >= 25 and two.sum() >= 100 and (~two).sum() >= 1000
    assert ((x1 & 31) == 31).any() and ((x0 & 31) == 0).any() and (two & ((x1 & 31) == 0)).any() and (two & ((x0 & 31) == 31)).any()
    assert len(set((x0[two] >> 5).tolist())) >= 10                # ... at many different words of the row
    _compare(b, iters, b["name"]["line"])


@pytest.mark.parametrize("iters", [1, 3])
def test_blocks_clipped_by_the_grid(default_batch, iters):
    """Balls clipped by each face of the grid, and balls wholly outside it (an empty block: the lane searches nothing and records
    the radius as its lower bound; more than the trimmed 30 % of this case's queries end that way, so the bounds are refined behind
    the rounds)."""
    b = default_batch
    _assert_global(b, "faces")
    grid, tc, qd, lo, hi, ok = _host(b, "faces")
    dims = np.array([grid["nx"], grid["ny"], grid["nz"]])
    full = hi - lo + 1 >= 3                                       # an unclipped ball spans 3 or 4 cells
    for d in range(3):
        assert (ok & (lo[:, d] == 0) & ~full[:, d]).any() and (ok & (hi[:, d] == dims[d] - 1) & ~full[:, d]).any(), d
    assert (~ok).sum() == 24                                      # the 24 queries 2 m outside
    _compare(b, iters, b["name"]["faces"])


@pytest.mark.parametrize("iters", [1, 3])
def test_the_flattest_grid(default_batch, iters):
    """A target in one z-plane: nz = 2 (the least there is), every ball clipped in z to one or two slabs."""
    b = default_batch
    _assert_global(b, "flat")
    grid, tc, qd, lo, hi, ok = _host(b, "flat")
    assert grid["nz"] == 2 and ok.all() and set((hi[:, 2] - lo[:, 2] + 1).tolist()) == {1, 2}
    _compare(b, iters, b["name"]["flat"])


@pytest.mark.parametrize("iters", [1, 3])
def test_row_counts_around_the_batch(default_batch, wide_batch, iters):
    """Balls of 1, 3, 4, 5, 8, 9 and 16 rows (and 25): the batch's remainder and its trip count."""
    _assert_global(wide_batch, "rowcounts")
    grid, tc, qd, lo, hi, ok = _host(wide_batch, "rowcounts")
    nrows = ((hi[:, 1] - lo[:, 1] + 1) * (hi[:, 2] - lo[:, 2] + 1))[ok]
    assert {1, 3, 4, 5, 8, 9, 16} <= set(nrows.tolist()) and nrows.max() >= 25, sorted(set(nrows.tolist()))
    assert {0, 1, 2, 3} == set((nrows % ROWS_AT_A_TIME).tolist())
    _compare(wide_batch, iters, wide_batch["name"]["rowcounts"])
    # ... and with the default radius: 9, 12 and 16 rows
    grid, tc, qd, lo, hi, ok = _host(default_batch, "runs")
    nrows = ((hi[:, 1] - lo[:, 1] + 1) * (hi[:, 2] - lo[:, 2] + 1))[ok]
    assert {9, 12, 16} <= set(nrows.tolist())


@pytest.mark.parametrize("iters", [1, 3])
def test_run_lengths_around_the_sweep(default_batch, iters):
    """Runs of exactly 0, 1, 2, 4, 5 and 9 points in a row of a ball, an empty row between two occupied ones, and balls whose only
    occupied rows lie in the last batch."""
    b = default_batch
    _assert_global(b, "runs")
    grid, tc, qd, lo, hi, ok = _host(b, "runs")
    assert ok.all()
    lens, gap, last_only, two_in_batch = set(), 0, 0, 0
    for i in range(len(qd)):
        rows = _walk(grid, tc, qd[i], lo[i], hi[i], b["radius"])
        lens |= set(rows)
        occ = [r for r, n in enumerate(rows) if n > 0]
        gap += any(b_ - a_ == 2 and rows[a_ + 1] == 0 for a_, b_ in zip(occ, occ[1:]))
        last_only += bool(occ) and occ[0] // ROWS_AT_A_TIME == (len(rows) - 1) // ROWS_AT_A_TIME and len(rows) > ROWS_AT_A_TIME
        two_in_batch += len({r // ROWS_AT_A_TIME for r in occ}) < len(occ)
    assert {-1, 0, 1, 2, 4, 5, 9} <= lens, sorted(lens)
    assert gap >= 3 and last_only >= 3 and two_in_batch >= 3, (gap, last_only, two_in_batch)
    _compare(b, iters, b["name"]["runs"])


@pytest.mark.parametrize("iters", [1, 3])
def test_ties_across_rows_and_batches(default_batch, iters):
    """A target point that exists twice (one run), and queries exactly half way between two points that lie in different rows of one
    batch and in rows of different batches (lattice coordinates: the distances are equal bit for bit): the match is the one that
    comes first in the sorted target, which the walk meets first."""
    b = default_batch
    slot = b["name"]["ties"]
    _assert_global(b, "ties")
    run = b["runs"][1]["lds"]
    grid, tc, qd, lo, hi, ok = _host(b, "ties", device_order=False)
    assert grid["nt"] == 4096 and np.array_equal(np.rint((grid["origin"] + grid["mu"]) * 64), [-8, -8, -8])     # the faces lie where the case puts them
    caller = grid["tq"][:, 3].copy().view(np.int32)              # caller index by sorted position
    pos = np.empty(len(caller), np.int64); pos[caller] = np.arange(len(caller))
    pairs = [(q0 + k, t0 + k, t0 + 16 + k) for q0, t0 in ((64, 4031), (80, 4063)) for k in range(16)]      # the y-pairs, then the z-pairs
    same_batch = other_batch = 0
    for q, ta, tb in pairs:                                      # the rows of the query's ball the two points lie in
        nyr = hi[q, 1] - lo[q, 1] + 1
        ra, rb = ((tc[pos[t]][2] - lo[q, 2]) * nyr + (tc[pos[t]][1] - lo[q, 1]) for t in (ta, tb))
        assert ra != rb and 0 <= min(ra, rb) and max(ra, rb) < nyr * (hi[q, 2] - lo[q, 2] + 1)
        same_batch += ra // ROWS_AT_A_TIME == rb // ROWS_AT_A_TIME
        other_batch += ra // ROWS_AT_A_TIME != rb // ROWS_AT_A_TIME
    assert same_batch >= 4 and other_batch >= 4, (same_batch, other_batch)
    _compare(b, iters, slot)
    if iters != 1:
        return
    ids, d2 = run["matches"][slot]
    k = np.arange(64)
    first = np.where(pos[k] < pos[3967 + k], k, 3967 + k)
    assert np.array_equal(ids[:64], first) and (d2[:64].view(np.uint32) == np.float32(5.0 / 4096.0).view(np.uint32)).all()
    for q, ta, tb in pairs:
        first = ta if pos[ta] < pos[tb] else tb
        assert ids[q] == first and d2[q].view(np.uint32) == np.float32(1.0 / 64.0).view(np.uint32), (q, ids[q], d2[q])


@pytest.mark.parametrize("iters", [1, 3])
def test_nothing_within_the_radius(default_batch, iters):
    """Queries whose ball holds candidates but none within the radius, and queries whose ball holds none: the radius as the lower
    bound, a seed (iteration 0: the nearest candidate seen, or -1; later: the previous match)."""
    b = default_batch
    slot = b["name"]["empty"]
    _assert_global(b, "empty")
    ids, d2 = b["runs"][1]["lds"]["matches"][slot]
    r2cap = np.float32(0.3) * np.float32(0.3)
    bound = d2.view(np.uint32) == r2cap.view(np.uint32)
    k = np.arange(256) % 10
    assert bound[(k == 3) | (k == 4)].all() and not bound[(k != 3) & (k != 4)].any()
    assert (ids[k == 4] == -1).all() and (ids[k == 3] >= 0).mean() > 0.5     # no candidate at all / a seed outside the radius
    if iters == 3:
        # later iterations: the poses move by millimetres, so these balls stay empty -- a query keeps a lower bound (the radius if it
        # searched again, at least 0.9 of it -- bound_now against r_need -- if its bound was certified without a search), and a seed:
        # the previous match where iteration 0 left one, -1 where it left none
        ids3, d23 = b["runs"][3]["lds"]["matches"][slot]
        assert (d23[(k == 3) | (k == 4)] >= np.float32(0.80) * r2cap).all() and (ids3[k == 4] == -1).all()
        assert (ids3[(k == 3) & (ids >= 0)] >= 0).all()
    _compare(b, iters, slot)


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("key", ["nan40", "nan64"])
def test_lanes_that_do_not_search(default_batch, key, iters):
    """Rows of NaN / inf in the first wave of a global round, sharing it with searching lanes or filling it."""
    b = default_batch
    slot = b["name"][key]
    c = b["cases"][slot]
    _assert_global(b, key)
    pts_dev, row = b["runs"][1]["lds"]["dev"][slot]
    bad_dev = ~np.isfinite(pts_dev).all(axis=1)
    k = c["nan_rows"]
    assert bad_dev[:k].all() and not bad_dev[k:].any()
    bad = ~np.isfinite(c["src"][:, :3]).all(axis=1)
    ids, d2 = b["runs"][iters]["lds"]["matches"][slot]
    assert bad.sum() == k and np.isinf(d2[bad]).all() and (ids[bad] == -1).all() and np.isfinite(d2[~bad]).all()
    _compare(b, iters, slot)


@pytest.mark.parametrize("which", ["default", "wide"])
def test_full_lists_in_later_iterations(default_batch, wide_batch, which):
    """Three iterations from 0.5 m off with every target point twice: nearly every certificate fails, every workgroup searches full
    rounds in every iteration -- with the 0.5 m radius balls of more than four rows a slab."""
    b = default_batch if which == "default" else wide_batch
    slot = b["name"]["far"]
    _assert_global(b, "far")
    grid, tc, qd, lo, hi, ok = _host(b, "far")
    if which == "wide":
        assert (hi[ok, 1] - lo[ok, 1] + 1).max() >= 5 and ((hi[ok, 1] - lo[ok, 1] + 1) * (hi[ok, 2] - lo[ok, 2] + 1)).max() >= 25
    counts = b["runs"][3]["lds"]["counts"][slot]
    assert counts[0] == 1024 and counts[1] > 768 and counts[2] > 768, counts[:3]
    _compare(b, 3, slot); _compare(b, 1, slot)


@pytest.mark.parametrize("iters", [1, 3])
def test_a_few_fail_in_later_iterations(wide_batch, iters):
    """Three iterations from 1 cm / 0.03 deg off with the 0.5 m radius: short lists of failing queries with their own radii."""
    b = wide_batch
    _assert_global(b, "near")
    _compare(b, iters, b["name"]["near"])


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("key", ["cube600", "cube800"])
def test_iteration_0_point_cap(default_batch, key, iters):
    """600 and 800 target points in the box of one round whose table and rows fit: iteration 0 stages the points of the first
    (more than the 512 of the other instantiations, no more than its own 768) and looks the second up through the row tables."""
    b = default_batch
    grid, tc, qd, lo, hi, ok = _host(b, key)
    paths = _round_paths(lo, hi, ok, tc)
    assert len(paths) == 1 and ok.all()
    e, r, p = paths[0]
    assert 0 < e <= TABLE_CAP and r <= ROW_CAP, paths
    assert (POINT_CAP < p <= POINT_CAP_FIRST) if key == "cube600" else p > POINT_CAP_FIRST, paths
    _compare(b, iters, b["name"][key])
