"""Device CalculateNormals (csrc/prep_normals.hip, kd_median_tree.h) leaf by leaf against the exact CPU reference
(tests/normals_ref.py), on every path that prepares a target, at the sizes where the two tree builders change form, on tied
and degenerate input.  Membership is exact, means are bit-equal, normals lie within the measured spread x 8 of the exact one.

The cloud the reference sees is the cloud AS THE DEVICE HOLDS IT: the caller's order for prepare_target and
prepare_target_from_target, the Morton order read back with get_source for the calls that build from a source slot.

Figures of the MI355X run (uninformative share per input, worst informative |n_dev - n_exact| / tol): DESIGN.md section 8.

One thing the sizes cannot reach: the forest's radix select switches to 1-bit digits and fill counters in global memory from
8 193 segments in a level, but segments of <= 64 points are ranked by counting instead, so the switch needs a scan of more
than 64 * 8 192 = 524 288 points; with the 150 000-point scan below the levels beyond 8 192 segments are counting levels.
"""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

import normals_ref as nr

pytestmark = pytest.mark.gpu

F = np.float32
BIG = 150_000
SINGLE_SIZES = [3, 4, 7, 8, 9, 14, 15, 56, 57, 64, 65, 112, 113, 1023, 1024, 1025, 7168, 7169, 57344, 57345, 120_000, 150_000]
_REF = {}
FIGURES = []


@functools.lru_cache(maxsize=None)
def base_scan():
    from staticmapping_amd import synth
    a, b, _ = synth.scan_pair("cfg2", n_points=120_000)
    pick = np.random.default_rng(2).choice(len(b), size=BIG - len(a), replace=False)
    return np.ascontiguousarray(np.concatenate([a[:, :4], b[pick, :4]]), dtype=F)


def subset(n, seed=3):
    """n rows of the one 150 000-row cloud (the 120 000-point cfg2 target scan and 30 000 rows of its source scan: a cfg2 scan
    of 150 000 points alone has 14.7 % uninformative leaves by the reference alone, this one 7.4 %), by a seeded choice"""
    base = base_scan()
    if n == len(base):
        return base
    return np.ascontiguousarray(base[np.random.default_rng(1_000_003 * seed + n).choice(len(base), size=n, replace=False)])


def reference(p_dev, normals):
    key = (hashlib.sha1(np.ascontiguousarray(p_dev).tobytes()).hexdigest(), bool(normals))
    if key not in _REF:
        _REF[key] = nr.LeafReference(p_dev, normals=normals)
    return _REF[key]


def check(label, p_dev, target, normals=True, cap=0.10):
    pts, nrm = target
    fig = nr.compare(reference(p_dev, normals), pts, nrm)
    fig["input"] = label
    FIGURES.append(fig)
    print(fig)
    return fig


def handle(slots, ns=BIG, nt=BIG // 4 + 64):
    import staticmapping_amd as sm
    return sm.IcpFastHip(pair_slots=slots, max_source_points=ns, max_target_points=nt)


# ---- the four ways to a prepared target ---------------------------------------------------------------------------------------
def via_raw(m, rows, slot=0):
    M = m.prepare_target(rows, slot=slot)
    return np.ascontiguousarray(rows[:, :3]), m.get_target(M, slot=slot)


def resident(m, rows, slot):
    """the slot's source as the device holds it, after checking that it is a permutation of the uploaded rows named by .w"""
    p_dev, idx = m.get_source(slot)
    assert len(idx) == len(rows) and np.array_equal(np.sort(idx), np.arange(len(rows)))
    assert np.array_equal(p_dev.view(np.uint32), np.ascontiguousarray(rows[idx, :3]).view(np.uint32))
    return p_dev


def via_source(m, rows, src_slot=0, dst_slot=1):
    m.set_input_source(rows, slot=src_slot)
    p_dev = resident(m, rows, src_slot)
    M = m.prepare_target_from_source(src_slot, dst_slot)
    return p_dev, m.get_target(M, slot=dst_slot)


def via_target(m, rows, raw_slot=1, dst_slot=0):
    """smhip_prepare_target_from_target as the IcpUsingPointMatcher chain calls it: a raw target keeps the caller's order"""
    m.set_input_target(np.ascontiguousarray(rows[:, :3]), None, slot=raw_slot)
    n_out = ctypes.c_int32()
    m._check(m._lib.smhip_prepare_target_from_target(m._h, raw_slot, dst_slot, ctypes.byref(n_out)))
    return np.ascontiguousarray(rows[:, :3]), m.get_target(n_out.value, slot=dst_slot)


def via_batch(m, clouds, normals_for, label, batched_upload=True):
    """clouds into source slots 0 .. S-1 (one batched upload or single ones), one prepare_targets_from_sources into the
    same slots' targets; every scan checked for membership and means, those of normals_for for normals too"""
    S = len(clouds)
    if batched_upload:
        m.set_input_sources_batch(clouds, list(range(S)))
    else:
        for k, c in enumerate(clouds):
            m.set_input_source(c, slot=k)
    devs = [resident(m, c, k) for k, c in enumerate(clouds)]
    Ms = m.prepare_targets_from_sources(list(range(S)), list(range(S)))
    out = []
    for k in range(S):
        t = m.get_target(int(Ms[k]), slot=k)
        check(f"{label}[{k}] n={len(clouds[k])}", devs[k], t, normals=k in normals_for)
        out.append(t)
    return out


# ---- sizes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["raw", "from_source", "from_target"])
def test_single_scan_at_every_size(path):
    m = handle(2, nt=BIG)
    go = dict(raw=via_raw, from_source=via_source, from_target=via_target)[path]
    for n in SINGLE_SIZES:
        p_dev, t = go(m, subset(n))
        check(f"{path} n={n}", p_dev, t, normals=True)
    m.close()


def test_one_and_two_points_give_the_no_target_status_and_the_handle_lives():
    import staticmapping_amd as sm
    m = handle(2, ns=1024, nt=1024)
    for n in (1, 2):
        rows = subset(n)
        with pytest.raises(sm.SmhipError, match="produced no target points"):
            m.prepare_target(rows)
        m.set_input_source(rows, slot=0)
        with pytest.raises(sm.SmhipError, match="produced no target points"):
            m.prepare_target_from_source(0, 1)
        with pytest.raises(sm.SmhipError, match="produced no target points"):
            m.prepare_targets_from_sources([0], [1])
        with pytest.raises(sm.SmhipError, match="produced no target points"):
            via_target(m, rows)
        p_dev, t = via_source(m, subset(9))
        check(f"after n={n}: from_source n=9", p_dev, t)
    m.close()


@pytest.mark.parametrize("S", [2, 3, 31])
def test_sort_form_batches(S):
    """fewer than 32 scans: one sort per level over all scans (seg_bits), scans of different sizes"""
    sizes = ([57345, 9, 20_000] + [8, 7, 65, 64, 113, 1025, 7169] + [3_000 + 411 * k for k in range(21)])[:S]
    m = handle(max(S, 2), ns=max(sizes))
    via_batch(m, [subset(n, seed=5 + k) for k, n in enumerate(sizes)], normals_for={0, 1, 2, S - 1}, label=f"batch{S}")
    m.close()


def _forest_sizes(S):
    return ([BIG, 7, 8, 64, 65, 7169, 65537, 9, 14, 15, 56, 57, 112, 113, 1023, 1024, 1025, 7168] + [2_000 + 337 * k for k in range(S)])[:S]


@pytest.mark.parametrize("S", [32, 40])
def test_forest_batches(S):
    """from 32 scans on: kd_forest_build, one workgroup per scan; one 150 000-point scan among small ones"""
    sizes = _forest_sizes(S)
    m = handle(S)
    via_batch(m, [subset(n, seed=7 + k) for k, n in enumerate(sizes)], normals_for={0, 1, 2, 3, 4, 5, 6, S - 1} if S == 32 else {1, 5, S - 1},
              label=f"forest{S}", batched_upload=S == 32)
    m.close()


def test_forest_twice_gives_the_same_bits():
    """leaf slots come from atomicAdd: the emit order must not depend on them"""
    S = 32
    sizes = [20_000 + 1_250 * k for k in range(S)]
    m = handle(max(S, 2), ns=max(sizes))
    clouds = [subset(n, seed=11 + k) for k, n in enumerate(sizes)]
    m.set_input_sources_batch(clouds, list(range(S)))
    runs = []
    for _ in range(2):
        Ms = m.prepare_targets_from_sources(list(range(S)), list(range(S)))
        runs.append([m.get_target(int(Ms[k]), slot=k) for k in range(S)])
    for k in range(S):
        assert np.array_equal(runs[0][k][0].view(np.uint32), runs[1][k][0].view(np.uint32))
        assert np.array_equal(runs[0][k][1].view(np.uint32), runs[1][k][1].view(np.uint32))
    for k in (0, 17, 31):
        check(f"forest repeat [{k}]", resident(m, clouds[k], k), runs[1][k], normals=k == 17)
    m.close()


def test_one_handle_through_large_small_forest_small():
    """workspaces are sized at creation and reused: counts, node_at and the forest's status must not leak between calls"""
    S = 32
    m = handle(S)
    p_dev, t = via_source(m, subset(BIG))
    check("stale: 150000", p_dev, t, normals=False)
    p_dev, t = via_source(m, subset(9))
    check("stale: 9 after 150000", p_dev, t)
    p_dev, t = via_raw(m, subset(9, seed=4))
    check("stale: raw 9", p_dev, t)
    sizes = _forest_sizes(S)
    via_batch(m, [subset(n, seed=13 + k) for k, n in enumerate(sizes)], normals_for={1, 2, 5}, label="stale: forest32")
    p_dev, t = via_source(m, subset(9))
    check("stale: 9 after the forest", p_dev, t)
    via_batch(m, [subset(n, seed=17 + k) for k, n in enumerate([9, 1025])], normals_for={0, 1}, label="stale: batch2 after the forest")
    m.close()


# ---- ties and degenerate leaves -----------------------------------------------------------------------------------------------
def tied_clouds():
    rng = np.random.default_rng(23)
    out = {}
    q = subset(20_000, seed=29).copy()
    q[:, :3] = (np.round(q[:, :3] / F(0.02)) * F(0.02)).astype(F)
    out["quantised 2 cm"] = q
    g = np.arange(16, dtype=F) * F(0.25) + F(1.0)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    lat = np.concatenate([lat[rng.permutation(len(lat))], np.zeros((len(lat), 1), F)], axis=1).astype(F)
    out["lattice 16^3"] = lat
    d = subset(20_000, seed=31).copy()
    d = np.concatenate([d, np.repeat(d[:1], 4096, axis=0)])
    out["4096 duplicates"] = np.ascontiguousarray(d[rng.permutation(len(d))])
    z = np.zeros((20_000, 4), F)
    z[:, :2] = rng.uniform(-2, 2, (20_000, 2)).astype(F)
    z[:, 2] = rng.uniform(-3, 3, 20_000).astype(F)
    z[: 10_000, 2] = np.where(rng.random(10_000) < 0.5, F(-0.0), F(0.0))
    out["signed zeros"] = np.ascontiguousarray(z[rng.permutation(len(z))])
    s = np.zeros((20_000, 4), F)
    s[:, :3] = rng.uniform(-1, 1, (20_000, 3)).astype(F)
    tiny = (rng.integers(-200, 200, 8_000).astype(np.float64) * 1.4e-45 * rng.integers(1, 3000, 8_000)).astype(F)   # float32 denormals
    s[: 8_000, 0] = tiny
    s[:, 1] += F(3.0)                                              # (no leaf plane through the origin by accident)
    out["denormals across 0"] = np.ascontiguousarray(s[rng.permutation(len(s))])
    return out


@pytest.mark.parametrize("name", ["quantised 2 cm", "lattice 16^3", "4096 duplicates", "signed zeros", "denormals across 0"])
def test_ties_raw_from_source_and_forest(name):
    """every rule about points ON a median: smallest index goes left, -0.0 before +0.0, argmax stays at the first widest side;
    long tie runs go through sort_indices' heap sort; leaves of duplicates are rank 0 and dropped"""
    c = tied_clouds()[name]
    S = 32
    m = handle(S, ns=len(c) + 64, nt=len(c) + 64)
    p_dev, t = via_raw(m, c)
    check(f"{name}: raw", p_dev, t)
    p_dev, t = via_source(m, c)
    check(f"{name}: from_source", p_dev, t)
    rng = np.random.default_rng(37)
    clouds = [c] + [np.ascontiguousarray(c[rng.permutation(len(c))[: len(c) - 97 * k]]) for k in range(1, S)]
    m.set_input_sources_batch(clouds, list(range(S)))
    Ms = m.prepare_targets_from_sources(list(range(S)), list(range(S)))
    for k in (0, 9, 31):
        check(f"{name}: forest[{k}]", resident(m, clouds[k], k), m.get_target(int(Ms[k]), slot=k), normals=k == 0)
    m.close()


def drop_cloud():
    """a scan with rings at z exactly 0 (leaves coplanar with the origin: det(M) == 0) and axis-parallel line segments on
    exactly representable coordinates (leaves of rank 1) mixed in"""
    rng = np.random.default_rng(41)
    base = subset(20_000, seed=43)
    th = rng.uniform(0, 2 * np.pi, 6_000)
    r = np.repeat(np.array([6.0, 9.0, 12.0]), 2_000)
    ring = np.stack([r * np.cos(th), r * np.sin(th), np.zeros_like(th), np.zeros_like(th)], axis=1).astype(F)
    seg = []
    for k in range(60):
        a = np.zeros((100, 4), F)
        axis = k % 3
        a[:, :3] = np.array([20 + k * 0.5, -15 + k * 0.25, 1 + k * 0.125], F)
        a[:, axis] += np.arange(100, dtype=F) / F(64)
        seg.append(a)
    c = np.concatenate([base, ring] + seg)
    return np.ascontiguousarray(c[rng.permutation(len(c))])


def test_dropped_leaves_rank_one_and_singular():
    c = drop_cloud()
    m = handle(2, ns=len(c), nt=len(c))
    for go in (via_raw, via_source, via_target):
        p_dev, t = go(m, c)
        R = reference(p_dev, True)
        L = R.leaves
        singular = sum(1 for k in np.flatnonzero(R.decision == nr.DROP) if (p_dev[L[k], 2] == 0).all() and len(np.unique(p_dev[L[k], :2], axis=0)) > 2)
        rank1 = sum(1 for k in np.flatnonzero(R.decision == nr.DROP) if (np.ptp(p_dev[L[k]], axis=0) == 0).sum() == 2)
        print("dropped: singular", singular, "rank one", rank1)
        assert singular > 100 and rank1 > 100
        check(f"drops: {go.__name__}", p_dev, t)
    m.close()
