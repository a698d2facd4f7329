"""Conditions of the fitness-search cases (tests/ndt_fitness_cases.py), checked without a GPU: every lattice case lies on the 2^-6 m
lattice inside the box and under its size caps, the float32 restatement of the device's arithmetic equals the integer brute force
bit for bit (the exactness argument of ndt_fitness_ref.py, shown rather than claimed), and every construction holds what its
description says."""
import itertools

import numpy as np
import pytest

import ndt_fitness_cases as C
import ndt_fitness_ref as R


@pytest.mark.parametrize("name", C.case_names())
def test_case_lies_on_the_lattice_inside_the_box_and_under_its_caps(name):
    c = C.case(name)
    tgt, src, fin = c.target(), c.source(), c.finite_rows()
    assert tgt.dtype == np.float32 and src.dtype == np.float32 and tgt.shape[1] == 4 and src.shape[1] == 4
    assert 1 <= len(tgt) <= C.MAX_TARGET and 1 <= len(src) <= C.MAX_SOURCE
    assert fin.sum() == len(c.query_u) and np.isfinite(tgt).all() and np.isfinite(src[fin]).all()
    assert not np.isfinite(src[~fin, :3]).all(axis=1).any()
    moved = src[fin, :3].astype(np.float64) + np.asarray(c.trans_u) * R.UNIT
    for a in (tgt[:, :3].astype(np.float64), src[fin, :3].astype(np.float64), moved):
        u = a / R.UNIT
        assert (u == np.round(u)).all() and u.min() >= -R.BOX and u.max() < R.BOX
    assert (moved / R.UNIT == c.query_u).all()
    assert (c.pose()[:3, :3] == np.eye(3)).all() and (c.pose()[:3, 3] / R.UNIT == np.asarray(c.trans_u)).all()
    assert len(np.unique(c.target_u, axis=0)) == len(c.target_u)            # no point twice: a designed neighbour is one point


@pytest.mark.parametrize("name", C.case_names())
def test_float32_brute_force_equals_the_integer_one(name):
    c = C.case(name)
    want = R.lattice_expected_d2(C.reference(name)[0])
    got = R.float32_brute_force(c.source()[c.finite_rows()], c.target(), (np.asarray(c.trans_u) * R.UNIT).astype(np.float32))
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    assert C.reference(name)[0].max() < 1 << 22


@pytest.mark.parametrize("name", [n for n in C.case_names() if C.case(n).designed is not None])
def test_the_designed_neighbour_is_the_brute_force_neighbour(name):
    c = C.case(name)
    best = C.reference(name)[0]
    has = c.designed >= 0
    d = c.query_u[has] - c.target_u[c.designed[has]]
    assert ((d * d).sum(axis=1) == best[has]).all()


def _fine(u):
    return np.floor_divide(u, R.FINE)


def test_corner_construction():
    c = C.case("corner")
    best, cube = C.reference("corner")
    kind = np.array(c.notes["kind"])
    assert (kind == "corner").sum() == 24 and (best[kind == "corner"] == 25).all() and (cube[kind == "corner"] == 147).all()
    for k in np.nonzero(kind == "corner")[0]:
        q, out = c.query_u[k], c.target_u[c.designed[k]]
        inside = c.target_u[c.designed[k] - 1]
        assert (np.abs(_fine(inside) - _fine(q)) == 1).all()                 # the diagonal neighbour of the query's fine cell
        assert (np.abs(inside - q) == 7).all()                               # ... at its far corner
        assert np.abs(_fine(out) - _fine(q)).max() == 2 and np.abs(out - q).sum() == 5      # one fine cell + one unit along an axis
    octants = {tuple(np.sign(c.target_u[c.designed[k] - 1] - c.query_u[k])) for k in np.nonzero(kind == "corner")[0]}
    assert len(octants) == 8
    assert (kind == "bound16").sum() == 15 and (best[kind == "bound16"] == 16).all() and (cube[kind == "bound16"] == 16).all()
    assert (kind == "bound14").sum() == 12 and (best[kind == "bound14"] == 14).all() and (cube[kind == "bound14"] == 14).all()
    assert not any(a * a + b * b + e * e == 15 for a, b, e in itertools.product(range(4), repeat=3))
    settled = R.settles_in_the_fine_cube(cube)
    assert settled[kind == "bound14"].all() and not settled[kind != "bound14"].any()


def _sort_key(t):
    """The order the table keeps a target's points in at leaf 1.0: voxel (z, y, x), mid cell, fine cell, caller index."""
    v = np.floor_divide(t, R.VOX); f = np.floor_divide(t, R.FINE) % 16
    mid = ((f[:, 2] >> 2) * 4 + (f[:, 1] >> 2)) * 4 + (f[:, 0] >> 2)
    fin = ((f[:, 2] & 3) * 4 + (f[:, 1] & 3)) * 4 + (f[:, 0] & 3)
    return np.lexsort((np.arange(len(t)), fin, mid, v[:, 0], v[:, 1], v[:, 2])), mid, fin


def test_runs_construction():
    c = C.case("runs")
    t = c.target_u
    best, cube = C.reference("runs")
    cells, counts = np.unique(_fine(t), axis=0, return_counts=True)
    count_of = {tuple(k): n for k, n in zip(cells.tolist(), counts.tolist())}
    assert sorted(c.notes["cells"].values()) == [1, 2, 3, 4, 5, 7, 8, 9, 9]
    order, mid, fin = _sort_key(t)
    rank = np.empty(len(t), int); rank[order] = np.arange(len(t))
    for base, n in c.notes["cells"].items():
        key = tuple(_fine(np.array(base)).tolist())
        assert count_of[key] == n
        members = np.nonzero((_fine(t) == np.array(key)).all(axis=1))[0]
        last = members[np.argmax(rank[members])]
        assert (t[last] == np.array(base) + [3, 1, 1]).all()                 # the run's last point is the designed neighbour
        qs = np.nonzero(c.designed == last)[0]
        assert sorted(best[qs].tolist()) == [4, 36] and sorted(cube[qs].tolist()) == [-1, 4]      # one for the cube, one for the shells
        m = (np.floor_divide(t, R.MID) == np.floor_divide(np.array(base), R.MID)).all(axis=1)
        assert m.sum() == n                                                  # alone in its mid cell: the shells' run is this run
    assert (t[order[-1]] == np.array(c.notes["last"]) + [3, 1, 1]).all()     # j1 == nt
    assert (_fine(t[order[-9:]]) == _fine(np.array(c.notes["last"]))).all()

    def occupancy(base):
        m = (np.floor_divide(t, R.MID) == np.floor_divide(np.array(base), R.MID)).all(axis=1)
        return sorted(fin[m].tolist())
    assert occupancy(c.notes["full"]) == list(range(64))
    assert occupancy(c.notes["only0"]) == [0] and occupancy(c.notes["only63"]) == [63]
    near_full = (np.floor_divide(c.query_u, R.MID) == 0).all(axis=1)
    f = _fine(c.query_u[near_full]) % 4
    assert len({tuple(x) for x in f.tolist()}) == 64 and (f == 3).all(axis=1).any()          # a query in every fine cell, (3, 3, 3) too


def test_probing_crowded_outside_and_far_constructions():
    c = C.case("probing")
    assert len(np.unique(np.floor_divide(c.target_u, R.MID), axis=0)) == len(c.target_u) == 4096
    assert len(c.query_u) == 4 * 256
    c = C.case("crowded")
    vox, n = np.unique(np.floor_divide(c.target_u, R.VOX), axis=0, return_counts=True)
    assert len(vox) == 27 and sorted(n.tolist()) == [3] * 26 + [C.BIG_VOXEL + 1]
    inside = (np.floor_divide(c.query_u, R.VOX) == 0).all(axis=1)
    assert 10 < inside.sum() < len(inside) - 10
    c = C.case("outside")
    t, q = c.target_u, c.query_u
    assert t.min(axis=0).tolist() == [-128] * 3 and t.max(axis=0).tolist() == [127] * 3      # the box is [-128, 128)^3 at leaf 1.0
    beyond = np.maximum(np.maximum(-128 - q, q - 128), 0).max(axis=1)
    assert set(np.ceil(beyond / 64).astype(int).tolist()) == {1, 2, 5} and len(q) == 92
    for a in range(3):
        assert (q[:, a] <= -192).any() and (q[:, a] >= 192).any()
    assert (C.reference("outside")[0] >= 64 * 64).all()
    for n in C.FAR_VOXELS:
        c = C.case(f"far/v{n}")
        assert len(np.unique(np.floor_divide(c.target_u, R.VOX), axis=0)) == len(c.target_u) == n
        assert len(c.query_u) == 64 and (C.reference(c.name)[0] > 96 * 96).all()
    # far/bound at leaf 1.0: the smallest farthest-corner distance over the voxels' boxes is not the nearest point's voxel's
    c = C.case("far/bound")
    lo = np.floor_divide(c.target_u, R.VOX) * R.VOX
    q = c.query_u[0]
    farthest = np.sqrt((np.maximum(np.abs(q - lo), np.abs(q - lo - R.VOX)) ** 2).sum(axis=1))
    d = np.sqrt(((c.target_u - q) ** 2).sum(axis=1))
    assert np.argmin(farthest) == 1 and np.argmin(d) == 0 == c.designed[0] and d[0] < d[1] < farthest[1] < farthest[0]


def test_sizes_and_nonfinite_constructions():
    assert [len(C.case(f"sizes/n{n}").query_u) for n in C.SIZES] == list(C.SIZES) == [1, 63, 64, 65, 255, 256, 257, 1025]
    for n in C.SIZES[1:]:
        s = R.settles_in_the_fine_cube(C.reference(f"sizes/n{n}")[1])
        assert s.any() and not s.all()                                       # both kinds in every scan of the open flags
    best, cube = C.reference("sizes/all_open")
    assert len(best) == 256 and (best == 192).all() and not R.settles_in_the_fine_cube(cube).any()
    best, cube = C.reference("sizes/none_open")
    assert len(best) == 256 and (best <= 1).all() and R.settles_in_the_fine_cube(cube).all()
    c = C.case("sizes/lane255")
    best, cube = C.reference("sizes/lane255")
    opened = ~R.settles_in_the_fine_cube(cube)
    assert len(best) == 256 and opened.sum() == 1 and (best[~opened] <= 1).all()
    k = int(np.nonzero(opened)[0][0])
    assert (np.delete(c.query_u, k, axis=0) < c.query_u[k]).all()            # the largest on every axis: last in a Morton order
    c, twin = C.case("nonfinite"), C.case("sizes/n65")
    src = c.source()
    assert len(src) == 67 and (~c.finite_rows()).tolist() == [i in (7, 40) for i in range(67)]
    assert np.isnan(src[7, 0]) and np.isinf(src[40, 1])
    assert src[c.finite_rows()].tobytes() == twin.source().tobytes() and c.target().tobytes() == twin.target().tobytes()


def test_scan_reference_against_brute_force_and_its_tolerance_terms():
    rng = np.random.default_rng(9)
    src = rng.normal(0, 20, size=(300, 3)).astype(np.float32)
    tgt = rng.normal(0, 20, size=(2000, 3)).astype(np.float32)
    ang = 0.5
    G = np.eye(4); G[:2, :2] = [[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]; G[:3, 3] = (3.0, -2.0, 0.5)
    d, tol = R.scan_reference(src, tgt, G)
    Gf = G.astype(np.float32).astype(np.float64)
    moved = src.astype(np.float64) @ Gf[:3, :3].T + Gf[:3, 3]
    brute = np.sqrt(((moved[:, None, :] - tgt.astype(np.float64)[None, :, :]) ** 2).sum(axis=2).min(axis=1))
    assert np.allclose(d, brute, rtol=1e-14, atol=0)
    # the float path of the device restated: inside the derived tolerance with room to spare
    moved32 = ((Gf[:3, :3].astype(np.float32)[None] * src[:, None, :]).sum(axis=2, dtype=np.float32) + Gf[:3, 3].astype(np.float32))
    d32 = moved32[:, None, :] - tgt[None, :, :]
    d2_32 = (d32 * d32).sum(axis=2, dtype=np.float32).min(axis=1)
    ratio = np.abs(d2_32.astype(np.float64) - d * d) / tol
    print(f"float32 restatement: worst |d2 - d^2| / tolerance = {ratio.max():.3f}")
    assert (ratio <= 1).all() and (tol > 0).all()
    # 1e7 m away: the float coordinate's spacing is 1 m and E must cover it
    G[:3, 3] = (1.0e7, 0, 0)
    d, tol = R.scan_reference(src, tgt, G)
    assert (tol >= 2 * d * 1.0).all()


def test_stage_rules():
    res = float(np.float32(0.3))
    marg = 1e-5
    d = np.array([res / 16, res / 16 * 1.001, 0.875 * res, 0.876 * res, 0.74 * res, 0.76 * res])
    assert R.stage_violations([0, 0, 1, 1, 2, 2], d, 0.3, marg).tolist() == [1, 3, 4]
    assert R.stage_violations([-1, 3], [0.0, 0.0], 1.0, marg).tolist() == [0, 1]
    assert R.score_of(np.array([1.0, np.inf, 3.0], np.float32)) == 2.0 and R.score_of(np.array([np.inf], np.float32)) == R.NO_SCORE
    t = R.to_f32([[-128, 0, 0], [127, 5, 5]])
    assert abs(R.table_margin(t, 1.0) - 4 * 2.0 ** -24 * 4.0) < 1e-12
