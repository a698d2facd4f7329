"""The constructed NDT cases of tests/ndt_deriv_ref.py on the CPU: their conditions (lattice exactness, list-entry totals, margins,
which voxels are searchable), the measured tolerance factor against oracle/ndt.py, and six deliberately wrong kernels that the
bound must reject."""
import ctypes
import ctypes.util
import functools
import math

import numpy as np
import pytest

import ndt_deriv_ref as R
from oracle import ndt as ondt

D1, D2 = R.gauss_constants_f32_options()


@functools.lru_cache(maxsize=None)
def _ref(name, double_math, hessian):
    case = {c.name: c for c in R.cases()}[name]
    return R.case_reference(case, D1, D2, double_math, hessian)


@functools.lru_cache(maxsize=None)
def _oracle_grid(name):
    return ondt.VoxelGrid(R.target(name))


def _oracle(case, double_math, hessian):
    ok = R.finite_rows(case.src)
    src, xt = case.src[ok], R.case_xt(case)[ok]
    s, g, H, n = ondt.compute_derivatives(_oracle_grid(case.target), src, xt, case.pose, D1, D2, hessian,
                                          real=np.float64 if double_math else None)
    return np.concatenate([[s], g, np.asarray(H, dtype=np.float64).reshape(-1)]), n


def test_targets_are_exact_lattices_and_the_tables_are_the_oracles():
    for name in ("block", "strip", "mixed", "far"):
        assert R.check_lattice(R.target(name))
    tb = R.tables()
    assert len(tb["block"].key) == 216 and (tb["block"].n == 8).all() and len(R.target("block")) == 1728
    assert len(tb["strip"].key) == 720 and len(R.target("strip")) == 5760
    assert tb["strip"].min_b[0] == -40 and (tb["strip"].div_b[0] + 31) // 32 == 3          # a row spans three words, min_b < 0
    m = tb["mixed"]
    got = {tuple((i + m.min_b).tolist()): int(n) for i, n in zip(m.idx, m.n)}
    assert got == R.MIXED_VOXELS
    assert sorted(n for n in got.values() if n > 1000) == [R.BIG_VOXEL, R.BIG_VOXEL + 1, 4000]
    assert len(R.target("mixed")) < 10000
    assert R.build_table(R.target("far")).words > R.MAX_WORDS
    for name in ("block", "strip", "mixed"):
        t, o = tb[name], _oracle_grid(name)
        s = t.searchable()
        assert t.key[s].tolist() == o.key.tolist() and o.occupied == len(t.key)
        assert t.centroid[s].tobytes() == o.centroid.tobytes() and t.mean[s].tobytes() == o.mean.tobytes()
        assert t.valid[s].all() and o.valid.all()
        assert np.allclose(t.icov[s], o.icov, rtol=0, atol=1e-12 * np.abs(o.icov).max())
    # the thin crowded voxel goes through the eigenvalue inflation (:346-356): its icov has the 1 / (0.01 w_max) ceiling
    # -- before the inflation its smallest covariance eigenvalue is below 0.01 of the largest (no other voxel's is), after it the
    # ratio is the 0.01 exactly, to rounding
    k = [tuple((i + m.min_b).tolist()) for i in m.idx].index((3, 3, 0))
    s = m.searchable()
    below = m.eig[:, 0] < R.EIG_MULT * m.eig[:, 2]
    assert below[k] and below[s].sum() == 1 and not (m.eig[k, 1] < R.EIG_MULT * m.eig[k, 2])
    w = np.linalg.eigvalsh(m.icov[k])
    assert abs(w[2] / w[0] * R.EIG_MULT - 1.0) < 1e-9 and abs(1.0 / w[0] - m.eig[k, 2]) < 1e-9 * m.eig[k, 2]
    for name in ("block", "strip"):
        t = tb[name]
        assert not (t.eig[:, 0] < R.EIG_MULT * t.eig[:, 2]).any()
    # rows that are not finite are no points of the grid (:209-213)
    o2 = ondt.VoxelGrid(R.with_nonfinite_rows(R.target("mixed")))
    o1 = _oracle_grid("mixed")
    assert (~R.finite_rows(R.with_nonfinite_rows(R.target("mixed")))).sum() == 4
    assert o2.key.tolist() == o1.key.tolist() and o2.mean.tobytes() == o1.mean.tobytes() and o2.icov.tobytes() == o1.icov.tobytes()


def test_the_float_pose_matrix_has_one_value():
    """The cases lean on R.pose_matrix_f32 being what a float implementation without fused multiply-adds gives: the float cosines
    and sines of the poses' angles are the correctly rounded ones in numpy and in the C library (cosf / sinf, which the device's
    host code calls), and the oracle's matrix -- the same products through numpy's matmul -- is within an ulp of it."""
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    for f in (libm.cosf, libm.sinf):
        f.restype = ctypes.c_float; f.argtypes = [ctypes.c_float]
    for p in R.POSES.values():
        for a in p[3:]:
            a32 = np.float32(a)
            assert np.cos(a32) == np.float32(math.cos(float(a32))) == np.float32(libm.cosf(float(a32)))
            assert np.sin(a32) == np.float32(math.sin(float(a32))) == np.float32(libm.sinf(float(a32)))
        T, To = R.pose_matrix_f32(p), ondt.pose_to_matrix_f32(np.asarray(p))
        assert T.dtype == np.float32 and (np.abs(T.astype(np.float64) - To.astype(np.float64)) <= np.spacing(np.abs(To))).all()
    assert R.pose_matrix_f32(R.POSES["Pi"]).tobytes() == ondt.pose_to_matrix_f32(np.asarray(R.POSES["Pi"])).tobytes()


def test_cases_meet_their_conditions():
    tb = R.tables()
    names = [c.name for c in R.cases()]
    assert len(set(names)) == len(names)
    for ns in R.SIZES:
        assert f"block/ns{ns}/Pa" in names
    for c in R.cases():
        t = tb[c.target]
        xt = R.case_xt(c)
        pi, vi, gap = R.find_pairs(t, xt)
        assert gap > R.MARGIN, c.name
        assert R.plane_gap(xt, c.on_plane) > R.MARGIN, c.name
        ent = R.list_entries(t, xt)
        if c.entries is not None:
            assert len(c.src) == 64 and ent.sum() == c.entries, (c.name, ent.sum())
        if "interior" in c.name:
            # every query lists all 27: any 64 of them, whichever the device's point order gives a wave, list 1728 entries
            assert (ent == 27).all() and len(c.src) % 64 == 0 and 64 * int(ent.min()) == 1728 > R.PAIR_CAP
        if c.target == "strip":
            bad = ~R.finite_rows(c.src)
            assert bad.sum() == 3 and np.isnan(c.src[bad][:, :3]).all(axis=1).sum() == 2
            assert not np.isin(np.nonzero(bad)[0], pi).any()
            cell = np.floor(xt.astype(np.float64)) - t.min_b
            fin = ~bad
            for ix in (0, 31, 32, 33, 63, 64, 79):
                assert ((cell[fin, 0] == ix) & (cell[fin, 1:] >= 0).all(axis=1) & (cell[fin, 1:] <= 2).all(axis=1)).any(), (c.name, ix)
            for a in range(3):
                for edge, step in ((-1, -1), (t.div_b[a], 1)):
                    one = fin & (cell[:, a] == edge)
                    two = fin & (cell[:, a] == edge + step)
                    assert one.any() and two.any(), (c.name, a, edge)
                    assert np.isin(np.nonzero(one)[0], pi).any(), (c.name, a, edge)          # neighbours inside: must contribute
                    assert ent[one].min() > 0 and ent[two].max() == 0
                    assert not np.isin(np.nonzero(two)[0], pi).any()
            far = fin & (np.abs(xt[:, 0]) > 9000)
            assert far.sum() == 1 and ent[far][0] == 0
            if c.pose_name == "Pi":                           # exact transform: the plane queries sit on their planes
                on = xt[c.on_plane].astype(np.float64)
                assert c.on_plane.sum() == 8 and ((on == np.round(on)).any(axis=1)).all()
                src64 = c.src[fin, :3].astype(np.float64) + np.array(R.POSES["Pi"][:3])
                assert (xt[fin].astype(np.float64) == src64).all()
        if c.target == "mixed":
            vox = {tuple((i + t.min_b).tolist()): k for k, i in enumerate(t.idx)}
            assert vox[(0, 0, 0)] not in vi and t.n[vox[(0, 0, 0)]] == 5               # the 5-point voxel: listed, never paired
            assert ent[np.floor(xt.astype(np.float64)).astype(int).tolist().index([0, 0, 0])] >= 2
            for special in R.MIXED_VOXELS:
                if special != (0, 0, 0):
                    assert vox[special] in vi, (c.name, special)                          # the 6-point voxel among them
    # the window cases: under, at and one over the cap, and the most a wave can list
    assert R.WINDOW_MIX["one_window"][1] <= R.PAIR_CAP == R.WINDOW_MIX["exactly_1024"][1] == R.WINDOW_MIX["one_over_1025"][1] - 1
    assert R.PAIR_CAP < 64 * 27 <= 2 * R.PAIR_CAP


def _combos():
    return [(dm, h) for dm in (False, True) for h in (True, False)]


def test_measured_rho_and_pair_counts():
    """rho = the largest |oracle - reference| / S_c over every case, component, arithmetic and Hessian setting; the stored RHO
    bounds it and K follows from it.  The reference's pair counts are the oracle's."""
    rho = {}
    for c in R.cases():
        for dm, h in _combos():
            ref = _ref(c.name, dm, h)
            got, n = _oracle(c, dm, h)
            assert n == ref.pairs, (c.name, n, ref.pairs)
            assert (ref.e != 0).all()                         # every kept pair's e is in range (:504-505): kept pairs = summed pairs
            r, k = R.worst_ratio(got if h else np.concatenate([got[:7], np.zeros(36)]), ref)
            if r > rho.get((dm, h), (0, None, None))[0]:
                rho[(dm, h)] = (r, c.name, k)
    worst = max(v[0] for v in rho.values())
    for (dm, h), (r, name, k) in sorted(rho.items()):
        print(f"rho {'double' if dm else 'float'} hessian {'on' if h else 'off'}: {r:.4f} at {name} component {k}")
    print(f"rho = {worst:.4f}; K = {2.0 ** math.ceil(math.log2(4 * max(1.0, worst)))}")
    assert worst <= R.RHO
    assert R.K == 2.0 ** math.ceil(math.log2(4 * max(1.0, R.RHO)))


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_wrong_kernels_are_rejected(mutation):
    """Each wrong kernel, applied to a copy of the reference, leaves K S_c on at least one case (or changes the pair count)."""
    tb = R.tables()
    caught = []
    for c in R.cases():
        if c.pose_name == "Pi" or (mutation == "min_points_le" and c.target != "mixed"):
            continue
        for dm in (False, True):
            ref = _ref(c.name, dm, True)
            if mutation == "mirror_not_swapped":
                bad, n = ref.full(swap=False), ref.pairs
            else:
                vals, _, n, _, _ = R.evaluate(tb[c.target], c.src, R.case_xt(c), c.pose, D1, D2, dm, True, mutate=mutation)
                bad = R.full_vector(vals)
            r, _ = R.worst_ratio(bad, ref)
            caught.append((r > R.K, n != ref.pairs))
    by_value = any(v for v, _ in caught)
    by_count = any(p for _, p in caught)
    if mutation in ("min_points_le", "drop_weakest_pair"):
        assert by_count
    assert by_value, mutation
    if mutation not in ("min_points_le",):
        assert sum(v for v, _ in caught) >= len(caught) // 2      # not a fluke of one case
