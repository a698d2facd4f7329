"""pclomp's direct neighbourhoods on the CPU (tests/ndt_direct_ref.py): how the three stencils and KDTREE's pair set contain one
another on the constructed cases of ndt_deriv_ref, the min_points and box rules on a hand-built target, the floats at which the
division's cell is not the multiplication's, the oracle's whole alignment in each mode, the tolerance factor measured for the
direct pair sets, and the option's place in the C header and the ctypes binding."""
import math
import os
import re

import numpy as np
import pytest

import ndt_deriv_ref as R
import ndt_direct_ref as D
from oracle import ndt as ondt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D1, D2 = R.gauss_constants_f32_options()


def _set(pairs):
    return set(zip(pairs[0].tolist(), pairs[1].tolist()))


def test_stencils():
    assert len(D.stencil(D.DIRECT1)) == 1 and len(D.stencil(D.DIRECT7)) == 7 and len(D.stencil(D.DIRECT26)) == 26
    s26 = set(D.stencil(D.DIRECT26))
    assert (0, 0, 0) not in s26 and all((-a, -b, -c) in s26 for a, b, c in s26)           # 13 half-neighbours and their negatives
    assert set(D.stencil(D.DIRECT7)) - s26 == {(0, 0, 0)}


@pytest.mark.parametrize("name", R.case_names())
def test_pair_sets_contain_one_another(name):
    c = R.case(name)
    t = R.tables()[c.target]
    xt = R.case_xt(c)
    p1, p7, p26 = (_set(D.direct_pairs(t, xt, m)) for m in (D.DIRECT1, D.DIRECT7, D.DIRECT26))
    kd = R.find_pairs(t, xt)
    assert p1 <= p7
    assert p7 <= p26 | p1
    assert _set(kd[:2]) <= p26 | p1                          # a centroid within one resolution lies in one of the 27 cells
    assert not (p26 & p1)
    for m, p in ((D.DIRECT1, p1), (D.DIRECT7, p7), (D.DIRECT26, p26)):
        pairs = D.direct_pairs(t, xt, m)
        assert len(p) == len(pairs[0]) == D.brute_force_count(t, xt, m), (name, m)
        assert (np.diff(pairs[0]) >= 0).all()                # by point
    bad = np.nonzero(~R.finite_rows(c.src))[0]
    assert not any(i in bad for i, _ in p26 | p1)            # a row that is not finite has no pairs


def test_min_points_and_the_box_on_three_voxels():
    """Voxels (0, 0, 0), (1, 0, 0), (2, 0, 0) with 5, 6 and 7 points: the box is 3 x 1 x 1 cells."""
    rng = np.random.default_rng(7)
    tgt = np.concatenate([R._voxel_points(rng, (x, 0, 0), n) for x, n in ((0, 5), (1, 6), (2, 7))])
    t = R.build_table(np.concatenate([tgt, np.zeros((len(tgt), 1))], axis=1).astype(np.float32))
    assert t.n.tolist() == [5, 6, 7] and t.div_b.tolist() == [3, 1, 1]
    grid = ondt.VoxelGrid(tgt.astype(np.float32))
    q = np.array([[0.5, 0.5, 0.5],       # 0: in the 5-point voxel
                  [1.5, 0.5, 0.5],       # 1: in the 6-point voxel
                  [3.5, 0.5, 0.5],       # 2: one cell outside in x, next to the 7-point voxel
                  [4.5, 0.5, 0.5],       # 3: two cells outside
                  [2.5, 1.5, 0.5],       # 4: one cell outside in y, above the 7-point voxel
                  [2.5, 1.5, 1.5],       # 5: one cell outside in y and z: an edge neighbour of the 7-point voxel
                  [2.5, 2.5, 0.5]], dtype=np.float32)
    for table in (t, grid):
        five = 0 if table is t else None                     # the table lists the 5-point voxel (slot 0); the oracle grid does not hold it
        slot = {1: 1, 2: 2} if table is t else {1: 0, 2: 1}
        p1, p7, p26 = (_set(D.direct_pairs(table, q, m)) for m in (D.DIRECT1, D.DIRECT7, D.DIRECT26))
        if five is not None:
            assert not any(v == five for _, v in p1 | p7 | p26)                            # 5 points: no pair in any mode
        assert p1 == {(1, slot[1])}                                                         # query 0's own voxel has 5 points
        assert p7 == {(0, slot[1]), (1, slot[1]), (1, slot[2]), (2, slot[2]), (4, slot[2])}
        assert p26 == {(0, slot[1]), (1, slot[2]), (2, slot[2]), (4, slot[2]), (4, slot[1]), (5, slot[2]), (5, slot[1])}
        for p in (p1, p7, p26):
            assert not any(i in (3, 6) for i, _ in p)        # two cells outside: none
        assert any(i == 2 for i, _ in p7) and any(i == 2 for i, _ in p26) and not any(i == 2 for i, _ in p1)


def test_division_and_multiplication_disagree_at_resolution_03():
    x, cd, cm = D.disagreeing_floats()
    print(f"{len(x)} of 2400 floats have floor(x / 0.3f) != floor(x * (1 / 0.3f))")
    assert len(x) >= 8
    assert (np.abs(cd - cm) == 1).all()
    c = D.division_case()
    assert len(c["src"]) >= 8 and c["expect_div"].sum() >= 4 and c["expect_mul"].sum() >= 4
    grid = ondt.VoxelGrid(c["target"], resolution=D.LEAF_03)
    pi, _ = D.direct_pairs(grid, c["xt"], D.DIRECT1, D.LEAF_03)
    assert sorted(pi.tolist()) == np.nonzero(c["expect_div"])[0].tolist()
    # the build puts every target point where both rules put it, and both cells of every query are occupied
    tp = c["target"][:, :3]
    lf = np.float32(D.LEAF_03)
    assert (np.floor(tp / lf) == np.floor(tp * (np.float32(1) / lf))).all()
    occ = set(map(tuple, np.floor(tp / lf).astype(int).tolist()))
    cy = np.floor(c["xt"][:, 1] / lf).astype(int); cz = np.floor(c["xt"][:, 2] / lf).astype(int)
    assert all((a, y, z) in occ and (b, y, z) in occ for a, b, y, z in zip(c["cd"], c["cm"], cy, cz))


@pytest.mark.parametrize("mode", D.DIRECT_MODES)
def test_oracle_alignment_in_a_direct_mode_ends_before_the_cap(mode):
    r = D.oracle_align(mode)
    print(f"{D.MODE_NAMES[mode]}: {r['iterations']} iterations, {r['derivative_calls']} derivative calls")
    assert 0 < r["iterations"] < 35 and np.isfinite(r["result"]).all()
    src, _, _, T = D.golden_pair()
    assert abs(r["result"][0, 3] - T[0, 3]) < 0.25           # moved towards the truth from 0.25 m short


def test_batch_guesses_take_different_numbers_of_iterations():
    its = [D.oracle_align(D.DIRECT7, k)["iterations"] for k in range(len(D.BATCH_OFFSETS))]
    print("DIRECT7 iterations of the batch guesses:", its)
    assert len(set(its)) > 1


def test_measured_rho_of_the_direct_pair_sets():
    """ndt_deriv_ref's tolerance rule measured on the direct pair sets: rho = the largest |oracle - reference| / S_c over the
    cases, modes, arithmetics and Hessian settings, the oracle being oracle.ndt.compute_derivatives on the same pairs.  The
    RHO committed in ndt_direct_ref must bound it, and that module's K -- the GPU test's -- follows from it by ndt_deriv_ref's rule."""
    worst = (0.0, None)
    grids = {name: {m: D.DirectVoxelGrid(R.target(name), m) for m in D.DIRECT_MODES} for name in ("block", "strip", "mixed")}
    for c in R.cases():
        ok = R.finite_rows(c.src)
        src, xt = c.src[ok], R.case_xt(c)[ok]
        for m in D.DIRECT_MODES:
            for dm in (False, True):
                ref = D.case_reference(c.name, D1, D2, dm, True, m)
                s, g, H, n = ondt.compute_derivatives(grids[c.target][m], src, xt, c.pose, D1, D2, True, real=np.float64 if dm else None)
                assert n == ref.pairs, (c.name, m, n, ref.pairs)
                r, k = R.worst_ratio(np.concatenate([[s], g, np.asarray(H, dtype=np.float64).reshape(-1)]), ref)
                if r > worst[0]:
                    worst = (r, (c.name, D.MODE_NAMES[m], dm, k))
    print(f"rho over the direct pair sets = {worst[0]:.4f} at {worst[1]}; committed RHO = {D.RHO}; K = {2.0 ** math.ceil(math.log2(4 * max(1.0, worst[0])))}")
    assert worst[0] <= D.RHO
    assert D.K == 2.0 ** math.ceil(math.log2(4 * max(1.0, D.RHO)))


def test_option_in_the_header_and_the_binding():
    import ctypes
    from staticmapping_amd import _capi
    assert _capi.NdtOptions.search_method.offset == 28 and ctypes.sizeof(_capi.NdtOptions) == 48
    assert _capi.NdtOptions.search_method.size == 4
    h = open(os.path.join(ROOT, "include", "smhip.h")).read()
    got = dict(re.findall(r"#define\s+SMHIP_NDT_SEARCH_(\w+)\s+(\d+)", h))
    assert got == {"KDTREE": "0", "DIRECT26": "1", "DIRECT7": "2", "DIRECT1": "3"}           # pclomp/ndt_omp.h:52-57
    assert (_capi.NDT_SEARCH_KDTREE, _capi.NDT_SEARCH_DIRECT26, _capi.NDT_SEARCH_DIRECT7, _capi.NDT_SEARCH_DIRECT1) == (0, 1, 2, 3)
    assert (D.KDTREE, D.DIRECT26, D.DIRECT7, D.DIRECT1) == (0, 1, 2, 3)
    body = h[h.index("typedef struct smhip_ndt_options"):h.index("} smhip_ndt_options;")]
    assert re.search(r"int32_t\s+search_method;", body) and re.search(r"int32_t\s+reserved\[4\];", body)
