"""registrators::Ndt on constructed inputs (tests/ndt_deriv_ref.py): the voxel table bit for bit where it has one value, and single
computeDerivatives evaluations -- float and double arithmetic, Hessian on and off -- against the float64 reference, pair counts
exactly and every component inside K S_c (K and S_c: see ndt_deriv_ref.py; K is measured on the CPU, never here).

The cases reach what scans do not: a wave's second window of list entries (under, at, one over and well over the cap), sources
of 1 .. 1025 points (fewer than a granule, one and two waves, more than a workgroup), queries one and two voxels outside the
box and at both ends of every occupancy word, points on lattice planes, non-finite source rows, voxels at the min_points and
the stats / stats_big boundaries, degenerate voxels, and a box that the bit grid refuses.

Every test prints its worst |device - reference| / S_c; DESIGN.md section 8 records the figures of an MI355X run.
"""
import numpy as np
import pytest

import ndt_deriv_ref as R
from oracle import ndt as ondt

pytestmark = pytest.mark.gpu

D1, D2 = R.gauss_constants_f32_options()         # the handle's options are floats (smhip_ndt_options)
WORST = {}


@pytest.fixture(scope="module")
def handles():
    """One matcher per constructed target, its table built."""
    import staticmapping_amd as sm
    made = {}

    def get(target):
        if target not in made:
            m = sm.NdtHip(max_source_points=2048, max_target_points=16384)
            m.set_input_target(R.target(target))
            m.build_voxels()
            made[target] = m
        return made[target]
    yield get
    for m in made.values():
        m.close()


def _table_bits(m):
    n = m.build_voxels()
    return n, m.get_voxels(n)


def _check_table(m, t):
    n, (keys, counts, means, icov, cent) = _table_bits(m)
    assert n == len(t.key) and keys.tolist() == t.key.tolist()              # every occupied voxel, in slot order
    assert counts.tolist() == t.n.tolist()                                   # (none fails the eigenvalue check: no -1)
    assert cent.tobytes() == t.centroid.tobytes()
    assert means.tobytes() == t.mean.tobytes()
    ref6 = np.stack([t.icov[:, 0, 0], t.icov[:, 0, 1], t.icov[:, 0, 2], t.icov[:, 1, 1], t.icov[:, 1, 2], t.icov[:, 2, 2]], axis=1)
    s = t.searchable()
    assert (icov[~s] == 0).all()
    ulp = 2.0 ** -23 * np.abs(ref6).max(axis=1, keepdims=True)               # the raw sums are exact: only the last rounding may differ
    err = np.abs(icov.astype(np.float64) - ref6)
    print(f"icov: worst error {np.max(err[s] / ulp[s]):.3f} ulp of the voxel's largest entry")
    assert (err[s] <= ulp[s]).all()
    return keys, counts, means, icov, cent


@pytest.mark.parametrize("target", ["block", "strip", "mixed"])
def test_voxel_table_bit_for_bit(target, handles):
    t = R.tables()[target]
    keys, counts, _, icov, _ = _check_table(handles(target), t)
    if target == "mixed":
        by_vox = {tuple((i + t.min_b).tolist()): k for k, i in enumerate(t.idx)}
        assert counts[by_vox[(0, 0, 0)]] == 5 and (icov[by_vox[(0, 0, 0)]] == 0).all()          # not searchable
        assert counts[by_vox[(3, 0, 0)]] == 6 and (icov[by_vox[(3, 0, 0)]] != 0).any()
        assert sorted(counts[counts > 1000].tolist()) == [R.BIG_VOXEL, R.BIG_VOXEL + 1, 4000]   # both sides of the stats / stats_big split


def test_target_rows_that_are_not_finite_are_refused_whole():
    """oracle.ndt.VoxelGrid passes over rows that are not finite; the C ABI does not let them in: smhip_set_target_f32 refuses the
    cloud (the handle's targets also feed searches that cannot take them) and leaves the slot without a target.  The same rows
    without the four bad ones then give the table's usual bits."""
    import staticmapping_amd as sm
    m = sm.NdtHip(max_source_points=2048, max_target_points=16384)
    bad = R.with_nonfinite_rows(R.target("mixed"))
    assert (~R.finite_rows(bad)).sum() == 4
    with pytest.raises(sm.SmhipError) as e:
        m.set_input_target(bad)
    assert e.value.status == 1 and "NaN / Inf" in str(e.value)
    m.set_input_target(bad[R.finite_rows(bad)])
    _check_table(m, R.tables()["mixed"])
    m.close()


def _evaluate(m, c, dm, h):
    s, g, H, pairs = m.compute_derivatives_ex(c.pose, h, dm)
    return np.concatenate([[s], g, H.reshape(-1)]), pairs


@pytest.mark.parametrize("name", R.case_names())
def test_one_evaluation(name, handles):
    c = R.case(name)
    m = handles(c.target)
    m.set_input_source(c.src)
    failures = []
    for dm in (False, True):
        for h in (True, False):
            ref = R.case_reference(c, D1, D2, dm, h)
            got, pairs = _evaluate(m, c, dm, h)
            again, pairs2 = _evaluate(m, c, dm, h)
            r, k = R.worst_ratio(got, ref)
            key = ("double" if dm else "float", "on" if h else "off")
            WORST[key] = max(WORST.get(key, 0.0), r)
            print(f"{name} {key[0]} hessian {key[1]}: pairs {pairs} (reference {ref.pairs}), worst |dev - ref| / S = {r:.4f} at component {k}")
            if pairs != ref.pairs:
                failures.append((key, "pairs", pairs, ref.pairs))
            if not r <= R.K:
                failures.append((key, "component", k, r, got[k], ref.full()[k], ref.full_scale()[k]))
            if not h and not (got[7:] == 0).all():
                failures.append((key, "Hessian returned with compute_hessian = 0"))
            if got.tobytes() != again.tobytes() or pairs != pairs2:
                failures.append((key, "a repeated evaluation differs"))
    assert not failures, failures


def test_worst_ratios_of_this_run():
    """A print-only summary for the record in DESIGN.md: the worst ratio per arithmetic and Hessian setting over whichever cases of
    test_one_evaluation ran before it in this process (none, if it runs alone).  It asserts nothing: every case asserts its own."""
    for key, r in sorted(WORST.items()):
        print(f"worst |dev - ref| / S, {key[0]} arithmetic, Hessian {key[1]}: {r:.4f}")


def test_a_second_handle_gives_the_same_bits(handles):
    import staticmapping_amd as sm
    for name in ("block/one_over_1025/Pb", "block/interior_256/Pa", "block/ns1025/Pc", "block/ns1/Pa"):
        c = R.case(name)
        m1 = handles("block")
        m2 = sm.NdtHip(max_source_points=2048, max_target_points=16384)
        m2.set_input_target(R.target("block")); m2.build_voxels()
        m1.set_input_source(c.src); m2.set_input_source(c.src)
        for dm in (False, True):
            for h in (True, False):
                a, pa = _evaluate(m1, c, dm, h)
                b, pb = _evaluate(m2, c, dm, h)
                assert a.tobytes() == b.tobytes() and pa == pb, (name, dm, h)
        m2.close()


def _pose_matrix(pose):
    return R.pose_matrix_f32(pose).astype(np.float64)


def test_align_on_the_all_interior_case_matches_the_oracle():
    import staticmapping_amd as sm
    c = R.case("block/interior_256/Pa")
    tgt = R.target("block")
    G = _pose_matrix(c.pose)
    m = sm.NdtHip(max_source_points=2048, max_target_points=16384)
    m.set_input_source(c.src); m.set_input_target(tgt)
    ok, T = m.align(G)
    ref = ondt.ndt_align(c.src, tgt, guess=G)
    st = m.last_ndt_stats
    print(f"iterations {st['iterations']} / {ref['iterations']}, derivative calls {st['derivative_calls']} / {ref['derivative_calls']}")
    assert st["iterations"] == ref["iterations"] and st["derivative_calls"] == ref["derivative_calls"]
    da, dt = sm.se3_error(T, ref["result"])
    assert da < 1e-4 and dt < 1e-3, (da, dt)                       # test_ndt_align_parity's tolerances
    m.close()


def test_batch_of_tiny_and_full_size_pairs_equals_the_single_calls_bit_for_bit():
    """align_batch over slots of 1, 65 and 257 source points (block) and one 30 k-point scan against a 90 k-point submap: the
    workgroups per evaluation follow the largest source, and every pair must still return its single call's bits."""
    import staticmapping_amd as sm
    from staticmapping_amd import synth
    scene = synth.make_scene(0)
    poses = [synth.make_pose(t=(0.8 * k, 0.02 * k, 0.0), rpy_deg=(0, 0, 0.5 * k)) for k in range(4)]
    scans = [synth.velodyne_scan(scene, P, seed=10 + k, n_points=30000) for k, P in enumerate(poses)]
    tgt = np.concatenate([s[:, :3].astype(np.float64) @ P[:3, :3].T + P[:3, 3] for s, P in zip(scans[:3], poses[:3])])
    tgt = np.concatenate([tgt, np.zeros((len(tgt), 1))], axis=1).astype(np.float32)
    G = poses[3].copy(); G[0, 3] -= 0.3
    pairs = [(R.case(f"block/ns{ns}/Pa").src, R.target("block"), _pose_matrix(R.POSES["Pa"])) for ns in (1, 65, 257)]
    pairs.insert(2, (scans[3], tgt, G))
    single = []
    m1 = sm.NdtHip(max_source_points=len(scans[3]), max_target_points=len(tgt))
    for s, t, g in pairs:
        m1.set_input_source(s); m1.set_input_target(t)
        ok, T = m1.align(g)
        single.append((T, m1.get_fitness_score(), dict(m1.last_ndt_stats)))
    m1.close()
    mb = sm.NdtHip(max_source_points=len(scans[3]), max_target_points=len(tgt), pair_slots=4)
    for k, (s, t, g) in enumerate(pairs):
        mb.set_input_source(s, slot=k); mb.set_input_target(t, slot=k)
    for rep in range(2):                                           # second pass: the tables are kept
        T, sc, st = mb.align_batch(4, [p[2] for p in pairs])
        for k in range(4):
            assert T[k].tobytes() == single[k][0].tobytes(), (rep, k)
            assert (sc[k] == single[k][1] or (np.isnan(sc[k]) and np.isnan(single[k][1]))) and st[k] == single[k][2], (rep, k, st[k], single[k][2])
    mb.close()


def test_a_box_beyond_the_bit_grid_is_refused_and_the_handle_goes_on(handles):
    """Two 8-point clusters 400 m apart on every axis: 13 x 401 x 401 words, twice what the bit grid holds.  build_voxels and align
    answer SMHIP_ERR_CAPACITY, and the next target on the same handle gives the usual bits."""
    import staticmapping_amd as sm
    far = R.target("far")
    assert R.build_table(far).words > R.MAX_WORDS
    c = R.case("block/interior_64/Pa")
    m = sm.NdtHip(max_source_points=2048, max_target_points=16384)
    m.set_input_source(c.src); m.set_input_target(far)
    with pytest.raises(sm.SmhipError) as e:
        m.build_voxels()
    assert e.value.status == 7 and "exceeds the bit grid" in str(e.value)
    with pytest.raises(sm.SmhipError) as e:
        m.align(_pose_matrix(c.pose))
    assert e.value.status == 7 and "exceeds the bit grid" in str(e.value)
    m.set_input_target(R.target("block"))
    _check_table(m, R.tables()["block"])
    ref = handles("block")
    ref.set_input_source(c.src)
    for dm in (False, True):
        a, pa = _evaluate(m, c, dm, True)
        b, pb = _evaluate(ref, c, dm, True)
        assert a.tobytes() == b.tobytes() and pa == pb == R.case_reference(c, D1, D2, dm, True).pairs
    m.close()
