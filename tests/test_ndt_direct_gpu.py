"""registrators::Ndt under pclomp's direct neighbourhoods (smhip_ndt_options.search_method = DIRECT26 / DIRECT7 / DIRECT1) against
tests/ndt_direct_ref.py: single evaluations on the constructed inputs of ndt_deriv_ref (pair counts exactly, every component
inside K S_c with ndt_direct_ref.K, measured on the CPU), the centre cell by division at resolution 0.3, whole alignments against
the oracle in the same mode, a DIRECT7 batch against its single calls, the voxel table kept across a change of mode, and the
values smhip_ndt_set_options refuses."""
import numpy as np
import pytest

import ndt_deriv_ref as R
import ndt_direct_ref as D
from oracle import ndt as ondt

pytestmark = pytest.mark.gpu

D1, D2 = R.gauss_constants_f32_options()


@pytest.fixture(scope="module")
def handles():
    """One matcher per constructed target, its table built (the table does not depend on the mode)."""
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


def _evaluate(m, pose, dm, h):
    s, g, H, pairs = m.compute_derivatives_ex(pose, h, dm)
    return np.concatenate([[s], g, H.reshape(-1)]), pairs


@pytest.mark.parametrize("name", R.case_names())
def test_one_evaluation_in_every_direct_mode(name, handles):
    c = R.case(name)
    m = handles(c.target)
    m.set_input_source(c.src)
    failures = []
    for mode in D.DIRECT_MODES:
        m.set_ndt_options(search_method=mode)
        for dm in (False, True):
            for h in (True, False):
                ref = D.case_reference(name, D1, D2, dm, h, mode)
                got, pairs = _evaluate(m, c.pose, dm, h)
                again, pairs2 = _evaluate(m, c.pose, dm, h)
                r, k = R.worst_ratio(got, ref)
                key = (D.MODE_NAMES[mode], "double" if dm else "float", "on" if h else "off")
                print(f"{name} {key[0]} {key[1]} hessian {key[2]}: pairs {pairs} (reference {ref.pairs}), worst |dev - ref| / S = {r:.4f} at component {k}")
                if pairs != ref.pairs:
                    failures.append((key, "pairs", pairs, ref.pairs))
                if not r <= D.K:
                    failures.append((key, "component", k, r, got[k], ref.full()[k], ref.full_scale()[k]))
                if not h and not (got[7:] == 0).all():
                    failures.append((key, "Hessian returned with compute_hessian = 0"))
                if got.tobytes() != again.tobytes() or pairs != pairs2:
                    failures.append((key, "a repeated evaluation differs"))
    m.set_ndt_options(search_method=D.KDTREE)
    assert not failures, failures


def test_the_centre_cell_is_taken_by_division():
    """Resolution 0.3: queries at floats where floor(x / 0.3f) is not floor(x * (1 / 0.3f)), both cells occupied, one of them below
    min_points (ndt_direct_ref.division_case).  DIRECT1 pairs a query exactly when the DIVISION's cell is the searchable one: the
    even queries.  A kernel that keeps the build's tx * inv pairs the odd ones instead."""
    import staticmapping_amd as sm
    c = D.division_case()
    d1, d2 = R.gauss_constants_f32_options(resolution=D.LEAF_03)
    grid = ondt.VoxelGrid(c["target"], resolution=D.LEAF_03)
    m = sm.NdtHip(max_source_points=2048, max_target_points=16384, resolution=D.LEAF_03, search_method=D.DIRECT1)
    m.set_input_target(c["target"])
    m.build_voxels()
    m.set_input_source(c["src"])
    ref = D.reference(grid, c["src"], c["xt"], c["pose"], d1, d2, False, True, D.DIRECT1, D.LEAF_03)
    got, pairs = _evaluate(m, c["pose"], False, True)
    r, k = R.worst_ratio(got, ref)
    print(f"all {len(c['src'])} queries: pairs {pairs} (division {int(c['expect_div'].sum())}, multiplication {int(c['expect_mul'].sum())}), worst ratio {r:.4f} at {k}")
    assert pairs == ref.pairs == int(c["expect_div"].sum())
    assert r <= D.K
    # the pair SET: every query alone
    paired = []
    for j in range(len(c["src"])):
        m.set_input_source(c["src"][j:j + 1])
        paired.append(_evaluate(m, c["pose"], False, False)[1])
    assert paired == c["expect_div"].astype(int).tolist(), paired
    assert paired != c["expect_mul"].astype(int).tolist()
    m.close()


@pytest.fixture(scope="module")
def aligned():
    """The golden-size pair aligned on the device in all four modes, each on a fresh handle."""
    import staticmapping_amd as sm
    src, tgt, G, _ = D.golden_pair()
    out = {}
    for mode in (D.KDTREE,) + D.DIRECT_MODES:
        m = sm.NdtHip(max_source_points=len(src), max_target_points=len(tgt), search_method=mode)
        m.set_input_source(src); m.set_input_target(tgt)
        ok, T = m.align(G)
        out[mode] = (T, m.get_fitness_score(), dict(m.last_ndt_stats))
        m.close()
    return out


@pytest.mark.parametrize("mode", D.DIRECT_MODES)
def test_whole_alignment_matches_the_oracle_in_the_same_mode(mode, aligned):
    import staticmapping_amd as sm
    T, fit, st = aligned[mode]
    ref = D.oracle_align(mode)
    print(f"{D.MODE_NAMES[mode]}: iterations {st['iterations']} / {ref['iterations']}, derivative calls {st['derivative_calls']} / {ref['derivative_calls']}, "
          f"pairs of the last evaluation {st['pairs_last']:.0f}")
    assert st["iterations"] == ref["iterations"] and st["derivative_calls"] == ref["derivative_calls"]
    da, dt = sm.se3_error(T, ref["result"])
    assert da < 1e-4 and dt < 1e-3, (da, dt)                                  # tests/test_ndt_gpu.py's tolerances
    assert abs(fit - ref["score"]) <= 1e-3 * ref["score"]
    assert abs(st["trans_probability"] - ref["trans_probability"]) <= 1e-4 * abs(ref["trans_probability"])


def test_the_four_modes_give_four_results(aligned):
    modes = (D.KDTREE,) + D.DIRECT_MODES
    for i, a in enumerate(modes):
        for b in modes[i + 1:]:
            assert aligned[a][0].tobytes() != aligned[b][0].tobytes(), (a, b)
            assert aligned[a][2]["pairs_last"] != aligned[b][2]["pairs_last"], (a, b)
    src = D.golden_pair()[0]
    assert aligned[D.DIRECT1][2]["pairs_last"] <= len(src)                   # at most one voxel a point


def test_direct7_batch_equals_the_single_calls_bit_for_bit():
    import staticmapping_amd as sm
    src, tgt, _, _ = D.golden_pair()
    guesses = D.batch_guesses()
    single = []
    m1 = sm.NdtHip(max_source_points=len(src), max_target_points=len(tgt), search_method=D.DIRECT7)
    m1.set_input_source(src); m1.set_input_target(tgt)
    for g in guesses:
        ok, T = m1.align(g)
        single.append((T, m1.get_fitness_score(), dict(m1.last_ndt_stats)))
    m1.close()
    its = [s[2]["iterations"] for s in single]
    assert its == [D.oracle_align(D.DIRECT7, k)["iterations"] for k in range(4)] and len(set(its)) > 1
    mb = sm.NdtHip(max_source_points=len(src), max_target_points=len(tgt), pair_slots=4, search_method=D.DIRECT7)
    for k in range(4):
        mb.set_input_source(src, slot=k); mb.set_input_target(tgt, slot=k)
    for rep in range(2):                                                      # second pass: the tables are kept
        T, sc, st = mb.align_batch(4, guesses)
        for k in range(4):
            assert T[k].tobytes() == single[k][0].tobytes(), (rep, k)
            assert sc[k] == single[k][1] and st[k] == single[k][2], (rep, k, st[k], single[k][2])
    mb.close()


def test_the_kept_table_serves_a_change_of_mode(aligned):
    import staticmapping_amd as sm
    src, tgt, G, _ = D.golden_pair()
    m = sm.NdtHip(max_source_points=len(src), max_target_points=len(tgt))
    m.set_target_cache(True)
    m.set_input_source(src); m.set_input_target(tgt)
    for mode in (D.KDTREE, D.DIRECT7, D.KDTREE):
        m.set_ndt_options(search_method=mode)
        ok, T = m.align(G)
        want = aligned[mode]
        assert T.tobytes() == want[0].tobytes() and m.get_fitness_score() == want[1] and m.last_ndt_stats == want[2], mode
    m.close()


def test_other_values_are_refused_and_change_nothing(aligned):
    import staticmapping_amd as sm
    src, tgt, G, _ = D.golden_pair()
    m = sm.NdtHip(max_source_points=len(src), max_target_points=len(tgt), search_method=D.DIRECT7)
    m.set_input_source(src); m.set_input_target(tgt)
    for bad in (-1, 4):
        with pytest.raises(sm.SmhipError) as e:
            m.set_ndt_options(search_method=bad)
        assert e.value.status == 1 and "bad NDT options" in str(e.value)
    ok, T = m.align(G)
    assert T.tobytes() == aligned[D.DIRECT7][0].tobytes() and m.last_ndt_stats == aligned[D.DIRECT7][2]
    m.close()
