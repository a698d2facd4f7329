"""What the graph of a join shows under the factors of the reference's multi-trajectory optimiser, on tests/multi_trajectory_ref.py
(numpy, no device): the findings DESIGN.md section 6, "Joining maps", builds on.  The graph is 8 + 8 submaps 4 m apart, the incremental
map loaded 0.5 m on x and on y and 0.5 degrees off, cross edges to incremental submaps 3 and up with 1 cm of noise.

Everything is measured on the mutual pose base_k^-1 incremental_k: with both priors equally strong the base map moves as much as the
incremental one (1.6 m here), so only the mutual position of the two maps is observable."""
import numpy as np
import pytest

import multi_trajectory_ref as mt
import pose_graph_ref as ref

NB = NI = 8
WITH_EDGE = range(3, NI)
# The wrong cross edge (3 m, 0.2 rad) is the one to incremental submap 6: an interior one, with a good edge on either side of it.
WRONG = 6


@pytest.fixture(scope="module")
def clean():
    case = mt.join_case(NB, NI)
    free = mt.optimize(mt.assemble(case), solver="pcg")
    held = mt.optimize(mt.assemble(case, hold_base=True), solver="pcg")
    return case, free, held


def test_the_factor_list_is_the_builders():
    case = mt.join_case(NB, NI)
    g = mt.assemble(case)
    # 7 base connections, 5 loop constraints, 7 incremental connections, 2 priors
    assert len(g["kinds"]) == 21 and list(g["kinds"][:19]) == [0] * 19 and list(g["kinds"][19:]) == [1, 1]
    assert [tuple(x) for x in g["ij"][:7]] == [(k, k + 1) for k in range(7)]
    assert [tuple(x) for x in g["ij"][7:12]] == [(s, 8 + s) for s in WITH_EDGE] and g["loops"] == list(range(7, 12))
    assert [tuple(x) for x in g["ij"][12:19]] == [(8 + k, 9 + k) for k in range(7)]
    assert [tuple(x) for x in g["ij"][19:]] == [(0, 0), (8, 8)]
    assert (g["huber"][g["loops"]] == 1.0).all() and g["huber"].sum() == 5.0
    assert (g["sigmas"][7:12] == 0.025).all() and (g["sigmas"][:7] == 0.01).all() and (g["sigmas"][19:] == 0.1).all()
    held = mt.assemble(case, hold_base=True)
    assert len(held["kinds"]) == 20 and tuple(held["ij"][-1]) == (8, 8) and list(held["fixed"]) == [1] * 8 + [0] * 8
    # a connection is target^-1 source of the loaded poses: no residual at the start, so the whole initial cost is the loop constraints'
    r, _, _, _ = mt.robust.linearize(g, g["poses"])
    assert np.abs(np.delete(r, g["loops"], axis=0)).max() < 1e-12 and np.abs(r[g["loops"]]).max() > 1.0


def test_base_free_only_the_mutual_pose_at_submaps_with_loop_edges_is_recovered(clean):
    case, (poses, st), _ = clean
    start = [mt.mutual_error(case, mt.loaded(case), s) for s in range(NI)]
    end = [mt.mutual_error(case, poses, s) for s in range(NI)]
    print("stop", st["stop"], "steps", st["accepted"], st["rejected"], "pcg", st["pcg_iterations"], "start", np.round(start, 3), "end", np.round(end, 4))
    assert st["stop"] == ref.STOP_COST and st["rejected"] == 0 and 8 <= st["accepted"] <= 11
    assert abs(start[0] - np.hypot(0.5, 0.5)) < 0.01
    assert all(end[s] < 0.05 * start[s] for s in WITH_EDGE)
    assert end[0] > 0.2 * start[0]                                        # before the first loop edge the submaps stay bent toward their loaded pose
    moved = np.linalg.norm(poses[:NB, :3, 3] - case["base"][:, :3, 3], axis=1).max()
    assert moved > 0.5                                                    # the base map itself moves: its prior is no stronger than the other


def test_base_held_keeps_the_base_bits_and_needs_one_cg_iteration_per_step(clean):
    case, (free, st_free), (poses, st) = clean
    end = [mt.mutual_error(case, poses, s) for s in range(NI)]
    start = [mt.mutual_error(case, mt.loaded(case), s) for s in range(NI)]
    print("stop", st["stop"], "steps", st["accepted"], "pcg", st["pcg_iterations"], "against", st_free["pcg_iterations"], "with the base free; end", np.round(end, 4))
    assert st["stop"] == ref.STOP_COST
    assert poses[:NB].tobytes() == case["base"].tobytes()
    assert st["pcg_max"] == 1 and st["pcg_iterations"] == st["accepted"] and st_free["pcg_max"] > 10
    assert all(end[s] < 0.05 * start[s] for s in WITH_EDGE)


def test_one_wrong_cross_edge_needs_the_huber_threshold(clean):
    case, (want, _), _ = clean
    bad = mt.join_case(NB, NI, wrong=WRONG)
    assert all(np.array_equal(a[2], b[2]) == (a[1] != WRONG) for a, b in zip(case["cross"], bad["cross"]))     # the other edges are the clean ones

    def off(poses):
        return max(float(np.linalg.norm(mt.mutual(bad, poses, s)[:3, 3] - mt.mutual(case, want, s)[:3, 3])) for s in WITH_EDGE)
    robust, st_r = mt.optimize(mt.assemble(bad, loop_huber=1.0))
    plain, st_p = mt.optimize(mt.assemble(bad, loop_huber=0.0))
    print("with Huber(1): %.4f m from the clean result, stop %d; without: %.3f m, stop %d" % (off(robust), st_r["stop"], off(plain), st_p["stop"]))
    assert st_r["stop"] == ref.STOP_COST and off(robust) < 0.02
    assert off(plain) > 1.0
    w = mt.robust.report(mt.assemble(bad, loop_huber=1.0), robust)[1]
    at = mt.assemble(bad)["loops"]
    assert [w[k] < 0.1 for k in at] == [s == WRONG for s in WITH_EDGE] and (np.delete(w, at[WRONG - 3]) == 1.0).all()
