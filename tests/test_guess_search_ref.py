"""tests/guess_search_ref.py, the definition the device guess search is tested against, checked on its own: constructed clouds whose
scores are known, the tie rule key by key, the floor rule on voxel borders, the sample rule, and the experiment of DESIGN.md §6
("Guess search") with the CPU oracle's ICP started from the drifted and from the searched guess."""
import numpy as np
import pytest

import guess_search_cases as cases
import guess_search_ref as ref
from oracle import icp_pointmatcher as opm

ROT90 = np.array([[0.0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
WINDOW = dict(half_xy=4, half_z=1, yaw_steps=1, yaw_step=float(np.radians(10.0)))


def seen_from(target, guess, shift_voxels, res=0.5):
    """the source that `guess` followed by a shift of whole voxels puts exactly on the target (lattice clouds: exact in float32)"""
    s = target.copy()
    p = target[:, :3].astype(np.float64) - res * np.asarray(shift_voxels, np.float64)
    s[:, :3] = (p - guess[:3, 3]) @ guess[:3, :3]                  # R^T (p - t)
    return s


@pytest.mark.parametrize("guess", [np.eye(4), ROT90], ids=["0deg", "90deg"])
@pytest.mark.parametrize("shift", [(0, 0, 0), (3, -2, 1), (-4, 4, -1)])
def test_lattice_clouds_score_n_at_the_true_candidate_only(guess, shift):
    target = cases.lattice(150, seed=3)
    r = ref.search(target, seen_from(target, guess, shift), guess, **WINDOW)
    assert r["best"] == (0,) + shift and r["best_score"] == 150
    assert (r["volume"] == 150).sum() == 1                         # the unique maximum
    assert r["guess_score"] == r["volume"][1, 1, 4, 4] and r["n_candidates"] == 3 * 3 * 81 and r["n_source_used"] == 150
    want = guess.copy()
    want[:3, 3] += 0.5 * np.array(shift)
    assert np.array_equal(r["transform"], want)
    if shift == (0, 0, 0):
        assert r["guess_score"] == 150


def test_whole_volume_equals_the_definition_word_for_word():
    rng = np.random.default_rng(5)
    target = np.zeros((60, 4), np.float32)
    target[:, :3] = rng.uniform(-2, 2, (60, 3))
    source = np.zeros((40, 5), np.float32)
    source[:, :3] = rng.uniform(-2.5, 2.5, (40, 3))
    guess = np.eye(4)
    guess[:3, 3] = (0.3, -0.2, 0.1)
    o = dict(half_xy=2, half_z=1, yaw_steps=1, resolution=0.3, yaw_step=0.2)
    r = ref.search(target, source, guess, **o)
    for a in (-1, 0, 1):
        for k in (-1, 0, 1):
            for j in range(-2, 3):
                for i in range(-2, 3):
                    assert r["volume"][a + 1, k + 1, j + 2, i + 2] == ref.score_brute(target, source, guess, a, i, j, k, **o)


def test_two_copies_tie_and_the_nearer_one_wins():
    shape = cases.lattice(40, seed=7, span=3)
    far = shape.copy()
    far[:, 0] -= 4 * 0.5 * 5                                       # a second copy 20 voxels along -x
    target = np.concatenate([shape, far])
    for near, other in (((1, 0, 0), (-19, 0, 0)), ((-2, 1, 0), (-22, 1, 0))):
        source = seen_from(shape, np.eye(4), near)
        r = ref.search(target, source, np.eye(4), half_xy=22, half_z=0, yaw_steps=0)
        v = r["volume"][0, 0]
        assert v[near[1] + 22, near[0] + 22] == 40 == v[other[1] + 22, other[0] + 22] and (v == 40).sum() == 2
        assert r["best"] == (0,) + near and r["runner_up_score"] == 40


def test_each_later_key_of_the_pick_rule():
    def volume(cells):
        v = np.zeros((5, 3, 7, 7), np.int32)
        for a, i, j, k in cells:
            v[a + 2, k + 1, j + 3, i + 3] = 5
        return v
    pick = lambda cells: ref.pick(volume(cells), 3, 1, 2)[0]
    assert ref.pick(np.zeros((5, 3, 7, 7), np.int32), 3, 1, 2) == ((0, 0, 0, 0), 0, 0)          # all equal: the guess
    assert pick([(1, 2, -1, 0), (-1, -3, 3, 1)]) == (1, 2, -1, 0)                               # the smaller i^2 + j^2 + k^2
    assert pick([(1, 2, -1, 0), (2, 1, 2, 0)]) == (1, 2, -1, 0)                                 # then the smaller |a|
    assert pick([(1, 2, -1, 0), (-1, 1, 2, 0)]) == (-1, 1, 2, 0)                                # then the smaller a
    assert pick([(-1, 1, 2, 0), (-1, 0, 2, -1)]) == (-1, 0, 2, -1)                              # then the smaller k
    assert pick([(-1, 0, 2, -1), (-1, 2, 0, -1)]) == (-1, 2, 0, -1)                             # then the smaller j
    assert pick([(-1, 2, 0, -1), (-1, -2, 0, -1)]) == (-1, -2, 0, -1)                           # then the smaller i
    v = volume([(0, 0, 0, 0)]) * 2
    for cell, s in (((0, 2, -2, 1), 8), ((1, -2, 2, -1), 7), ((-1, 1, 1, 1), 6)):               # within 2 voxels and 1 yaw step: not apart
        v[cell[0] + 2, cell[3] + 1, cell[2] + 3, cell[1] + 3] = s
    assert ref.pick(v, 3, 1, 2) == ((0, 0, 0, 0), 10, 0)
    v[2, 1, 3, 6] = 4                                                                           # i = 3
    assert ref.pick(v, 3, 1, 2)[2] == 4
    v[4, 1, 3, 3] = 9                                                                           # a = 2
    assert ref.pick(v, 3, 1, 2)[2] == 9


def test_floor_rule_on_voxel_borders():
    f = np.float32
    assert ref.voxels(np.array([[-0.5, 0.5, -0.0]], f), 0.5).tolist() == [[-1, 1, 0]]
    assert ref.voxels(np.array([[-1.0, -1.0000001, 0.99999994]], f), 0.5).tolist() == [[-2, -3, 1]]
    # 0.3 is not a float: 0.6f / 0.3f is exactly 2, 0.9f / 0.3f rounds to 2.9999998 (the real quotient is 3), (0.3f * 3) / 0.3f is 3
    assert ref.voxels(np.array([[0.6, -0.6, 0.9]], f), 0.3).tolist() == [[2, -2, 2]]
    assert ref.voxels(np.array([[f(0.3) * f(3), -0.9, -0.3]], f), 0.3).tolist() == [[3, -3, -1]]
    rng = np.random.default_rng(11)
    k = rng.integers(-4000, 4000, (5000, 3))
    for res in (0.3, 0.5, 0.1):
        p = (k * f(res)).astype(f)                                     # on or within an ulp of a border
        p = np.concatenate([p, np.nextafter(p, f(np.inf)), np.nextafter(p, f(-np.inf))])
        want = np.floor((p.astype(np.float64) / np.float64(f(res))).astype(f))      # the double quotient of two floats rounds once more to the float one
        assert np.array_equal(ref.voxels(p, res), want.astype(np.int64))
    with pytest.raises(ref.Refused) as e:
        ref.voxels(np.array([[6.0e8, 0, 0]], f), 0.5)
    assert e.value.status == "capacity"
    assert ref.voxels(np.array([[5.3e8, 0, 0]], f), 0.5)[0, 0] < ref.MAX_VOXEL


@pytest.mark.parametrize("M", [5, 64])
def test_sample_rule(M):
    for n in (M - 1, M, M + 1, 2 * M - 1, 3 * M + 1):
        rows = ref.sample_rows(n, M)
        assert rows.tolist() == (list(range(n)) if n <= M else [(k * n) // M for k in range(M)])
        assert len(set(rows.tolist())) == len(rows)
        target = cases.lattice(50, seed=13)
        source = np.repeat(seen_from(target, np.eye(4), (1, 1, 0)), 4, axis=0)[:n]
        source[1::2, 0] = np.nan                                       # the rule counts the rows that are left
        kept = ref.finite_rows(source)
        by_hand = np.zeros((len(ref.sample_rows(len(kept), M)), 4), np.float32)
        by_hand[:, :3] = kept[ref.sample_rows(len(kept), M)]
        a = ref.search(target, source, np.eye(4), max_source_points=M, **WINDOW)
        b = ref.search(target, by_hand, np.eye(4), max_source_points=10 * M, **WINDOW)
        assert a["n_source_used"] == len(by_hand) == min(M, len(kept)) and np.array_equal(a["volume"], b["volume"])
    assert ref.sample_rows(2**31 - 1, 4096)[-1] == (4095 * (2**31 - 1)) // 4096


def test_refusals_of_the_restatement():
    t, s = cases.lattice(10, 1), cases.lattice(10, 2)
    bad = [("invalid", dict(resolution=0.0)), ("invalid", dict(resolution=float("nan"))), ("invalid", dict(half_xy=-1)), ("invalid", dict(half_z=-1)),
           ("invalid", dict(yaw_steps=-1)), ("invalid", dict(max_source_points=0)), ("invalid", dict(yaw_step=float("inf"))),
           ("capacity", dict(half_xy=2896, half_z=0, yaw_steps=0)), ("capacity", dict(half_z=(1 << 19) + 1, half_xy=0, yaw_steps=0)), ("capacity", dict(max_points=9))]
    for status, o in bad:
        with pytest.raises(ref.Refused) as e:
            ref.search(t, s, np.eye(4), **o)
        assert e.value.status == status, o
    nan = np.full((4, 4), np.nan, np.float32)
    for a, b, g in ((nan, s, np.eye(4)), (t, nan, np.eye(4)), (t, s, np.full((4, 4), np.inf)), (t[:0], s, np.eye(4)), (t[:, :3], s, np.eye(4))):
        with pytest.raises(ref.Refused) as e:
            ref.search(a, b, g, **WINDOW)
        assert e.value.status == "invalid"
    assert ref.check(10, 10, dict(ref.DEFAULTS, half_xy=2895, half_z=0, yaw_steps=0), np.eye(4), max_points=10) == (5791, 1, 1)


@pytest.fixture(scope="module")
def experiment_search():
    target, source, truth, guess = cases.experiment()
    return ref.search(target, source, guess)


def test_experiment_pick_is_within_one_voxel_and_one_yaw_step_of_the_truth(experiment_search):
    _, _, truth, guess = cases.experiment()
    r = experiment_search
    print("pick", r["best"], "score", r["best_score"], "at the guess", r["guess_score"], "runner-up", r["runner_up_score"])
    assert np.abs(r["transform"][:3, 3] - truth[:3, 3]).max() <= 0.5
    yaw = lambda T: np.degrees(np.arctan2(T[1, 0], T[0, 0]))
    assert abs(yaw(r["transform"]) - yaw(truth)) <= 2.0 + 1e-9
    assert r["best_score"] > 2 * r["guess_score"] and r["n_source_used"] == 4096 and r["n_candidates"] == 176505


def test_oracle_icp_fails_from_the_drifted_guess_and_lands_from_the_searched_one(experiment_search):
    target, source, truth, guess = cases.experiment()
    keep = np.ones(len(ref.finite_rows(source)), bool)
    out = {}
    for name, start in (("drifted", guess), ("searched", experiment_search["transform"])):
        accepted, result, score, iterations = opm.align(source, target, start, keep, use_c=True)
        out[name] = (np.linalg.norm(result[:3, 3] - truth[:3, 3]), np.abs(result[:3, :3] - truth[:3, :3]).max())
        print(name, "accepted", accepted, "score %.3f" % score, "iterations", iterations, "translation error %.3f m" % out[name][0], "rotation entries %.5f" % out[name][1])
        assert score > 0.75                                            # CloseLoop would take either edge
    assert out["drifted"][0] > 1.0                                     # measured 1.169 m
    assert out["searched"][0] < 0.1 and out["searched"][1] < 0.01      # measured 0.005 m
