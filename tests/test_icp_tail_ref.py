"""The multi-precision reference of IcpFast's iteration tail (tests/icp_tail_ref.py) against cases worked by hand, and the two
oracles (oracle/icp_fast.py, oracle/csrc/smref_icp.c) over the decision ladder that the device code answers in
test_icp_tail_cpp.py: the oracles are pinned by the same matrices as the device.  No GPU."""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import icp_tail_cases as cases  # noqa: E402
import icp_tail_ref as ref  # noqa: E402
from oracle import cref  # noqa: E402
from oracle import icp_fast as py_oracle  # noqa: E402

mpf = mp.mpf
TINY = mpf(10) ** -50


def _close(a, b, tol=TINY):
    return abs(mpf(a) - mpf(b)) <= tol


# ---------------------------------------------------------------------------------------------- hand-worked cases
def test_normal_equations_of_two_rows_by_hand():
    # p = (1, 2, 3), q = (1, 2, 2.5), n = z: F = (p x n, n) = (2, -1, 0, 0, 0, 1), r = 0.5
    # p = (0, 1, 0), q = (0.25, 1, 0), n = x: F = (0, 0, -1, 1, 0, 0), r = -0.25
    A, b = ref.normal_equations(ref.M([[1, 2, 3], [0, 1, 0]]), ref.M([[1, 2, 2.5], [0.25, 1, 0]]), ref.M([[0, 0, 1], [1, 0, 0]]))
    want = np.zeros((6, 6))
    for F in ([2, -1, 0, 0, 0, 1], [0, 0, -1, 1, 0, 0]):
        want += np.outer(F, F)
    assert (ref.to_np(A) == want).all()
    assert (ref.to_np(b) == -(0.5 * np.array([2, -1, 0, 0, 0, 1.0]) - 0.25 * np.array([0, 0, -1, 1, 0, 0.0]))).all()


def test_full_pivot_qr_pivots_and_rank_by_hand():
    # diag(3, 0, 5, 1, 0, 2): the pivots come out largest first, the corner is exactly zero after four steps
    piv = ref.fullpiv_qr_pivots(ref.M(np.diag([3.0, 0, 5, 1, 0, 2])))
    assert [float(p) for p in piv] == [5, 3, 2, 1, 0, 0]
    assert ref.qr_rank(ref.M(np.diag([3.0, 0, 5, 1, 0, 2])))[0] == 4
    # [[1, 1], [1, 1]] padded: rank 1, pivot sqrt(2) (the norm of the column (1, 1))
    A = np.zeros((6, 6)); A[:2, :2] = 1
    piv = ref.fullpiv_qr_pivots(ref.M(A))
    assert _close(piv[0], mp.sqrt(2)) and all(p == 0 for p in piv[1:])
    # Eigen's rule on a diagonal: eps * 6 * the largest pivot is the line, and the line itself is NOT above it
    e6 = 6 * 2.0 ** -52
    assert ref.qr_rank(ref.M(np.diag([1.0, 1, 1, 1, 1, e6 * 1.5])))[0] == 6
    assert ref.qr_rank(ref.M(np.diag([1.0, 1, 1, 1, 1, e6])))[0] == 5
    assert ref.qr_rank(ref.M(np.diag([1.0, 1, 1, 1, 1, e6 * 0.75])))[0] == 5
    assert _close(ref.qr_rank(ref.M(np.diag([1.0, 1, 1, 1, 1, e6 * 0.75])))[2], 0.75)


def test_full_and_minimum_norm_solutions_by_hand():
    A = np.diag([2.0, 4, 8, 16, 32, 64])
    x = ref.solve_full(ref.M(A), ref.M([2, 4, 8, 16, 32, 64]))
    assert all(_close(v, 1) for v in x)
    # the plane x + y = 2 in the first two coordinates: the shortest solution is (1, 1)
    B = np.zeros((6, 6)); B[:2, :2] = 1; B[2, 2] = 3
    x, rank = ref.solve_reference(ref.M(B), ref.M([2, 2, 6, 0, 0, 0]))
    assert rank == 2 and _close(x[0], 1) and _close(x[1], 1) and _close(x[2], 2) and all(_close(v, 0) for v in x[3:])
    assert ref.eig_gap(ref.M(B), 2) > mpf(10) ** 50                   # (the dropped eigenvalues are zero to the working precision)
    assert _close(ref.eig_gap(ref.M(np.diag([8.0, 4, 2, 1, 0.5, 0.125])), 5), 4)


def test_angle_axis_quaternion_and_distance_by_hand():
    R = ref.angle_axis([mpf(0), mpf(0), mp.pi / 2, 0, 0, 0])
    want = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    assert all(_close(R[i][j], want[i][j]) for i in range(3) for j in range(3))
    assert ref.angle_axis([mpf(0)] * 6) == ref.eye(3)
    br, q = ref.quat_from_rot(R)
    assert br == 0 and _close(q[0], mp.sqrt(mpf(1) / 2)) and _close(q[3], mp.sqrt(mpf(1) / 2)) and _close(q[1], 0) and _close(q[2], 0)
    for axis in range(3):                                            # half turns: trace -1, the branch of that axis
        d = [-1.0] * 3; d[axis] = 1.0
        br, q = ref.quat_from_rot(ref.M(np.diag(d)))
        assert br == 1 + axis and [float(v) for v in q] == [0.0] + [1.0 if k == axis else 0.0 for k in range(3)]
    # ties go to the earlier axis (Eigen's strict `>`)
    assert ref.quat_from_rot(ref.M([[0, 1, 0], [1, 0, 0], [0, 0, -1]]))[0] == 1
    assert ref.quat_from_rot(ref.M([[-1, 0, 0], [0, 0, 1], [0, 1, 0]]))[0] == 2
    qa = [mp.cos(mpf("0.1")), mp.sin(mpf("0.1")), mpf(0), mpf(0)]      # 0.2 rad about x
    qi = [mpf(1), mpf(0), mpf(0), mpf(0)]
    assert _close(ref.angular_distance(qa, qi), mpf("0.2")) and _close(ref.angular_distance(qa, [-v for v in qi]), mpf("0.2"))
    assert ref.angular_distance(qa, qa) == 0


def test_sigma_max_by_hand():
    assert _close(ref.sigma_max3(ref.M(np.diag([3.0, -7, 2]))), 7)
    assert _close(ref.sigma_max3(ref.M([[0, 2, 0], [0, 0, 0], [0, 0, 0]])), 2)      # not symmetric: no eigenvalue, one singular value
    # R(theta) - I about z: two singular values 2 sin(theta / 2), one zero
    th = 0.3
    D = cases.make_pose((0, 0, th))[:3, :3] - np.eye(3)
    assert abs(float(ref.sigma_max3(ref.M(D))) - 2 * np.sin(th / 2)) < 1e-15


def test_convergence_rule_by_hand():
    q0 = [mpf(1), mpf(0), mpf(0), mpf(0)]
    z = [mpf(0)] * 3
    assert ref.check_convergence([q0] * 4, [z] * 4)[0] is False                    # four entries: never
    assert ref.check_convergence([q0] * 5, [z] * 5)[0] is True
    step = lambda k, d: [mpf(k) * mpf(d), mpf(0), mpf(0)]
    assert ref.check_convergence([q0] * 5, [step(k, "0.00999") for k in range(5)])[0] is True
    assert ref.check_convergence([q0] * 5, [step(k, "0.01001") for k in range(5)])[0] is False
    assert ref.check_convergence([q0] * 6, [step(0, 0)] + [step(k, "0.00999") for k in range(5)])[0] is True


def test_quantile_rank_rule_by_hand():
    d2 = np.array([5.0, 1.0, 4.0, 2.0, 3.0, np.inf])
    limit, keep = ref.quantile_keep(d2, 0.7)                          # 5 finite values, int(5 * 0.69999999) = 3 -> the 4th smallest
    assert limit == 4.0 and keep.tolist() == [False, True, True, True, True, False]
    limit, keep = ref.quantile_keep(d2, 1.0)
    assert limit == 5.0 and keep.sum() == 5


def test_driver_recovers_a_known_motion_and_composes_with_the_mean():
    s = cases.get_scene("box")
    run = ref.scene_run("box")
    assert run["iterations"] == 5 and run["kept"] == [len(s["target"])] * 5 and run["ranks"] == [6] * 5
    assert run["min_gap"] >= 0.05
    # f32 rounding of the source is all that separates the answer from the motion: 1e-7 m on 3 m
    assert np.abs(ref.to_np(run["results"][5]) - s["motion"]).max() < 1e-7
    # the mean enters through T_mean T_iter T_mean^-1: a shifted copy of the scene gives the shifted answer
    off = np.array([8.0, -16.0, 4.0])
    r2 = ref.icp_driver(s["source"].astype(np.float64) + off, s["target"] + off, s["normals"], max_iteration=1)
    Tm = np.eye(4); Tm[:3, 3] = off
    Ti = np.eye(4); Ti[:3, 3] = -off
    want = ref.matmul(ref.M(Tm), ref.matmul(run["results"][1], ref.M(Ti)))
    assert all(_close(r2["results"][1][i][j], want[i][j], mpf(10) ** -45) for i in range(4) for j in range(4))


# ---------------------------------------------------------------------------------------------- the scenes are what they claim
def test_scenes_are_dyadic_symmetric_and_unambiguous():
    for nm in cases.SCENES + ["z_shift", "box07", "identical_box", "box_offset"]:
        s = cases.get_scene(nm)
        n = len(s["target"])
        assert 1500 <= n <= 2500, (nm, n)
        assert (s["target"] * 64 == np.round(s["target"] * 64)).all() and (s["target"].sum(axis=0) == 0).all(), nm
        assert (s["normals"].astype(np.float32).astype(np.float64) == s["normals"]).all(), nm
        if s["motion"] is not None:
            assert np.linalg.norm(s["motion"][:3, 3]) <= 0.03 + 1e-12, nm
            assert np.arccos(min(1.0, (np.trace(s["motion"][:3, :3]) - 1) / 2)) <= 0.003, nm
    for nm in cases.SCENES:
        run = ref.scene_run(nm)
        print(nm, "ranks", run["ranks"], "smallest runner-up gap %.4f m" % run["min_gap"])
        assert run["min_gap"] >= 0.05, (nm, run["min_gap"])
        s = cases.get_scene(nm)
        if s["rank"] is not None:
            assert run["ranks"] == [s["rank"]] * 5, (nm, run["ranks"])
    # the eps-corridors straddle the rule: Cholesky at the large tilts, minimum norm at the smallest
    L = {r["name"]: r for r in ref.ladder_reference()["rows"]}
    for e, rank in ((1e-3, 6), (1e-5, 6), (3e-6, 6), (1e-6, 6), (1e-8, 5)):
        r = L[f"scene:eps_corridor:{e:g}"]
        assert r["rank"] == rank and not r["in_band"], (e, r["rank"], r["ratio"])
    run = ref.scene_run("box07", max_iteration=2, ratio=0.7)
    assert run["min_gap"] >= 0.05 and run["min_quantile_gap"] >= 1e-3, (run["min_gap"], run["min_quantile_gap"])


# ---------------------------------------------------------------------------------------------- the oracles over the ladder
def _judge(solve, who):
    L = ref.ladder_reference()
    wrong, bad = [], []
    for r in L["rows"]:
        x, full = solve(r["A"], r["b"])
        assert np.isfinite(x).all(), (who, r["name"])
        if r["in_band"]:
            res = np.linalg.norm(r["A"] @ x - r["b"])
            assert res <= 1e-10 * (np.linalg.norm(r["A"], 2) * np.linalg.norm(x) + np.linalg.norm(r["b"])), (who, r["name"], res)
            continue
        if full is not None and full != (r["rank"] == 6):
            wrong.append((r["name"], r["ratio"], full))
        if r["rank"] < 6 and not r["gap"] >= 1e6:
            continue
        err = float(ref.norm([mpf(float(a)) - v for a, v in zip(x, r["x"])]))
        print(f"{who} {r['name']:30s} err {err:.3e} tol {r['tol']:.3e}")
        if not err <= r["tol"]:
            bad.append((r["name"], err, r["tol"]))
    assert not wrong, (who, wrong)
    assert not bad, (who, bad)


def test_c_oracle_over_the_decision_ladder():
    def solve(A, b):
        x, rank = cref.solve6(A, b)
        return x, rank == 6
    _judge(solve, "smref_icp.c")


def test_python_oracle_over_the_decision_ladder():
    """Its error IS the measure the tolerances are made of, so only its branch and its finiteness are news here."""
    def solve(A, b):
        if not np.abs(A).max() > 0:
            return np.zeros(6), None
        return py_oracle.solve_possibly_underdetermined(A, b), None
    _judge(solve, "icp_fast.py")
    L = ref.ladder_reference()
    assert abs(L["band"] - 4 * L["worst_pivot_error"]) < 1e-12 and 0.3 < L["worst_pivot_error"] < 0.4   # 0.362, B = 1.45
