"""tests/pose_graph_gps_ref.py, the restatement of the PRIOR and POINT factors and of IsamOptimizer's GPS bookkeeping, checked on
its own: Jacobians against central differences, the PRIOR against its fixed-twin BETWEEN, direct against PCG, the iteration counts
the rank argument of DESIGN.md section 6 predicts, the alone-solve from identity, and what the factors do to a drifted drive."""
import numpy as np
import pytest

import pose_graph_cases as base
import pose_graph_gps_cases as cases
import pose_graph_gps_ref as gps
import pose_graph_ref as ref


def _numeric(kind, Xi, Xj, data, h=1e-6):
    """plain central differences of the residual along the retraction: (e, A, B); a PRIOR has node i alone"""
    e0 = gps.factor_residual(kind, Xi, Xj, data)
    A, B = np.zeros((6, 6)), np.zeros((6, 6))
    for c in range(6):
        d = np.zeros(6)
        d[c] = h
        if kind == gps.PRIOR:
            plus, minus = ref.retract(Xi, d), ref.retract(Xi, -d)
            A[:, c] = (gps.factor_residual(kind, plus, plus, data) - gps.factor_residual(kind, minus, minus, data)) / (2 * h)
            continue
        A[:, c] = (gps.factor_residual(kind, ref.retract(Xi, d), Xj, data) - gps.factor_residual(kind, ref.retract(Xi, -d), Xj, data)) / (2 * h)
        B[:, c] = (gps.factor_residual(kind, Xi, ref.retract(Xj, d), data) - gps.factor_residual(kind, Xi, ref.retract(Xj, -d), data)) / (2 * h)
    return e0, A, B


@pytest.mark.parametrize("angle", [1e-9, 0.3, 2.0, np.pi - 1e-6])
def test_prior_jacobian_against_central_differences(angle):
    """Every entry of A against (e(X retract +h) - e(X retract -h)) / 2h at h = 1e-6, the rotation block included: at pi - 1e-6 a
    step of 1e-6 along one coordinate moves the angle by less than 1e-6 (the axis has no unit component), so Log stays on one
    branch.  Truncation h^2 x (third derivative) / 6 ~ 1e-12 and cancellation eps |e| / h ~ 1e-9: the bound is 1e-7."""
    rng = np.random.default_rng(17)
    P = ref.random_pose(rng, angle=0.7)
    a = np.array([0.3, -0.5, 0.81])
    a /= np.linalg.norm(a)
    X = P.copy()
    X[:3, :3] = P[:3, :3] @ ref.exp_so3(angle * a)
    X[:3, 3] = P[:3, 3] + [0.4, -1.0, 0.3]
    e, A, B = gps.factor_jacobians(gps.PRIOR, X, X, gps.prior_data(P))
    assert abs(np.linalg.norm(e[:3]) - angle) < 1e-9 and (B == 0.0).all()
    _, An, _ = _numeric(gps.PRIOR, X, X, gps.prior_data(P))
    print("angle", angle, "worst difference", np.abs(A - An).max())
    assert np.abs(A - An).max() < 1e-7
    assert (A[:3, 3:] == 0.0).all() and (A[3:, :3] == 0.0).all()


def test_a_wrong_inverse_right_jacobian_would_be_noticed(monkeypatch):
    """the check above has teeth: with Jr^-1 replaced by another invertible matrix the analytic block is far from the differences"""
    monkeypatch.setattr(ref, "jr_inv", lambda phi: np.eye(3) + 0.25 * ref.hat(phi))
    rng = np.random.default_rng(17)
    P = ref.random_pose(rng, angle=0.7)
    X = ref.retract(P, np.array([0.2, -0.3, 0.5, 0.4, -1.0, 0.3]))
    _, A, _ = gps.factor_jacobians(gps.PRIOR, X, X, gps.prior_data(P))
    _, An, _ = _numeric(gps.PRIOR, X, X, gps.prior_data(P))
    assert np.abs(A[:3, :3] - An[:3, :3]).max() > 1e-2 and np.abs(A[3:] - An[3:]).max() < 1e-7


def test_point_jacobians_against_central_differences():
    rng = np.random.default_rng(18)
    worst = 0.0
    for _ in range(20):
        Xi, Xj = ref.random_pose(rng, scale=100.0), ref.random_pose(rng, scale=30.0)
        data = gps.point_data(rng.normal(size=3), rng.normal(size=3) * 100.0)
        e, A, B = gps.factor_jacobians(gps.POINT, Xi, Xj, data)
        _, An, Bn = _numeric(gps.POINT, Xi, Xj, data)
        worst = max(worst, np.abs(A - An).max(), np.abs(B - Bn).max())
        assert (e[3:] == 0.0).all() and (A[3:] == 0.0).all() and (B[3:] == 0.0).all()
    print("worst difference", worst)
    # central differences at h = 1e-6 of entries up to |p| ~ 100: h^2 |p| / 6 ~ 2e-11 truncation, eps |z| / h ~ 1e-7 cancellation
    assert worst < 1e-6


@pytest.mark.parametrize("angle", [1e-9, 0.4, np.pi - 1e-6])
def test_prior_is_the_between_from_a_fixed_twin(angle):
    """the BETWEEN from a constant node at P measured as the identity: the same residual, and that factor's B"""
    rng = np.random.default_rng(19)
    P = ref.random_pose(rng)
    X = ref.retract(P, np.concatenate([angle * np.array([0.6, 0.0, 0.8]), [0.5, -2.0, 0.1]]))
    e, A, _ = gps.factor_jacobians(gps.PRIOR, X, X, gps.prior_data(P))
    eb, _, Bb = ref.jacobians(P, X, np.eye(4))
    assert np.abs(e - eb).max() < 1e-15 * max(1.0, np.abs(e).max()) * 8 and np.abs(A - Bb).max() < 1e-14
    # and as graphs: a free node with a PRIOR ends where the node with a BETWEEN to a fixed twin ends
    start = ref.random_pose(rng)
    g = gps.make_graph([start], [0], [(gps.PRIOR, 0, 0, gps.prior_data(P), ref.DEFAULT_SIGMAS)])
    got, st = gps.optimize(g)
    want, sw = ref.optimize(np.stack([P, start]), np.array([1, 0], np.uint8), [(0, 1)], np.eye(4)[None])
    assert max(base.pose_difference(got[:1], want[1:])) < 1e-12 and (st["accepted"], st["rejected"]) == (sw["accepted"], sw["rejected"])
    assert max(base.pose_difference(got[:1], P[None])) < 1e-9


CASES = ["alone", "drive240", "drive64_all", "drive240_all", "chain1_all", "chain2_last", "chain4_second", "chain23_all", "chain63_second", "chain64_last"]


@pytest.mark.parametrize("name", CASES)
def test_direct_and_pcg_agree(name):
    same, diff = cases.qualifies(name)
    g, p, st = cases.reference(name)
    _, _, sq = cases.reference(name, "pcg")
    print(name, "direct", st["accepted"], st["rejected"], "pcg", sq["accepted"], sq["rejected"], sq["pcg_each"], "difference", diff)
    assert same and diff < 1e-10
    assert st["stop"] in (ref.STOP_STEP, ref.STOP_COST)
    assert cases.gradient_ratio(g, p) < 1e-9


def test_the_drive_of_seed_3_is_the_documented_example_that_need_not_qualify():
    """n = 240, three loops, a factor every second node, seed 3: a prototype of this generator saw the two solves stop one step apart
    at the flat minimum (3.5e-7 apart).  With this file's generator they agree; either way the graph is not used for device parity.
    What is asserted is only what holds in both outcomes: each solve ends at a minimum of its own."""
    same, diff = cases.qualifies("drive240_seed3")
    print("same counts", same, "difference", diff)
    g, p, _ = cases.reference("drive240_seed3")
    assert diff < 1e-6 and cases.gradient_ratio(g, p) < 1e-9


@pytest.mark.parametrize("name", ["drive64_all", "drive240_all", "alone"])
def test_pcg_needs_a_dozen_iterations_whatever_n_is(name):
    """M keeps every diagonal block and the chain; the frame node's arrow is all that is left of H, of rank at most 12, so CG ends in
    a dozen iterations at 64 and at 240 nodes (drives that never close a loop, a factor on every node) and for the alone graph.
    Every interior loop edge adds 12 more distinct eigenvalues: drive240_all_loops (three loop edges, one of them at the fixed node)
    measured 40-43, as the existing cap 12 x (non-chain factors) + 64 allows for."""
    _, _, sq = cases.reference(name, "pcg")
    print(name, sq["pcg_each"])
    assert 0 < max(sq["pcg_each"]) < 30


def test_interior_loop_edges_cost_twelve_iterations_each():
    g = cases.graph("drive240_all_loops")
    H, _ = gps.assemble(g, g["poses"])
    ev = np.linalg.eigvals(np.linalg.solve(ref.chain_part(H), H)).real
    assert int((np.abs(ev - 1.0) > 1e-6).sum()) <= 12 + 2 * 12          # the arrow, and the two loop edges between free nodes


@pytest.mark.parametrize("yaw", [0.4, 1.2, 2.6, -3.0])
def test_alone_solve_from_identity_puts_the_antennas_in_place_at_every_yaw(yaw):
    """The first 25 poses of the seed-5 drive at their true places (the alone graph holds them with sigma 1e-2, so a drifted pose is a
    different frame, not an error of the solve), ENU with 0.05 m of noise, the frame started at identity.  What is asserted is not
    the frame's own translation -- the image of the map origin, 150 m from the data, which 0.009 rad of tilt moves by 1.3-1.4 m and
    which is only printed -- but the frame where it is observed.  Every yaw ends in the same frame there: the antennas of the 25 poses land within 0.30 m of their true ENU places and the rotation is within 0.014 rad of the truth.
    Measured: 4, 6, 16 and 19 steps (none rejected at 0.4 and 1.2, 7 of them rejected at 2.6 and -3.0, where the start is more than
    2.2 rad away); rotation 0.0089-0.0093 rad off for all four -- the tilt about the 100 m arc's chord, which 0.05 m of noise over
    an 8 m sagitta leaves that loose -- and therefore the image of the map origin, 150 m from the data, 1.32-1.37 m off; the antennas
    themselves are printed below."""
    truth = ref.circle_drive(240, 5)["truth"][:25]
    frame = ref.make_pose((0.01, -0.02, yaw), (350.0, -120.0, 12.0))
    enu = cases.enu_of(truth, 5, frame=frame)
    got, st = gps.alone_solve(truth, enu, cases.LEVER)
    at_origin = np.linalg.norm(got[:3, 3] - frame[:3, 3])
    dt = np.linalg.norm(cases.enu_positions(truth, got) - cases.enu_positions(truth, frame), axis=1).max()
    dr = np.linalg.norm(ref.log_so3(frame[:3, :3].T @ got[:3, :3]))
    print("yaw", yaw, "steps", st["accepted"], st["rejected"], "antennas off by", dt, "rotation", dr, "the origin's image", at_origin)
    assert st["stop"] in (ref.STOP_STEP, ref.STOP_COST) and st["accepted"] + st["rejected"] <= 30
    assert dt < 0.30 and dr < 0.014


def test_gps_factors_bound_the_drift_of_a_drive():
    g, p, st = cases.reference("drive240")
    before, after = cases.enu_error(g, g["poses"]), cases.enu_error(g, p)
    print("ENU-frame error before %.3f m, after %.3f m" % (before, after))
    assert before > 5.0 and after <= 0.1 * before


def test_gps_rule():
    """:264-288 on made-up fixes and angles"""
    has = [True] * 40
    ang = [0.049 * k for k in range(40)]                   # passes 1.6 at frame 33
    r = gps.gps_rule(has, ang, init_num=25)
    assert r["cached"] == list(range(33)) and r["trigger"] == 33 and r["sampled"] == list(range(34, 40))
    r = gps.gps_rule(has, ang, init_num=36)                # the angle is there first, the count decides
    assert r["cached"] == list(range(36)) and r["trigger"] == 36
    r = gps.gps_rule(has, [0.0] * 40)                      # never turns: everything cached, no factor at all
    assert r["trigger"] is None and r["factors"] == [] and len(r["cached"]) == 40
    r = gps.gps_rule(has, ang, init_num=5, sample_step=2)
    assert r["trigger"] == 33 and r["sampled"] == [34, 36, 38]
    has[3] = has[33] = has[35] = False
    r = gps.gps_rule(has, ang, init_num=5)
    assert 3 not in r["cached"] and r["trigger"] == 34 and r["sampled"] == [36, 37, 38, 39]
    assert r["factors"] == r["cached"] + r["sampled"]
