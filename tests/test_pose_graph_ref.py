"""tests/pose_graph_ref.py against itself (no GPU): its Jacobians against central differences of its own residual, a consistent graph
recovered from a perturbed start, and its two solvers -- dense direct and chain-preconditioned conjugate gradients -- at the same
poses."""
import numpy as np
import pytest

import pose_graph_cases as cases
import pose_graph_ref as ref


def _central(Xi, Xj, Z, h):
    A, B = np.zeros((6, 6)), np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        A[:, k] = (ref.residual(ref.retract(Xi, d), Xj, Z) - ref.residual(ref.retract(Xi, -d), Xj, Z)) / (2 * h)
        B[:, k] = (ref.residual(Xi, ref.retract(Xj, d), Z) - ref.residual(Xi, ref.retract(Xj, -d), Z)) / (2 * h)
    return A, B


@pytest.mark.parametrize("angle", [None, 1e-9, 1e-3, 0.5 * np.pi, 2.2, 3.0, np.pi - 1e-6])
def test_jacobians_agree_with_central_differences(angle):
    """Random poses; the residual rotation E is set to `angle` about a random axis (None: uniform in [0, pi]) -- 1e-9 is inside both
    small-angle series, pi - 1e-6 inside the branch that takes the axis from the symmetric part.  Step 1e-6: the truncation error is
    h^2 / 6 times a third derivative of order |t| ~ 10, about 2e-11; the rounding error is eps |e| / h with |e| up to ~ 20 (metres), about
    5e-9.  Bound 2e-8."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(20):
        Xi, Xj = ref.random_pose(rng), ref.random_pose(rng)
        E = ref.random_pose(rng, angle=angle, scale=1.0)
        Z = ref.inv(Xi) @ Xj @ ref.inv(E)                     # so that Z^-1 Xi^-1 Xj = E
        e, A, B = ref.jacobians(Xi, Xj, Z)
        if angle is not None:
            assert abs(np.linalg.norm(e[:3]) - angle) < 1e-9 * max(1.0, angle / 1e-9 * 1e-7)
        a, b = _central(Xi, Xj, Z, 1e-6)
        worst = max(worst, np.abs(A - a).max(), np.abs(B - b).max())
    print("worst difference", worst)
    assert worst < 2e-8


def test_log_is_the_inverse_of_exp_at_every_branch():
    rng = np.random.default_rng(6)
    for th in (0.0, 1e-12, 1e-5, 0.9e-4, 1.1e-4, 0.5, 2.0, 2.0944, 2.0945, 3.0, np.pi - 1e-6, np.pi - 1e-9):
        a = rng.normal(size=3)
        a /= np.linalg.norm(a)
        assert np.abs(ref.log_so3(ref.exp_so3(th * a)) - th * a).max() < 1e-12, th      # (at pi - 1e-9 the angle itself is the hard part)
    # exactly pi: either sign of the axis is the same rotation
    a = np.array([2.0, -1.0, 0.5]) / np.linalg.norm([2.0, -1.0, 0.5])
    assert np.abs(np.abs(ref.log_so3(2 * np.outer(a, a) - np.eye(3))) - np.pi * np.abs(a)).max() < 1e-12


def test_a_consistent_graph_is_recovered():
    """Edges measured from the truth without noise, the start 0.1 rad / 0.3 m off at every free node: the cost goes to (rounding)
    zero and every pose back to the truth.  Cost bound: residuals of ~50 eps |t| / sigma with |t| ~ 100 m are ~1e-11, squared and
    summed over 45 x 6 entries: below 1e-19."""
    g = cases.chain_graph(40, 21, loops=[(0, 39), (5, 30), (12, 13 + 9), (3, 17), (25, 8), (30, 2)], rot_noise=0.0, trans_noise=0.0, start_noise=0.1)
    g["poses"][1:, :3, 3] += np.random.default_rng(3).normal(size=(39, 3)) * 0.3
    for solver in ("direct", "pcg"):
        poses, st = ref.optimize(g["poses"], g["fixed"], g["edges"], g["Z"], solver=solver)
        print(solver, st["costs"], st["stop"], st["rejected"])
        assert st["initial_cost"] > 100 and st["final_cost"] < 1e-19
        assert np.abs(poses - g["truth"]).max() < 1e-9
        assert st["stop"] in (ref.STOP_STEP, ref.STOP_COST)


@pytest.mark.parametrize("name", ["circle64", "circle240", "n5", "n63", "n64", "n65", "missing_chain_edge", "fixed_in_the_middle", "near_pi", "triangle"])
def test_direct_and_preconditioned_solves_reach_the_same_poses(name):
    """Both walk the same Gauss-Newton steps and take the same decisions: a step whose cost change is inside the rounding of the cost
    is accepted by either (the band of the module docstring; without it the direct solve rejected one such step on n64 that the
    preconditioned one took, and the two ended 2.8e-11 m apart).  Both walk the same steps (the inner solve's 1e-8 relative residual moves a step by 1e-8 of itself), so they
    differ by rounding: 1e-11 m is a hundred times what an f64 solve of these systems leaves (~1e-13) and a hundredth of the 1e-9
    the device is held to.  The preconditioned solve stays below its cap, and at the circle drives below 30 iterations per step with
    three loop edges -- block-Jacobi needs hundreds to thousands there."""
    g, want, st = cases.reference(name)
    got, st2 = ref.optimize(g["poses"], g["fixed"], g["edges"], g["Z"], solver="pcg")
    dt, dr = cases.pose_difference(got, want)
    print(name, "difference", dt, dr, "pcg iterations", st2["pcg_iterations"], "longest", st2["pcg_max"], "steps", st2["accepted"], st2["rejected"])
    assert dt < 1e-11 and dr < 1e-11
    assert st2["pcg_max"] < 12 * ref.non_chain_edges(g["edges"]) + 64
    if name.startswith("circle"):
        assert st2["pcg_max"] < 30
        assert st["final_cost"] < 1e-3 * st["initial_cost"]
