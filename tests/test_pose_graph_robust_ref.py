"""What tests/pose_graph_robust_ref.py alone must satisfy for the C++ and device tests against it to mean anything (DESIGN.md
section 6, "Robust factors"): the cases of tests/pose_graph_robust_cases.py end by a stop rule and away from every place where two
correct implementations may part ways -- an acceptance decided inside the cost band, a factor on its threshold -- the direct and
PCG solves agree, the wrong edge is the one that loses its weight, the result is better than the plain solve's, zero thresholds
change no bit, and J^T r is the gradient of half the cost."""
import numpy as np
import pytest

import pose_graph_cases as base
import pose_graph_gps_ref as gps
import pose_graph_ref as ref
import pose_graph_robust_cases as cases
import pose_graph_robust_ref as robust

# the restatement's own numbers on the four rings (accepted / rejected steps, the corrupted edge's final weight, the error ratio
# against the plain solve): what the prototype behind the definition gave, to the digits it was quoted with
EXPECTED = {"robust16": (9, 0, 0.0586, 0.23), "robust64": (11, 0, 0.0573, 0.21), "robust65": (12, 0, 0.0584, 0.47), "robust240": (12, 0, 0.0554, 0.21)}


@pytest.mark.parametrize("name", cases.SMALL)
def test_the_cases_qualify(name):
    g, poses, st, (s, w, c) = cases.reference(name)
    _, other, so, _ = cases.reference(name, "pcg")
    plain, _ = cases.plain(name)
    assert st["stop"] in (ref.STOP_STEP, ref.STOP_COST)
    assert not [x for x in st["decrease_over_band"] if 0.95 <= x <= 1.05]
    hub = g["huber"]
    has = hub > 0.0
    assert (np.abs(s[has] - hub[has]) / hub[has] >= 1e-3).all()
    dt, dr = base.pose_difference(poses, other)
    ratio = cases.error(name, g, poses) / cases.error(name, g, plain)
    print(name, "steps", st["accepted"], st["rejected"], "direct against pcg", dt, dr, "weight of the wrong factor", w[g["bad"]], "error ratio", ratio)
    assert dt < 1e-9 and (st["accepted"], st["rejected"]) == (so["accepted"], so["rejected"])
    assert (w[g["bad"]] < 0.1).all()
    assert (w[[k for k in g["loops"] if k not in g["bad"]]] == 1.0).all() and (w[~has] == 1.0).all()
    assert ratio < 0.6
    assert abs(sum(c) - st["final_cost"]) <= 1e-12 * st["final_cost"]
    if name in EXPECTED:
        acc, rej, weight, err = EXPECTED[name]
        assert (st["accepted"], st["rejected"]) == (acc, rej)
        assert abs(w[g["bad"][0]] - weight) < 5e-5 and abs(ratio - err) < 5e-3
        assert dt <= 7.7e-12


def test_zero_thresholds_give_the_plain_restatement_bit_for_bit():
    for name in ("robust16", "robust_point"):
        g = dict(cases.graph(name))
        want, sw = gps.optimize(g)
        for hub in (None, np.zeros(len(g["kinds"]))):
            g["huber"] = hub
            got, sg = robust.optimize(g)
            assert got.tobytes() == want.tobytes()
            assert all(sg[key] == sw[key] for key in sw)
        g["huber"] = np.full(len(g["kinds"]), 1e30)       # never exceeded
        got, sg = robust.optimize(g)
        assert got.tobytes() == want.tobytes() and sg["costs"] == sw["costs"]


@pytest.mark.parametrize("name", ["robust16", "robust_point"])
def test_the_gradient_is_that_of_half_the_cost(name):
    """J^T r against a central difference of cost / 2 along every free coordinate, at the third iterate's neighbourhood: the
    restatement's result moved by 0.02 rad / m at every free node, where the wrong factor is above its threshold and the good ones
    are below.  h = 1e-6: the truncation is h^2 times a third derivative of order |g| / (0.1 m)^2, the rounding eps cost / h."""
    g, poses, _, _ = cases.reference(name)
    rng = np.random.default_rng(4)
    at = np.stack([P if f else ref.retract(P, rng.normal(size=6) * 0.02) for P, f in zip(poses, g["fixed"])])
    s, w, _ = robust.report(g, at)
    hub = g["huber"]
    assert (w < 1.0).any() and (w[hub > 0.0] == 1.0).any()
    assert (np.abs(s[hub > 0.0] - hub[hub > 0.0]) > 1e-3).all()      # no kink inside the difference
    _, grad = robust.assemble(g, at)
    h = 1e-6
    fd = np.zeros_like(grad)
    for k in range(len(at)):
        if g["fixed"][k]:
            continue
        for a in range(6):
            d = np.zeros(6)
            d[a] = h
            up, dn = at.copy(), at.copy()
            up[k], dn[k] = ref.retract(at[k], d), ref.retract(at[k], -d)
            fd[6 * k + a] = 0.5 * (robust.cost(g, up) - robust.cost(g, dn)) / (2.0 * h)
    print(name, "largest |g|", np.abs(grad).max(), "largest difference", np.abs(fd - grad).max())
    assert np.abs(fd - grad).max() <= 1e-6 * np.abs(grad).max()


def test_the_large_ring_qualifies():
    """robust1500 through the sparse solve: both wrong loops lose their weight, the six good ones keep theirs"""
    g, poses, st, (s, w, c) = cases.reference("robust1500")
    plain, _ = cases.plain("robust1500")
    hub = g["huber"]
    has = hub > 0.0
    ratio = cases.truth_error(g, poses) / cases.truth_error(g, plain)
    print("steps", st["accepted"], st["rejected"], "weights", w[g["loops"]], "error ratio", ratio)
    assert st["stop"] in (ref.STOP_STEP, ref.STOP_COST)
    assert not [x for x in st["decrease_over_band"] if 0.95 <= x <= 1.05]
    assert (np.abs(s[has] - hub[has]) / hub[has] >= 1e-3).all()
    assert (w[g["bad"]] < 0.1).all() and (w[[k for k in g["loops"] if k not in g["bad"]]] == 1.0).all()
    assert ratio < 0.6
