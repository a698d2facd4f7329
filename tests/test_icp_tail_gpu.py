"""The serial end of an IcpFast iteration ON THE DEVICE -- the 6x6 solve with its invertibility rule, the pose update, the history
ring and CheckConvergence (finalize_tail in csrc/icp_kernels.hip, arithmetic in csrc/icp_tail_math.h) -- on scenes whose normal
equations are rank deficient or nearly so: a plane, two parallel planes, a corridor, and corridors whose free axis is held by a
tilt of eps.  Every scene runs through the one-launch kernel (icp_one), the separate launches (`finalize`) and a two-slot batch,
and the pose is compared with the multi-precision driver of tests/icp_tail_ref.py.

Tolerance, per run: 8 x the error of the C oracle (f64, exact neighbours) against the same multi-precision run, with a floor of
64 eps |result| -- the margin convention of test_normals_exact_gpu.py.  The scenes keep every runner-up neighbour >= 0.05 m away
(asserted in test_icp_tail_ref.py and again here), so the matches are not in question and only the tail is measured.

The compensated kernel (`finalize_comp`): the mode fixes the sweep factors at f_i = i / n, so "every factor zero" is a source of
ONE row (f_0 = 0).  Its normal equations vanish, the solve must take the rank-0 path and the pose must stay at the guess, exactly.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_tail_cases as cases  # noqa: E402
import icp_tail_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = cases.EPS
PATHS = ("one_launch", "separate", "batch2")
ITERATIONS = (1, 2, 5)


@pytest.fixture(scope="module")
def smhip():
    import staticmapping_amd as sm
    from staticmapping_amd import _capi
    lib = _capi.load_library()
    assert lib.smhip_device_count() >= 1, "no gfx950 device visible"
    return sm


def _align(sm, s, path, guess=None, **opts):
    """-> (result 4x4, stats) of slot 0 (and the assertion that every slot of a batch answers alike)."""
    slots = 2 if path == "batch2" else 1
    if path != "one_launch":
        opts["no_single_kernel"] = 1
    m = sm.IcpFastHip(pair_slots=slots, max_source_points=len(s["source"]), max_target_points=len(s["target"]), **opts)
    try:
        for k in range(slots):
            m.set_input_source(s["source"].astype(np.float64), slot=k)
            m.set_input_target(s["target"], s["normals"], slot=k)
        res, _, stats = m.align_batch(slots, None if guess is None else [guess] * slots)
        used, fell = m.single_launch_counts()
        assert fell == 0 and (used == 1 if path == "one_launch" else used == 0), (path, used, fell)
        for k in range(1, slots):
            assert np.array_equal(res[k], res[0]) and stats[k] == stats[0], "the two slots hold the same pair"
        return res[0].copy(), dict(stats[0])
    finally:
        m.close()


_ORACLE = {}


def _c_oracle(name, iters, ratio=1.0, early_exit=False):
    key = (name, iters, ratio, early_exit)
    if key not in _ORACLE:
        from oracle import cref
        s = cases.get_scene(name)
        _ORACLE[key] = cref.icp_fast_align(s["source"].astype(np.float64), s["target"], s["normals"], max_iteration=iters,
                                           dist_outlier_ratio=ratio, early_exit=early_exit)
    return _ORACLE[key]


def _err(T, exact):
    return float(np.linalg.norm(np.asarray(T) - ref.to_np(exact)))    # (f64 of the exact entries: 1e-16 of 1, far below any tolerance here)


def _tolerance(name, iters, exact, ratio=1.0):
    o = _c_oracle(name, iters, ratio)
    return max(8.0 * _err(o["result"], exact), 64.0 * EPS * float(np.linalg.norm(ref.to_np(exact)))), _err(o["result"], exact)


def _in_band(name):
    rows = {r["name"]: r for r in ref.ladder_reference()["rows"]}
    r = rows.get("scene:" + name)
    return bool(r and r["in_band"])


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", cases.SCENES)
def test_pose_against_the_multi_precision_driver(smhip, name, path):
    s = cases.get_scene(name)
    runs = [ref.scene_run(name)]
    if _in_band(name):                                               # an f64 QR cannot tell which side of the rule this matrix is on: either
        runs.append(ref.scene_run(name, force_rank=5))
    for run in runs:
        assert run["min_gap"] >= 0.05, (name, run["min_gap"])
    for iters in ITERATIONS:
        T, st = _align(smhip, s, path, max_iteration=iters, early_exit=0, dist_outlier_ratio=1.0)
        assert st["status"] == 0 and st["iterations"] == iters and st["kept"] == runs[0]["kept"][iters - 1], (name, path, iters, st)
        assert np.isfinite(T).all()
        verdicts = []
        for run in runs:
            exact = run["results"][iters]
            tol, oracle_err = _tolerance(name, iters, exact) if len(runs) == 1 else (None, None)
            if tol is None:                                          # the oracle too is on one side: its error against ITS side counts
                o = _c_oracle(name, iters)
                oracle_err = min(_err(o["result"], r["results"][iters]) for r in runs)
                tol = max(8.0 * oracle_err, 64.0 * EPS * float(np.linalg.norm(ref.to_np(exact))))
            err = _err(T, exact)
            print(f"{name} {path} iterations {iters} ranks {run['ranks'][:iters]}: device error {err:.3e}, oracle error {oracle_err:.3e}, tolerance {tol:.3e}")
            verdicts.append(err <= tol)
        assert any(verdicts), (name, path, iters)


def test_disputed_eps_scene_takes_the_reference_rules_branch(smhip):
    """eps = 1e-6: the smallest QR pivot is 12.9 x the rule's threshold, so the reference solves the corridor's axis (Cholesky) --
    where a Cholesky-pivot threshold of 1e-13 dmax gave it up and left the pose 0.0107 m short along the corridor."""
    name = "eps_corridor:1e-06"
    s = cases.get_scene(name)
    full, reduced = ref.scene_run(name), ref.scene_run(name, force_rank=5)
    assert full["ranks"] == [6] * 5 and not _in_band(name)
    assert abs(float(full["results"][1][0][3]) - 11 / 1024) < 1e-9 and abs(float(reduced["results"][1][0][3])) < 1e-6
    for path in PATHS:
        T, _ = _align(smhip, s, path, max_iteration=1, early_exit=0, dist_outlier_ratio=1.0)
        tol, _ = _tolerance(name, 1, full["results"][1])
        print(path, "x translation", T[0, 3], "error", _err(T, full["results"][1]), "tolerance", tol)
        assert _err(T, full["results"][1]) <= tol and abs(T[0, 3] - 11 / 1024) < 1e-6, (path, T[0, 3])


@pytest.mark.parametrize("path", PATHS)
def test_pure_z_shift_of_a_plane_leaves_the_rotation_exactly_the_identity(smhip, path):
    """b is exactly (0, 0, 0, 0, 0, -N shift) and A exactly diagonal of rank 3: x[0:3] = 0, the angle-axis step divides 0 by 0 and
    its NaN guard must put the identity back -- exactly -- while the translation is kept."""
    s = cases.get_scene("z_shift")
    run = ref.scene_run("z_shift")
    assert run["ranks"] == [3] * 5 and run["min_gap"] >= 0.05
    for iters in ITERATIONS:
        T, st = _align(smhip, s, path, max_iteration=iters, early_exit=0, dist_outlier_ratio=1.0)
        assert st["status"] == 0 and st["iterations"] == iters and st["kept"] == len(s["target"])
        assert np.array_equal(T[:3, :3], np.eye(3)), (path, iters, T)
        tol, _ = _tolerance("z_shift", iters, run["results"][iters])
        assert _err(T, run["results"][iters]) <= tol, (path, iters, T[:3, 3])
        assert abs(T[2, 3] + s["shift"]) <= tol and T[0, 3] == 0 and T[1, 3] == 0, (path, iters, T[:3, 3])


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["identical_box", "box_offset"])
def test_early_exit_stops_at_the_drivers_iteration(smhip, name, path):
    """The history ring at the first iteration where CheckConvergence is possible: five entries, the identity among them."""
    s = cases.get_scene(name)
    run = ref.scene_run(name, max_iteration=20, early_exit=True)
    assert run["iterations"] == 4 and run["min_gap"] >= 0.05
    T, st = _align(smhip, s, path, max_iteration=20, early_exit=1, dist_outlier_ratio=1.0)
    assert st["status"] == 0 and st["iterations"] == run["iterations"], (name, path, st)
    o = _c_oracle(name, 20, 1.0, True)
    assert o["iterations"] == run["iterations"]
    exact = run["results"][run["iterations"]]
    tol = max(8.0 * _err(o["result"], exact), 64.0 * EPS * float(np.linalg.norm(ref.to_np(exact))))
    assert _err(T, exact) <= tol, (name, path, _err(T, exact), tol)


@pytest.mark.parametrize("path", PATHS)
def test_box_at_ratio_07(smhip, path):
    s = cases.get_scene("box07")
    run = ref.scene_run("box07", max_iteration=2, ratio=0.7)
    assert run["min_gap"] >= 0.05 and run["min_quantile_gap"] >= 1e-3      # the kept set is not in question
    for iters in (1, 2):
        T, st = _align(smhip, s, path, max_iteration=iters, early_exit=0, dist_outlier_ratio=0.7)
        assert st["status"] == 0 and st["iterations"] == iters and st["kept"] == run["kept"][iters - 1], (path, iters, st, run["kept"])
        tol, _ = _tolerance("box07", iters, run["results"][iters], ratio=0.7)
        assert _err(T, run["results"][iters]) <= tol, (path, iters, _err(T, run["results"][iters]), tol)


@pytest.mark.parametrize("batch", [False, True])
def test_compensated_tail_with_vanishing_normal_equations_keeps_the_guess(smhip, batch):
    """One source row: its sweep factor is 0 / 1 = 0, the compensated row scales J by it, A and b are exactly zero.  The solve must
    answer the zero matrix with x = 0 (rank 0), the NaN guard with the identity: the pose stays at the guess, bit for bit."""
    s = cases.get_scene("box")
    guess = cases.make_pose((0.001, 0.002, -0.001), (0.01, -0.005, 0.02))
    slots = 2 if batch else 1
    m = smhip.IcpFastHip(pair_slots=slots, max_source_points=8, max_target_points=len(s["target"]), inner_compensation=True)
    try:
        for k in range(slots):
            m.set_input_source((s["target"][:1] + np.array([0.01, 0.0, 0.01])), slot=k)
            m.set_input_target(s["target"], s["normals"], slot=k)
        for iters in ITERATIONS:
            m.set_options(max_iteration=iters, early_exit=0, dist_outlier_ratio=1.0)
            res, _, stats = m.align_batch(slots, [guess] * slots)
            for k in range(slots):
                assert stats[k]["status"] == 0 and stats[k]["iterations"] == iters and stats[k]["kept"] == 1, stats[k]
                assert np.array_equal(res[k], guess), (iters, res[k] - guess)
    finally:
        m.close()
