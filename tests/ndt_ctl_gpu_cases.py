"""The GPU cases of tests/test_ndt_ctl_gpu.py, one per process: `python tests/ndt_ctl_gpu_cases.py CASE`.  Every case prints its
figures before it asserts and ends with the line `ok CASE`."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

try:                                  # one HIP runtime per process: torch's first (tests/conftest.py)
    import torch  # noqa: F401
except ImportError:
    pass
import numpy as np

import staticmapping_amd as sm
from staticmapping_amd import synth
from oracle import cref


def f32(v):
    """An option as the device holds it (smhip_ndt_options' fields are floats)."""
    return float(np.float32(v))


def scene():
    """ndt_case of tests/test_ndt_gpu.py, smaller: a 3 000-point scan against 12 000 points merged from 3 scans."""
    sc = synth.make_scene(0)
    poses = [synth.make_pose(t=(0.8 * k, 0.02 * k, 0.0), rpy_deg=(0, 0, 0.5 * k)) for k in range(4)]
    scans = [synth.velodyne_scan(sc, P, seed=10 + k, n_points=(4000 if k < 3 else 3000)) for k, P in enumerate(poses)]
    tgt = np.concatenate([s[:, :3].astype(np.float64) @ P[:3, :3].T + P[:3, 3] for s, P in zip(scans[:3], poses[:3])])
    tgt = np.concatenate([tgt, np.zeros((len(tgt), 1))], axis=1).astype(np.float32)
    return scans[3], tgt, poses[3]


def guess(T, name):
    """0.3: 0.3 m short along x (ndt_case's).  0.8: 0.8 m short along x and pitched by 2 degrees -- of the 96 guesses 0.8 m away in
    the plane with 2 degrees about one axis, one of the two for which the oracle's line search loops under all three option
    pairs of mt_loop.  0.8yaw: 0.8 m away and yawed by 2 degrees, the guess of the exits (its first Newton step is longer than
    step_size, and at epsilon 0.01 it needs 20 iterations).  The others: the batch's, chosen for different loop lengths."""
    t, rpy = {"0.3": ((-0.3, 0, 0), (0, 0, 0)), "0.8": ((-0.8, 0, 0), (0, 2.0, 0)), "0.8yaw": ((-0.8, 0.1, 0), (0, 0, 2.0)), "x0.2": ((-0.2, 0.05, 0), (0, 0, 0.3)),
              "x0.45": ((-0.45, 0.05, 0), (0, 0, 0.3)), "x1.2": ((-1.2, 0.05, 0), (0, 0, 0.3))}[name]
    return T @ synth.make_pose(t=t, rpy_deg=rpy)


def matcher(src, tgt, slots=1, **opts):
    m = sm.NdtHip(max_source_points=len(src), max_target_points=len(tgt), pair_slots=slots, **opts)
    for k in range(slots):
        m.set_input_source(src, slot=k); m.set_input_target(tgt, slot=k)
    return m


def oracle(src, tgt, G, step_size=0.1, trans_eps=0.1, max_iterations=35):
    return cref.ndt_align(src, tgt, guess=G, step_size=f32(step_size), trans_eps=f32(trans_eps), max_iterations=max_iterations)


WORST = dict(da=0.0, dt=0.0, fit=0.0, tp=0.0)


def compare(tag, R, fit, st, ref):
    """iterations and derivative calls equal; pose, fitness score and transformation probability inside the bounds of
    test_ndt_align_parity (tests/test_ndt_gpu.py): 1e-4 rad, 1e-3 m, 1e-3 and 1e-4 relative."""
    da, dt = sm.se3_error(R, ref["result"])
    dfit = abs(fit - ref["score"]) / ref["score"]
    dtp = abs(st["trans_probability"] - ref["trans_probability"]) / abs(ref["trans_probability"]) if ref["trans_probability"] else abs(st["trans_probability"])
    print(f"{tag}: iterations {st['iterations']} / {ref['iterations']}, derivative calls {st['derivative_calls']} / {ref['derivative_calls']}, "
          f"rotation {da:.3e} (1e-4), translation {dt:.3e} (1e-3), fitness {dfit:.3e} (1e-3), probability {dtp:.3e} (1e-4); "
          f"oracle loop lengths {[r['trials'] for r in ref['trace']]}")
    for k, v in (("da", da), ("dt", dt), ("fit", dfit), ("tp", dtp)):
        WORST[k] = max(WORST[k], v)
    assert st["iterations"] == ref["iterations"] and st["derivative_calls"] == ref["derivative_calls"], (tag, st, ref["iterations"], ref["derivative_calls"])
    assert da < 1e-4 and dt < 1e-3, (tag, da, dt)
    assert dfit <= 1e-3 and dtp <= 1e-4, (tag, dfit, dtp)


def report_worst():
    print("worst: rotation %.3e rad (bound 1e-4), translation %.3e m (1e-3), fitness %.3e (1e-3), probability %.3e (1e-4)" %
          (WORST["da"], WORST["dt"], WORST["fit"], WORST["tp"]))


# ---------------------------------------------------------------------------------------------------- solve6_device
def case_solve6_device():
    """smhip_ndt_debug_solve6 (ndt_solve6 as hipcc compiles it: a * b + c contracted) on the systems of ndt_ctl_cases under the
    tolerance rule of test_ndt_ctl_cpp.py."""
    import ndt_ctl_cases as cases
    import ndt_ctl_ref as ref
    rows = ref.judged_systems()
    dropped = [r["name"] for r in rows if not r["admissible"]]
    assert len(dropped) <= cases.MAX_DROPPED_SHARE * len(rows), dropped
    m = sm.NdtHip(max_source_points=64, max_target_points=64)
    try:
        X = m.debug_solve6(np.stack([r["H"] for r in rows]), np.stack([r["b"] for r in rows]))
        X1 = m.debug_solve6(rows[-1]["H"][None], rows[-1]["b"][None])
    finally:
        m.close()
    assert np.array_equal(X1[0], X[-1])                              # a lane's answer does not depend on its neighbours
    bad, worst = [], {}
    for r, x in zip(rows, X):
        if not r["admissible"]:
            continue
        err = ref.error(x, r["x"])
        print(f"{r['name']:32s} kept {r['kept']} cond_kept {r['cond_kept']:.2e} err {err:.3e} tol {r['tol']:.3e} (oracle {r['oracle_err']:.3e})")
        if r["tol"] > 0 and err / r["tol"] > worst.get(r["family"], (0, 0, 0))[0]:
            worst[r["family"]] = (err / r["tol"], err, r["tol"])
        if not err <= r["tol"]:
            bad.append((r["name"], err, r["tol"]))
    print("worst error / tolerance per family:", {k: f"{v[0]:.3f} ({v[1]:.2e} / {v[2]:.2e})" for k, v in worst.items()})
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------- mt_loop
MT_OPTIONS = ((0.05, 0.1), (0.1, 0.2), (0.1, 0.5))


def case_mt_loop():
    src, tgt, T = scene()
    for ss, te in MT_OPTIONS:
        m = matcher(src, tgt, step_size=ss, transformation_epsilon=te)
        try:
            for gname in ("0.3", "0.8"):
                G = guess(T, gname)
                ref = oracle(src, tgt, G, ss, te)
                # the loop ran, with at least 2 trials, and the closing Hessian-only evaluation happened
                assert any(r["trials"] >= 2 and r["hessian_eval"] for r in ref["trace"]), (ss, te, gname, ref["trace"])
                _, R = m.align(G)
                compare(f"step_size {ss} epsilon {te} guess {gname}", R, m.get_fitness_score(), m.last_ndt_stats, ref)
        finally:
            m.close()
    report_worst()


# ---------------------------------------------------------------------------------------------------- exits
def case_exits():
    src, tgt, T = scene()
    # no overlap: nothing within a voxel of any point, score = gradient = Hessian = 0, dp_norm == 0 at once
    far = src.copy(); far[:, 0] += 200.0
    m = matcher(far, tgt)
    try:
        G = np.eye(4)
        _, R = m.align(G)
        st, fit = m.last_ndt_stats, m.get_fitness_score()
        ref = oracle(far, tgt, G)
        print("no overlap:", st, fit, "oracle", ref["iterations"], ref["derivative_calls"], ref["score"])
        assert np.array_equal(R, G) and st["iterations"] == 0 and st["derivative_calls"] == 1 and st["pairs_last"] == 0 and np.isfinite(fit), (R, st, fit)
        assert ref["iterations"] == 0 and ref["derivative_calls"] == 1 and np.array_equal(ref["result"], G)
        assert abs(fit - ref["score"]) <= 1e-3 * ref["score"]
    finally:
        m.close()
    G = guess(T, "0.8yaw")
    # the iteration cap: at transformation_epsilon 0.01 the uncapped run goes on for longer, so `it > max_iterations` ends these
    free = oracle(src, tgt, G, 0.1, 0.01)
    for cap in (1, 2):
        ref = oracle(src, tgt, G, 0.1, 0.01, max_iterations=cap)
        assert ref["iterations"] == cap + 2 < free["iterations"], (cap, ref["iterations"], free["iterations"])
        m = matcher(src, tgt, transformation_epsilon=0.01, max_iterations=cap)
        try:
            _, R = m.align(G)
            compare(f"max_iterations {cap}", R, m.get_fitness_score(), m.last_ndt_stats, ref)
        finally:
            m.close()
    # default options: the first Newton step is longer than step_size and is clamped to it
    ref = oracle(src, tgt, G)
    assert ref["trace"][0]["clamped"] and all(r["trials"] == 0 and not r["hessian_eval"] for r in ref["trace"]), ref["trace"]
    m = matcher(src, tgt)
    try:
        _, R = m.align(G)
        compare("default options, 0.8 m guess", R, m.get_fitness_score(), m.last_ndt_stats, ref)
    finally:
        m.close()
    report_worst()


# ---------------------------------------------------------------------------------------------------- mixed_batch
def case_mixed_batch():
    src, tgt, T = scene()
    ss, te = 0.1, 0.2
    names = ("0.3", "0.8", "x0.2", "x0.45", "x1.2")
    guesses = [guess(T, n) for n in names]
    refs = [oracle(src, tgt, G, ss, te) for G in guesses]
    loops = [tuple(r["trials"] for r in ref["trace"]) for ref in refs]
    print("oracle loop lengths:", dict(zip(names, loops)), "derivative calls:", [r["derivative_calls"] for r in refs])
    # Hessian and no-Hessian requests share launches (in round 2 a job whose first loop runs asks for a gradient while one whose
    # loop does not run asks for the next iteration's Hessian), and the jobs end in different rounds
    assert len(set(loops)) >= 4 and len({r["derivative_calls"] for r in refs}) >= 3
    assert any(l[0] == 0 for l in loops) and any(l[0] >= 2 for l in loops)
    single = []
    m1 = matcher(src, tgt, step_size=ss, transformation_epsilon=te)
    try:
        for G in guesses:
            _, R = m1.align(G)
            single.append((R, m1.get_fitness_score(), dict(m1.last_ndt_stats)))
    finally:
        m1.close()
    mb = matcher(src, tgt, slots=5, step_size=ss, transformation_epsilon=te)
    try:
        R, sc, st = mb.align_batch(5, guesses)
    finally:
        mb.close()
    for k, n in enumerate(names):
        assert R[k].tobytes() == single[k][0].tobytes() and sc[k] == single[k][1] and st[k] == single[k][2], (n, st[k], single[k][2])
        compare(f"slot {k} guess {n}", R[k], sc[k], st[k], refs[k])
    report_worst()


CASES = {"solve6_device": case_solve6_device, "mt_loop": case_mt_loop, "exits": case_exits, "mixed_batch": case_mixed_batch}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print("ok", sys.argv[1])
