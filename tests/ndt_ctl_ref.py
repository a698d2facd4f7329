"""What the serial end of Ndt (staticmapping_amd/csrc/ndt_ctl_math.h) is measured against.

The solve: Eigen::JacobiSVD(H).solve(b) (pclomp/ndt_omp_impl.hpp:127-129) is the pseudo-inverse applied to b with the singular
values at or below 6 eps sigma_max dropped.  pinv_reference forms it in mpmath at 60 digits (the tool of tests/icp_tail_ref.py):
the decomposition, the decision which values count and the product are all taken on exact values.  Nothing here is tuned to the
code under test.

The state machine: oracle/ndt.py's newton_mt -- the restatement of ndt_omp_impl.hpp:81-171, 633-916 -- run on the scripted
objectives of tests/ndt_ctl_cases.py with a book that counts every branch and records how far every comparison was from flipping.
"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

mp.mp.dps = 60
EPS = 2.0 ** -52
PHASE = {"init": 0, "trial": 1, "mt": 2, "hess": 3}


def pinv_reference(H, b):
    """-> dict(x [6 mpf], sigma [6 floats, descending], kept, cond_kept, near): `near` = some singular value lies within a factor 4
    of the threshold 6 eps sigma_max, so that which side is right is not defined for an f64 code."""
    Hm = mp.matrix([[mp.mpf(float(v)) for v in r] for r in np.asarray(H, dtype=np.float64).reshape(6, 6)])
    bm = [mp.mpf(float(v)) for v in np.asarray(b, dtype=np.float64)]
    x = [mp.mpf(0)] * 6
    if max(abs(v) for v in Hm) == 0:
        return dict(x=x, sigma=[0.0] * 6, kept=0, cond_kept=1.0, near=False)
    U, S, V = mp.svd_r(Hm)
    sig = [S[k] for k in range(6)]
    thr = mp.mpf(6) * mp.mpf(EPS) * max(sig)
    kept = [k for k in range(6) if sig[k] > thr]
    near = any(thr / 4 <= s <= thr * 4 for s in sig)
    for k in kept:
        c = mp.fsum(U[i, k] * bm[i] for i in range(6)) / sig[k]
        for i in range(6):
            x[i] += c * V[k, i]
    cond = float(max(sig) / min(sig[k] for k in kept)) if kept else 1.0
    return dict(x=x, sigma=sorted((float(s) for s in sig), reverse=True), kept=len(kept), cond_kept=cond, near=near)


def norm(v):
    return mp.sqrt(mp.fsum(a * a for a in v))


def error(x64, x_exact):
    """|x64 - x_exact| with the f64 vector entering exactly (inf if it is not finite)."""
    if not np.isfinite(np.asarray(x64, dtype=np.float64)).all():
        return float("inf")
    return float(norm([mp.mpf(float(a)) - e for a, e in zip(x64, x_exact)]))


_JUDGED = {}


def judged_systems():
    """Every system of ndt_ctl_cases.systems() with its exact answer, computed once per process and shared (treat as read-only):
    rows of dict(name, family, H, b, x [mpf], xnorm, sigma, kept, cond_kept, near, oracle_x, oracle_err, tol, admissible).
      tol = max(8 x the error of the C oracle's own svd_solve6 against the exact answer, 64 eps cond_kept |x|)
    -- the margin convention of test_icp_tail_gpu.py.  A system is admissible when no singular value is within a factor 4 of
    the threshold and the oracle itself is a usable yardstick: its error is finite and 8 x it stays below |x| (past that the
    tolerance would admit any answer of the right size, and the system would check nothing)."""
    if _JUDGED:
        return _JUDGED["rows"]
    import ndt_ctl_cases as cases
    from oracle import cref
    rows = []
    for s in cases.systems():
        r = dict(s)
        r.update(pinv_reference(s["H"], s["b"]))
        r["xnorm"] = float(norm(r["x"]))
        r["oracle_x"] = cref.ndt_svd_solve6(s["H"], s["b"])
        r["oracle_err"] = error(r["oracle_x"], r["x"])
        r["tol"] = max(8.0 * r["oracle_err"], 64.0 * EPS * r["cond_kept"] * r["xnorm"])
        usable = np.isfinite(r["oracle_err"]) and (8.0 * r["oracle_err"] < r["xnorm"] or r["oracle_err"] == 0.0)
        r["admissible"] = bool(not r["near"] and usable)
        rows.append(r)
    _JUDGED["rows"] = rows
    return rows


def run_reference(case):
    """newton_mt on a case of ndt_ctl_cases.runs() -> dict(requests [(phase, compute_hessian, eval_p)], iterations,
    derivative_calls, p, score, book)."""
    from oracle import ndt as ondt
    requests = []
    f = case["objective"]

    def objective(kind, x, hess):
        requests.append((PHASE[kind], int(bool(hess)), x.copy()))
        sc, g, H = f(x, len(requests))
        return sc, g, (H if hess else None)

    book = ondt._Book()
    out = ondt.newton_mt(objective, case["p0"], case["step_size"], case["trans_eps"], case["max_iterations"], book=book)
    out.update(requests=requests, book=book)
    return out
