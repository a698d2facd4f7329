"""The arithmetic of IcpFast's iteration tail (staticmapping_amd/csrc/icp_tail_math.h: solve6 and its invertibility rule, the
angle-axis step, the motion-potential bound, Eigen's quaternion of a rotation, angularDistance, CheckConvergence over the ring) on
the CPU box, branch by branch: tests/cpp/test_icp_tail.cc compiled with g++ alone answers the cases written here, and the answers
are compared with the multi-precision reference (tests/icp_tail_ref.py).  The same program built with
-fsanitize=address,undefined answers the same cases.

Measured here (and recorded in DESIGN.md, IcpFast section): the decision band B = 1.45 -- 4 x the 0.362 relative error of the
smallest pivot of oracle/icp_fast.py's f64 QR --, i.e. solve6 must take the reference rule's branch wherever the exact smallest
pivot is not within [1 / 2.45, 2.45] of eps * 6 * the largest."""
import functools
import os
import subprocess
import sys

import mpmath as mp
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import icp_tail_cases as cases  # noqa: E402
import icp_tail_ref as ref  # noqa: E402

EPS = cases.EPS
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
CHOLESKY_FAST, CHOLESKY_QR, MIN_NORM = 0, 1, 2


def _hip_include() -> str:
    for cand in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if cand and os.path.exists(os.path.join(cand, "include", "hip", "hip_runtime.h")):
            return os.path.join(cand, "include")
    raise RuntimeError("HIP headers not found (icp_tail_math.h includes hip/hip_runtime.h for the function attributes)")


def _build(exe_name, extra):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, exe_name)
    src = os.path.join(ROOT, "tests", "cpp", "test_icp_tail.cc")
    csrc = os.path.join(ROOT, "staticmapping_amd", "csrc")
    deps = [src, os.path.join(csrc, "icp_tail_math.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", _hip_include(),
                               "-I", csrc] + extra + [src, "-o", exe])
    return exe


def _hex(v):
    return " ".join(float(x).hex() for x in np.asarray(v, dtype=np.float64).ravel())


def _rows12(T):
    return np.asarray(T, dtype=np.float64)[:3, :4]


# ---------------------------------------------------------------------------------------------- the cases, in order
def _quat_pairs():
    rng = np.random.default_rng(3)
    out = []
    for i in range(6):
        q = rng.standard_normal(4); q /= np.linalg.norm(q)
        out.append(("equal", q, q.copy()))
        out.append(("antipodal", q, -q))
        ax = rng.standard_normal(3); ax /= np.linalg.norm(ax)
        h = 0.5e-9
        d = np.array([np.cos(h), *(np.sin(h) * ax)])                # q * d: 1e-9 rad further
        w1, v1, w2, v2 = q[0], q[1:], d[0], d[1:]
        q2 = np.array([w1 * w2 - v1 @ v2, *(w1 * v2 + w2 * v1 + np.cross(v1, v2))])
        out.append(("1e-9", q, q2))
        out.append(("1e-9 antipodal", q, -q2))
    return out


def _angle_axis_cases():
    u = np.array([1.0, -2.0, 0.5]); u /= np.linalg.norm(u)
    t = np.array([0.25, -0.5, 0.125])
    nan = float("nan")
    return [("zero_rotation", np.concatenate([np.zeros(3), t])),
            ("underflow", np.concatenate([u * 1e-170, t])),
            ("1e-8", np.concatenate([u * 1e-8, t])),
            ("3", np.concatenate([u * 3.0, t])),
            ("nan_translation", np.concatenate([u * 0.1, [t[0], nan, t[2]]])),
            ("nan_rotation", np.concatenate([[nan, 0.0, 0.0], t]))]


def _ring_cases():
    """(name, early_exit, [T 4x4 ...]): histories of 1..7 entries (the identity the Align starts from is the first), and steps
    whose last-four means sit either side of 1e-3 rad and 1e-2 m."""
    out = []
    tiny = [cases.make_pose((1e-5 * k, 0, 0), (1e-4 * k, 0, 0)) for k in range(1, 8)]
    for n in range(0, 7):
        out.append((f"tiny:{n + 1}", 1, tiny[:n]))
    out.append(("tiny_no_early_exit", 0, tiny[:6]))

    def walk(rot_step, trans_step, n, first_rot=None, first_trans=None):
        Ts, a, t = [], 0.0, 0.0
        for k in range(n):
            a += first_rot if (k == 0 and first_rot is not None) else rot_step
            t += first_trans if (k == 0 and first_trans is not None) else trans_step
            Ts.append(cases.make_pose((0, 0, a), (0, t, 0)))
        return Ts
    for nm, rs, ts in (("rot_below", 1e-3 * (1 - 1e-5), 1e-3), ("rot_above", 1e-3 * (1 + 1e-5), 1e-3),
                       ("trans_below", 1e-5, 1e-2 * (1 - 1e-5)), ("trans_above", 1e-5, 1e-2 * (1 + 1e-5))):
        out.append((nm, 1, walk(rs, ts, 4)))
    # the ring has shifted: a large FIRST step must have left the window by the sixth entry -- and must still be in it at the fifth
    out.append(("shift_rot", 1, walk(1e-4, 1e-4, 6, first_rot=0.5)))
    out.append(("shift_trans", 1, walk(1e-4, 1e-4, 6, first_trans=5.0)))
    # ... and a large LAST step counts
    Ts = walk(1e-4, 1e-4, 5); Ts.append(cases.make_pose((0, 0, 0.5), (0, 6e-4, 0)))
    out.append(("late_rot", 1, Ts))
    return out


@functools.lru_cache(maxsize=None)
def _cases_text():
    L = ref.ladder_reference()
    lines, index = [], []
    for r in L["rows"]:
        lines.append(f"solve {_hex(r['A'])} {_hex(r['b'])}"); index.append(("solve", r["name"]))
    for nm, A, b in cases.special_matrices():
        lines.append(f"solve {_hex(A)} {_hex(b)}"); index.append(("special", nm))
    for nm, R in cases.rotations():
        lines.append(f"quat {_hex(R)}"); index.append(("quat", nm))
    for nm, a, c in _quat_pairs():
        lines.append(f"qdist {_hex(a)} {_hex(c)}"); index.append(("qdist", nm))
    for nm, x in _angle_axis_cases():
        lines.append(f"aa {_hex(x)}"); index.append(("aa", nm))
    for i, (M0, M1) in enumerate(cases.potential_pairs()):
        lines.append(f"pot {_hex(M1)} {_hex(M0)}"); index.append(("pot", i))
    for nm, early, Ts in _ring_cases():
        lines.append(f"ring {early} {len(Ts)} " + " ".join(_hex(_rows12(T)) for T in Ts)); index.append(("ring", nm))
    return "\n".join(lines) + "\n", index


def _run(exe):
    text, index = _cases_text()
    path = os.path.join(BUILD, "icp_tail_cases.txt")
    with open(path, "w") as fh:
        fh.write(text)
    out = subprocess.run([exe, path], text=True, capture_output=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stderr == "", out.stderr[-4000:]                      # a sanitizer report that does not stop the program
    return out.stdout, index


@functools.lru_cache(maxsize=None)
def _answers():
    stdout, index = _run(_build("test_icp_tail", []))
    lines = stdout.strip().split("\n")
    assert lines[-1] == f"done {len(index)}", lines[-1]
    res, at = {}, 0
    fl = lambda toks: np.array([float.fromhex(t) for t in toks])
    for kind, nm in index:
        tok = lines[at].split(); at += 1
        if kind in ("solve", "special"):
            assert tok[0] == "solve"
            res[(kind, nm)] = (int(tok[1]), fl(tok[2:]))
        elif kind == "ring":
            n = int(tok[1])
            pushes = [tuple(int(v) for v in lines[at + k].split()[1:]) for k in range(n)]; at += n
            nh = pushes[-1][1] if pushes else 1
            entries = [fl(lines[at + k].split()[1:]) for k in range(nh)]; at += nh
            res[(kind, nm)] = (pushes, entries)
        else:
            assert tok[0] == kind, (tok[0], kind)
            res[(kind, nm)] = fl(tok[1:])
    return res, stdout


# ---------------------------------------------------------------------------------------------- the 6x6 solve
def test_ladder_keeps_four_rungs_on_each_side_of_the_band():
    L = ref.ladder_reference()
    print(f"band B = {L['band']:.4f} (largest relative pivot error of the oracle's f64 QR {L['worst_pivot_error']:.4f})")
    assert 0.0 < L["band"] < 9.0                                     # a band of a decade would decide nothing
    full = [r for r in L["rows"] if r["name"].startswith("full:")]
    above = [r for r in full if r["ratio"] > 1 + L["band"]]
    below = [r for r in full if r["ratio"] < 1 / (1 + L["band"])]
    assert len(above) >= 4 and len(below) >= 4, (len(above), len(below))
    # ... and close ones: four within two decades of the threshold on either side
    assert sum(r["ratio"] < 100 for r in above) >= 4 and sum(r["ratio"] > 0.01 for r in below) >= 4


def test_solve6_takes_the_reference_rules_branch_outside_the_band():
    L = ref.ladder_reference()
    ans, _ = _answers()
    wrong = []
    for r in L["rows"]:
        br, _ = ans[("solve", r["name"])]
        print(f"{r['name']:30s} rank {r['rank']} ratio {r['ratio']:.3e} in_band {r['in_band']} branch {br}")
        if r["in_band"]:
            continue
        if (br != MIN_NORM) != (r["rank"] == 6):
            wrong.append((r["name"], r["rank"], r["ratio"], br))
    assert not wrong, wrong


def test_fast_accept_never_contradicts_the_reference_rule():
    """A matrix the unrolled Cholesky accepts on its own (every pivot above 1e-13 dmax) is one the reference rule calls
    invertible, band or no band; and the ladder does reach all three branches."""
    L = ref.ladder_reference()
    ans, _ = _answers()
    seen = set()
    for r in L["rows"]:
        br, _ = ans[("solve", r["name"])]
        seen.add(br)
        if br == CHOLESKY_FAST:
            assert r["rank"] == 6 and r["ratio"] > 10.0, (r["name"], r["rank"], r["ratio"])
    assert seen == {CHOLESKY_FAST, CHOLESKY_QR, MIN_NORM}, seen
    # the window the pivot threshold alone used to hand to the pseudo-inverse: Cholesky by the rule
    window = [r for r in L["rows"] if not r["in_band"] and r["rank"] == 6 and r["ratio"] < 75.0]
    assert len(window) >= 4
    for r in window:
        assert ans[("solve", r["name"])][0] != MIN_NORM, (r["name"], r["ratio"])


def test_solve6_solution_against_the_exact_one():
    L = ref.ladder_reference()
    ans, _ = _answers()
    bad, checked = [], 0
    for r in L["rows"]:
        br, x = ans[("solve", r["name"])]
        assert np.isfinite(x).all(), (r["name"], x)
        A, b = r["A"], r["b"]
        if r["in_band"]:                                             # backward stability alone
            res = np.linalg.norm(A @ x - b)
            bound = 1e-10 * (np.linalg.norm(A, 2) * np.linalg.norm(x) + np.linalg.norm(b))
            print(f"{r['name']:30s} in band: residual {res:.3e} bound {bound:.3e}")
            assert res <= bound, (r["name"], res, bound)
            continue
        if r["rank"] < 6 and not r["gap"] >= 1e6:
            continue
        err = float(ref.norm([mp.mpf(float(a)) - v for a, v in zip(x, r["x"])]))
        print(f"{r['name']:30s} rank {r['rank']} err {err:.3e} tol {r['tol']:.3e} (oracle {r['oracle_err']:.3e})")
        checked += 1
        if not err <= r["tol"]:
            bad.append((r["name"], err, r["tol"]))
    assert checked >= 80
    assert not bad, bad


def test_solve6_on_non_finite_and_zero_matrices():
    """x is what the reference path gives -- rank 0, the zero vector, which the angle-axis step turns into the identity -- and
    never part finite, part NaN."""
    ans, _ = _answers()
    for nm, A, b in cases.special_matrices():
        br, x = ans[("special", nm)]
        print(nm, br, x)
        assert np.isfinite(x).all() or np.isnan(x).all(), (nm, x)
        if nm != "nan_rhs":
            assert br == MIN_NORM and (x == 0).all(), (nm, br, x)
        else:
            assert np.isnan(x).all(), (nm, x)                        # a full-rank A: Cholesky carries the NaN to every entry


# ---------------------------------------------------------------------------------------------- quaternions
def test_quat_from_rot_every_branch_within_16_eps():
    ans, _ = _answers()
    branches = set()
    for nm, R in cases.rotations():
        br, q = ref.quat_from_rot(ref.M(R))
        branches.add(br)
        got = ans[("quat", nm)]
        err = max(abs(float(mp.mpf(float(g)) - e)) for g, e in zip(got, q))
        print(f"{nm:18s} branch {br} err {err / EPS:.2f} eps")
        assert err <= 16 * EPS, (nm, br, got, [float(v) for v in q])
    assert branches == {0, 1, 2, 3}


def test_quat_angular_distance_equal_antipodal_and_close_pairs():
    ans, _ = _answers()
    for nm, a, c in _quat_pairs():
        got = float(ans[("qdist", nm)][0])
        want = float(ref.angular_distance(ref.M(a), ref.M(c)))
        print(f"{nm:16s} got {got:.6e} exact {want:.6e}")
        # q and -q are one rotation: the distance of an antipodal pair is that of the pair itself, not 2 pi minus it.
        # The vector part of a * conj(c) is four differences of products of size <= 1, each rounded twice: 16 eps covers its
        # absolute error, and the angle is twice its length.  `want` is exact on the same f64 quaternions.
        assert got >= 0 and abs(got - want) <= 32 * EPS, (nm, got, want)
        if nm.startswith("1e-9"):
            assert abs(want - 1e-9) < 32 * EPS, (nm, want)             # (the pair as rounded to f64 is 1e-9 rad apart)
        else:
            assert got == 0.0, (nm, got)                             # the products of an equal pair cancel exactly


# ---------------------------------------------------------------------------------------------- angle-axis
def test_angle_axis_step_and_its_nan_guard():
    ans, _ = _answers()
    for nm, x in _angle_axis_cases():
        dT = ans[("aa", nm)].reshape(3, 4)
        print(nm, dT.tolist())
        if nm in ("zero_rotation", "underflow", "nan_translation", "nan_rotation"):
            assert (dT[:, :3] == np.eye(3)).all(), (nm, dT)           # the rotation block is reset, exactly
        else:
            R = ref.angle_axis(ref.M(x))
            err = max(abs(float(mp.mpf(float(dT[i, j])) - R[i][j])) for i in range(3) for j in range(3))
            assert err <= 8 * EPS, (nm, err / EPS)
        t = dT[:, 3]
        assert all((a == b) or (np.isnan(a) and np.isnan(b)) for a, b in zip(t, x[3:])), (nm, t)   # the translation is kept


# ---------------------------------------------------------------------------------------------- the potential bound
def test_step_a_bounds_the_spectral_norm_from_above():
    ans, _ = _answers()
    pairs = cases.potential_pairs()
    assert len(pairs) == 2000
    worst_lo, worst_hi, angles = np.inf, 0.0, []
    for i, (M0, M1) in enumerate(pairs):
        sa, sb = (float(v) for v in ans[("pot", i)])
        D = [[mp.mpf(float(M1[r, c])) - mp.mpf(float(M0[r, c])) for c in range(3)] for r in range(3)]
        smax = ref.sigma_max3(D)
        fro = mp.sqrt(mp.fsum(v * v for r in D for v in r))
        dt = ref.norm([mp.mpf(float(M1[r, 3])) - mp.mpf(float(M0[r, 3])) for r in range(3)])
        angles.append(float(smax))
        assert smax > 0
        worst_lo = min(worst_lo, float(mp.mpf(sa) / smax)); worst_hi = max(worst_hi, float(mp.mpf(sa) / fro))
        assert smax <= mp.mpf(sa), (i, float(smax), sa)              # never an under-estimate: certificates rely on it
        assert mp.mpf(sa) <= fro * (1 + mp.mpf("1e-8")), (i, sa, float(fro))
        assert dt <= mp.mpf(sb), (i, float(dt), sb)
    print(f"step_a / sigma_max >= {worst_lo:.12f}, step_a / frobenius <= {worst_hi:.12f}, sigma_max from {min(angles):.2e} to {max(angles):.2e}")
    assert min(angles) < 1e-11 and max(angles) > 1.9


# ---------------------------------------------------------------------------------------------- convergence
def _ring_reference(Ts, early):
    quats, trans, flags = [[mp.mpf(1), mp.mpf(0), mp.mpf(0), mp.mpf(0)]], [[mp.mpf(0)] * 3], []
    for T in Ts:
        quats.append(ref.quat_from_rot(ref.M(T[:3, :3]))[1]); trans.append(ref.M(T[:3, 3]))
        conv, rd, td = ref.check_convergence(quats, trans)
        if rd is not None:                                           # rounding must not decide: 1e-6 away from both thresholds
            assert abs(float(rd) / 1e-3 - 1) > 1e-6 and abs(float(td) / 1e-2 - 1) > 1e-6
        flags.append(bool(conv and early))
    return flags, quats, trans


def test_convergence_over_the_history_ring():
    ans, _ = _answers()
    seen = {}
    for nm, early, Ts in _ring_cases():
        pushes, entries = ans[("ring", nm)]
        flags, quats, trans = _ring_reference(Ts, early)
        print(nm, pushes, flags)
        assert [bool(p[0]) for p in pushes] == flags, (nm, pushes, flags)
        assert [p[1] for p in pushes] == [min(k + 2, 5) for k in range(len(Ts))], (nm, pushes)
        for k, p in enumerate(pushes):
            if k + 2 < 5:
                assert not p[0], (nm, k)                             # nothing converges before the fifth entry
        # what the ring holds is the LATEST entries, oldest first
        keep = min(len(quats), 5)
        for e, q, t in zip(entries, quats[-keep:], trans[-keep:]):
            assert max(abs(float(mp.mpf(float(g)) - w)) for g, w in zip(e[:4], q)) <= 16 * EPS, nm
            assert all(float(w) == g for g, w in zip(e[4:], t)), nm
        seen[nm] = flags
    assert seen["tiny:5"] == [False, False, False, True] and seen["tiny:7"][-3:] == [True, True, True]
    assert not any(seen["tiny_no_early_exit"])
    assert seen["rot_below"][-1] and not seen["rot_above"][-1] and seen["trans_below"][-1] and not seen["trans_above"][-1]
    assert seen["shift_rot"][3:] == [False, True, True] and seen["shift_trans"][3:] == [False, True, True]
    assert seen["late_rot"][3:] == [True, True, False]


# ---------------------------------------------------------------------------------------------- the sanitizer build
def test_sanitizer_build_answers_the_same_cases():
    exe = _build("test_icp_tail_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    stdout, _ = _run(exe)
    assert stdout == _answers()[1]
