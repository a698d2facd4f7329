"""The serial end of Ndt (staticmapping_amd/csrc/ndt_ctl_math.h: ndt_solve6 with its fallback svd_solve6, trial_value_mt,
update_interval_mt and the Newton / More-Thuente state machine behind ndt_ctl_result) on the CPU box: tests/cpp/test_ndt_ctl.cc,
compiled with g++ alone, answers the systems and runs of tests/ndt_ctl_cases.py and is compared with tests/ndt_ctl_ref.py.  The
same program built with -fsanitize=address,undefined answers the same cases.

The solve   per system |x - x_exact| <= max(8 x the C oracle's own error, 64 eps cond_kept |x_exact|); x_exact = the
            pseudo-inverse under JacobiSVD's rule (drop sigma <= 6 eps sigma_max) in 60-digit arithmetic.  A system is used only
            if no singular value is within a factor 4 of that threshold and the oracle is a usable yardstick; at most 5 % of the
            systems may be dropped that way (measured: none of 110).
The machine the requests (phase, pose, Hessian wanted or not) of the device's state machine and of oracle/ndt.py's newton_mt on
            the same scripted objective -- both are answered by one Python function, so both see the same bits: equal in kind
            and count, `it` and `deriv_calls` equal, every requested pose and the final one within 1e-12 relative.  Measured:
            the largest gap is 5.7e-14 (the elimination against numpy's SVD in the Newton step; the test prints it), the
            smallest decision margin of the reference 3.1e-3 against the required 1e-6.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import ndt_ctl_cases as cases  # noqa: E402
import ndt_ctl_ref as ref  # noqa: E402

BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
POSE_RTOL = 1e-12


def _hip_include() -> str:
    for cand in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if cand and os.path.exists(os.path.join(cand, "include", "hip", "hip_runtime.h")):
            return os.path.join(cand, "include")
    raise RuntimeError("HIP headers not found (ndt_ctl_math.h includes hip/hip_runtime.h for the function attributes)")


def _build(exe_name, extra):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, exe_name)
    src = os.path.join(ROOT, "tests", "cpp", "test_ndt_ctl.cc")
    csrc = os.path.join(ROOT, "staticmapping_amd", "csrc")
    deps = [src, os.path.join(csrc, "ndt_ctl_math.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", _hip_include(),
                               "-I", csrc] + extra + [src, "-o", exe])
    return exe


def _hex(v):
    return " ".join(float(x).hex() for x in np.asarray(v, dtype=np.float64).ravel())


def _floats(toks):
    return np.array([float.fromhex(t) for t in toks])


class Program:
    """The C++ program as a co-process: one line out, one line back."""

    def __init__(self, exe):
        self.p = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, bufsize=1)
        self.lines = []

    def send(self, line):
        self.p.stdin.write(line + "\n"); self.p.stdin.flush()

    def read(self):
        line = self.p.stdout.readline()
        assert line, "the program ended early: " + self.p.stderr.read()[-4000:]
        self.lines.append(line)
        return line.split()

    def close(self):
        self.send("quit")
        tail = self.p.stdout.read()
        err = self.p.stderr.read()
        rc = self.p.wait(timeout=60)
        assert rc == 0 and err == "", (rc, err[-4000:])              # (a sanitizer report that does not stop the program shows here)
        self.lines.append(tail)
        return "".join(self.lines)


def _answer_all(exe):
    """-> (solves {name: (x of ndt_solve6, x of svd_solve6)}, mts {name: (converged, trial, interval[6])},
           runs {name: dict(requests, it, deriv_calls, phase, p, sc, g, H)}, the program's whole output)."""
    prog = Program(exe)
    try:
        solves, mts, runs = {}, {}, {}
        for s in cases.systems():
            prog.send(f"solve {_hex(s['H'])} {_hex(s['b'])}")
            tok = prog.read()
            assert tok[0] == "solve" and tok[7] == "|" and tok[8] == "svd"
            solves[s["name"]] = (_floats(tok[1:7]), _floats(tok[9:15]))
        for name, t in cases.mt_tuples():
            prog.send(f"mt {_hex(t)}")
            tok = prog.read()
            assert tok[0] == "mt"
            mts[name] = (int(tok[1]), float.fromhex(tok[2]), _floats(tok[3:9]))
        for c in cases.runs():
            prog.send(f"run {_hex([c['step_size'], c['trans_eps'], c['max_iterations']])} {_hex(c['p0'])}")
            requests = []
            while True:
                tok = prog.read()
                if tok[0] == "end":
                    v = _floats(tok[4:])
                    runs[c["name"]] = dict(requests=requests, it=int(tok[1]), deriv_calls=int(tok[2]), phase=int(tok[3]), p=v[:6], sc=v[6], g=v[7:13],
                                           H=v[13:49].reshape(6, 6))
                    break
                assert tok[0] == "req" and len(requests) < 2000, tok[0]
                phase, hess, x = int(tok[1]), int(tok[2]), _floats(tok[3:9])
                requests.append((phase, hess, x))
                sc, g, H = c["objective"](x, len(requests))
                if phase == ref.PHASE["hess"]:
                    # the device's kernel hands back a score and a gradient with the closing Hessian; the machine must not take them
                    sc, g = sc + 1.0, 2.0 * g + 1.0
                if not hess:
                    H = np.full((6, 6), 12345.0)                     # no Hessian was asked for: whatever the columns hold is not to be used
                prog.send(f"val {float(sc).hex()} {_hex(g)} {_hex(H)}")
        return solves, mts, runs, prog.close()
    finally:
        if prog.p.poll() is None:
            prog.p.kill()


@functools.lru_cache(maxsize=None)
def _answers():
    return _answer_all(_build("test_ndt_ctl", []))


@functools.lru_cache(maxsize=None)
def _reference_runs():
    return {c["name"]: ref.run_reference(c) for c in cases.runs()}


# ---------------------------------------------------------------------------------------------- the solve
def test_at_most_five_percent_of_the_systems_are_dropped():
    rows = ref.judged_systems()
    dropped = [r["name"] for r in rows if not r["admissible"]]
    print(f"{len(dropped)} of {len(rows)} systems dropped: {dropped}")
    assert len(rows) >= 100 and len(dropped) <= cases.MAX_DROPPED_SHARE * len(rows)
    fam = {r["family"] for r in rows if r["admissible"]}
    assert fam == {"well", "cond", "rank", "rounding", "hidden"}     # no family is dropped whole
    for want in ("cond1e+10", "cond1e+09", "cond1e+11", "rank0", "rank3", "smin1e-17", "smin1e-14", "hidden"):
        assert any(r["name"].startswith(want) and r["admissible"] for r in rows), want


def test_the_hidden_family_is_what_it_claims():
    """Pivots of the elimination within ten decades (the switch of ndt_solve6's first version would not have left the fast path)
    while the exact smallest singular value is below JacobiSVD's threshold: rank 5 by the reference's rule."""
    rows = [r for r in ref.judged_systems() if r["family"] == "hidden"]
    assert len(rows) == 2 * len(cases.HIDDEN_SEEDS)
    for r in rows:
        pmin, pmax = cases.device_rule_pivots(r["H"])
        assert pmin > 1e-10 * pmax and r["kept"] == 5 and r["sigma"][-1] < 6 * ref.EPS * r["sigma"][0] / 4, (r["name"], pmin / pmax, r["sigma"])


def _check_solve(which):
    solves = _answers()[0]
    bad, worst = [], {}
    for r in ref.judged_systems():
        if not r["admissible"]:
            continue
        x = solves[r["name"]][which]
        err = ref.error(x, r["x"])
        print(f"{r['name']:32s} kept {r['kept']} cond_kept {r['cond_kept']:.2e} err {err:.3e} tol {r['tol']:.3e} (oracle {r['oracle_err']:.3e})")
        fam = r["family"]
        if r["tol"] > 0 and err / r["tol"] > worst.get(fam, (0, 0, 0))[0]:
            worst[fam] = (err / r["tol"], err, r["tol"])
        if not err <= r["tol"]:
            bad.append((r["name"], err, r["tol"]))
    print("worst error / tolerance per family:", {k: f"{v[0]:.3f} ({v[1]:.2e} / {v[2]:.2e})" for k, v in worst.items()})
    assert not bad, bad


def test_ndt_solve6_against_the_exact_pseudo_inverse():
    _check_solve(0)


def test_svd_solve6_alone_against_the_exact_pseudo_inverse():
    """The fallback on every system, the well conditioned ones included: where the two paths meet they must both be right."""
    _check_solve(1)


# ---------------------------------------------------------------------------------------------- the helpers
def test_trial_value_and_update_interval_case_by_case():
    from oracle import ndt as ondt
    mts = _answers()[1]
    book = ondt._Book()
    for name, t in cases.mt_tuples():
        want_a = float(ondt._trial_value_b(book, *t))
        *want_iv, want_conv = ondt._update_interval_b(book, *t)
        conv, a, iv = mts[name]
        assert conv == int(want_conv), (name, conv, want_conv)
        assert np.array_equal(iv, np.array(want_iv, dtype=np.float64)), (name, iv, want_iv)       # copies of the inputs: exact
        assert (np.isnan(a) and np.isnan(want_a)) or abs(a - want_a) <= POSE_RTOL * abs(want_a), (name, a, want_a)
    print(book.counts)
    for k in ("trial:1", "trial:2", "trial:3", "trial:4", "update:1", "update:2", "update:3", "update:4"):
        assert book.counts.get(k, 0) >= 1, (k, book.counts)


# ---------------------------------------------------------------------------------------------- the machine
REQUIRED_BRANCHES = ("trial:1", "trial:2", "trial:3", "update:1", "update:3", "update:4", "mt:closed", "mt:cap", "mt:wolfe",
                     "loop0_no_hess", "loop>=1_with_hess", "d_phi_0>0", "d_phi_0==0", "exit:dp_norm_zero", "exit:dp_norm_nan",
                     "exit:max_iterations", "exit:trans_eps", "first_trial_clamped")


def test_reference_runs_reach_every_branch_with_a_margin():
    """Coverage is asserted on the reference side.  update_interval_mt's second outcome and trial_value_mt's fourth case are not
    in the list: the loop is open only when step_size <= trans_eps / 2, and then every trial value is clamped to trans_eps / 2 --
    the same point again.  The first call sees a_l = 0, f_l = 0 and a trial that failed the exit test (cases 1 or 2), the later
    ones a trial equal to an interval end (cases 1 or 3; outcomes 1, 3, 4).  No finite run reaches the other two; a NaN would,
    but a comparison with a NaN clears no margin.  test_trial_value_and_update_interval_case_by_case calls the helpers
    directly instead and takes all eight."""
    total, worst = {}, (1.0, None, None)
    for name, out in _reference_runs().items():
        b = out["book"]
        for k, v in b.counts.items():
            total[k] = total.get(k, 0) + v
        for what, m in b.margins:
            if m < worst[0]:
                worst = (m, name, what)
        assert all(m >= cases.MARGIN for _, m in b.margins), (name, min(b.margins, key=lambda t: t[1]))
    print("branch counts:", sorted(total.items()))
    print("smallest decision margin: %.3e in %s at %s" % worst)
    for k in REQUIRED_BRANCHES:
        assert total.get(k, 0) >= 1, (k, total)
    refs = _reference_runs()
    assert any(o["book"].counts.get("loop>=1_with_hess") and o["book"].counts.get("mt:closed") for o in refs.values())
    assert refs["all_zero"]["iterations"] == 0 and refs["all_zero"]["derivative_calls"] == 1
    assert refs["d_phi_0_zero"]["derivative_calls"] == 1 and refs["d_phi_0_zero"]["iterations"] == 2


def test_requests_equal_the_reference_restatement():
    runs = _answers()[2]
    worst = 0.0
    for c in cases.runs():
        got, want = runs[c["name"]], _reference_runs()[c["name"]]
        assert [(r[0], r[1]) for r in got["requests"]] == [(r[0], r[1]) for r in want["requests"]], c["name"]
        assert got["it"] == want["iterations"] and got["deriv_calls"] == want["derivative_calls"], (c["name"], got["it"], got["deriv_calls"])
        for k, (a, b) in enumerate(zip(got["requests"], want["requests"])):
            if np.isnan(b[2]).any():
                assert np.array_equal(np.isnan(a[2]), np.isnan(b[2])), (c["name"], k)
                continue
            gap = float(np.linalg.norm(a[2] - b[2]) / max(np.linalg.norm(b[2]), 1e-300))
            worst = max(worst, gap)
            assert gap <= POSE_RTOL, (c["name"], k, gap)
        gap = float(np.linalg.norm(got["p"] - want["p"]) / max(np.linalg.norm(want["p"]), 1e-300))
        worst = max(worst, gap)
        assert gap <= POSE_RTOL, (c["name"], "final p", gap)
    print(f"largest relative gap of a requested or final pose: {worst:.3e} (bound {POSE_RTOL:g})")


def test_closing_hessian_replaces_the_hessian_alone():
    """After a loop that ran, the Hessian-only evaluation: the machine's score and gradient stay the loop's last (the program is
    handed a different score and gradient with that evaluation), its Hessian is the new one."""
    runs = _answers()[2]
    checked = 0
    for c in cases.runs():
        got = runs[c["name"]]
        req = got["requests"]
        if not req or req[-1][0] != ref.PHASE["hess"]:
            continue
        last_mt = max(k for k, r in enumerate(req) if r[0] == ref.PHASE["mt"])
        sc, g, _ = c["objective"](req[last_mt][2], last_mt + 1)
        _, _, H = c["objective"](req[-1][2], len(req))
        if np.isnan(g).any():
            continue
        assert got["sc"] == sc and np.array_equal(got["g"], g) and np.array_equal(got["H"], H), c["name"]
        assert np.array_equal(req[-1][2], req[last_mt][2]), c["name"]          # the same pose once more
        checked += 1
    assert checked >= 3


# ---------------------------------------------------------------------------------------------- the sanitizer build
def test_sanitizer_build_answers_the_same_cases():
    exe = _build("test_ndt_ctl_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert _answer_all(exe)[3] == _answers()[3]
