"""The inputs of the serial-end tests of Ndt (tests/test_ndt_ctl_cpp.py on the host, the solve6_device case of
tests/test_ndt_ctl_gpu.py on the device): 6x6 systems for the Newton solve and scripted 6-D objectives for the Newton /
More-Thuente state machine.  Every seed is fixed; nothing here looks at the code under test.

MARGIN = 1e-6: every comparison the reference restatement takes on a run of runs() is at least this far (relative to the larger
of the two compared quantities) from flipping, or is a comparison of two copies of one number (a trial value clamped to a bound
against that bound, a gradient that is exactly zero).  It is a condition on the inputs, asserted by the test: a case that fails
it is replaced, not excused.
"""
import functools

import mpmath as mp
import numpy as np

EPS = 2.0 ** -52
MARGIN = 1e-6
MAX_DROPPED_SHARE = 0.05


# ------------------------------------------------------------------------------------------------------ systems
def _orth(rng):
    Q, R = np.linalg.qr(rng.standard_normal((6, 6)))
    return Q * np.sign(np.diag(R))


def _compose(Q, s):
    """Q diag(s) Q^T formed in 60-digit arithmetic and rounded once (an f64 product would add its own 1e-16 to every value)."""
    with mp.workdps(60):
        Qm = mp.matrix(Q.tolist())
        H = Qm * mp.diag([mp.mpf(float(v)) for v in s]) * Qm.T
        H = (H + H.T) / 2
        return np.array([[float(H[i, j]) for j in range(6)] for i in range(6)])


def _dyadic_orth(k):
    """An orthogonal matrix with dyadic entries (products of Householder reflections I - v v^T / 2, v of four +-1, and a
    permutation): Q diag(s) Q^T with dyadic s is then exact in f64, and so is its rank."""
    vs = [np.array([1, 1, 1, 1, 0, 0.]), np.array([0, 1, -1, 0, 1, 1.]), np.array([1, 0, 0, -1, 1, -1.]), np.array([1, -1, 0, 0, -1, 1.])]
    Q = np.eye(6)[np.roll(np.arange(6), k)]
    for v in (vs[k % 4], vs[(k + 1) % 4]):
        Q = Q @ (np.eye(6) - np.outer(v, v) / 2)
    assert np.array_equal(Q @ Q.T, np.eye(6))
    return Q


def device_rule_pivots(H):
    """The pivots of Gaussian elimination with partial pivoting on H in f64 (the order ndt_solve6 eliminates in) -> (min, max)."""
    A = np.array(H, dtype=np.float64)
    piv = []
    for c in range(6):
        r = c + int(np.argmax(np.abs(A[c:, c])))
        if A[r, c] == 0:
            return 0.0, max(piv + [0.0])
        A[[c, r]] = A[[r, c]]
        piv.append(abs(A[c, c]))
        for k in range(c + 1, 6):
            A[k, c + 1:] -= (A[k, c] / A[c, c]) * A[c, c + 1:]
    return min(piv), max(piv)


def hidden_deficiency(seed):
    """A symmetric matrix whose elimination pivots stay within ten decades although one singular value lies below JacobiSVD's
    threshold: +-scale D (I - (1 - s6) v v^T) D with D = diag(+-1), s6 = 1e-17 and the near-null vector v = (v1..v5, e) / |.|
    graded so that its last component e is ~1e-9.  The last two pivots are then ~e and ~s6 / e: neither is small against the
    first, their PRODUCT is.  (Kahan's matrix makes the same point for column-pivoted QR.)"""
    rng = np.random.default_rng(seed)
    v = np.concatenate([rng.uniform(0.35, 0.55, 5), [10.0 ** rng.uniform(-9.0, -8.3)]])
    v /= np.linalg.norm(v)
    d = rng.choice([-1.0, 1.0], 6)
    sign = rng.choice([-1.0, 1.0])
    scale = 2.0 ** rng.integers(-3, 4)
    with mp.workdps(60):
        vm = mp.matrix([mp.mpf(float(a)) for a in v])
        n2 = mp.fsum(a * a for a in vm)
        H = mp.eye(6) - (1 - mp.mpf("1e-17")) * (vm * vm.T) / n2
        out = np.array([[float(H[i, j]) for j in range(6)] for i in range(6)])
    return sign * scale * (d[:, None] * out * d[None, :])


# the seeds of hidden_deficiency found by search_hidden_deficiency(): pivots within ten decades, smallest singular value below
# threshold / 4
HIDDEN_SEEDS = (0, 1, 2, 3)


def search_hidden_deficiency(n=200):
    """The CPU search behind HIDDEN_SEEDS (run by hand): seeds whose matrix has min pivot > 1e-10 max pivot in f64 while the exact
    smallest singular value is below (6 eps sigma_max) / 4."""
    import ndt_ctl_ref as ref
    good = []
    for seed in range(n):
        H = hidden_deficiency(seed)
        pmin, pmax = device_rule_pivots(H)
        r = ref.pinv_reference(H, np.ones(6))
        if pmin > 1e-10 * pmax and r["kept"] == 5 and not r["near"]:
            good.append((seed, pmin / pmax, r["sigma"][-1] / r["sigma"][0]))
    return good


@functools.lru_cache(maxsize=None)
def systems():
    """-> tuple of dict(name, family, H [6, 6], b [6]).  Every matrix appears with a right-hand side in its range (b = H y) and
    with one that is not (random)."""
    out = []

    def add(family, name, H, rng):
        y = rng.uniform(-1, 1, 6)
        out.append(dict(family=family, name=f"{name}:range", H=H, b=H @ y))
        out.append(dict(family=family, name=f"{name}:free", H=H, b=rng.uniform(-1, 1, 6)))

    for seed in range(3):
        rng = np.random.default_rng(1000 + seed)
        mag = rng.uniform(1.0, 10.0, 6)
        add("well", f"definite:{seed}", _compose(_orth(rng), mag), rng)
        add("well", f"negative_definite:{seed}", _compose(_orth(rng), -mag), rng)
        add("well", f"indefinite:{seed}", _compose(_orth(rng), mag * np.array([1, -1, 1, -1, -1, 1.])), rng)
    for cond in (1e6, 1e9, 1e10, 1e11, 1e12, 1e14):
        for seed in range(4):
            rng = np.random.default_rng(2000 + seed + int(np.log10(cond)) * 10)
            s = np.concatenate([[1.0], 10.0 ** -rng.uniform(0, np.log10(cond), 4), [1.0 / cond]]) * rng.choice([-1.0, 1.0], 6)
            add("cond", f"cond{cond:g}:{seed}", _compose(_orth(rng), s * 2.0 ** rng.integers(-2, 3)), rng)
    for rank in (5, 4, 3, 0):
        for k in range(3 if rank else 1):
            rng = np.random.default_rng(3000 + 10 * rank + k)
            s = np.array([3.0, -2.0, 0.5, 1.0, -0.75, 4.0])
            s[rank:] = 0.0
            Q = _dyadic_orth(k)
            H = Q @ np.diag(s) @ Q.T
            add("rank", f"rank{rank}:{k}", H, rng)
    for ratio in (1e-17, 1e-14):
        for seed in range(4):
            rng = np.random.default_rng(4000 + seed + (0 if ratio < 1e-15 else 100))
            s = np.concatenate([rng.uniform(0.3, 1.0, 5), [ratio]]) * rng.choice([-1.0, 1.0], 6)
            s[0] = 1.0
            add("rounding", f"smin{ratio:g}:{seed}", _compose(_orth(rng), s), rng)
    for seed in HIDDEN_SEEDS:
        rng = np.random.default_rng(5000 + seed)
        add("hidden", f"hidden:{seed}", hidden_deficiency(seed), rng)
    return tuple(out)


# ------------------------------------------------------------------------------------------------------ objectives
class Objective:
    """score(p) = -1/2 (p - c)' A (p - c) - q (u . (p - c))^4 + sum_k w_k exp(-1/2 (p - m_k)' B_k (p - m_k)), with its gradient
    and Hessian in closed form (Ndt MAXIMISES the score; the line search works on phi = -score).  nan_from: the gradient is NaN
    from that evaluation (counted from 1) on."""

    def __init__(self, A, c, q=0.0, u=None, gauss=(), nan_from=None):
        self.A = np.asarray(A, dtype=np.float64); self.c = np.asarray(c, dtype=np.float64)
        self.q = float(q); self.u = np.zeros(6) if u is None else np.asarray(u, dtype=np.float64)
        self.gauss = [(float(w), np.asarray(m, dtype=np.float64), np.asarray(B, dtype=np.float64)) for w, m, B in gauss]
        self.nan_from = nan_from

    def __call__(self, p, n_eval):
        d = p - self.c
        Ad = self.A @ d
        t = float(self.u @ d)
        score = -0.5 * float(d @ Ad) - self.q * t ** 4
        g = -Ad - 4.0 * self.q * t ** 3 * self.u
        H = -self.A - 12.0 * self.q * t * t * np.outer(self.u, self.u)
        for w, m, B in self.gauss:
            e = p - m
            Be = B @ e
            v = w * float(np.exp(-0.5 * float(e @ Be)))
            score += v
            g = g - v * Be
            H = H + v * (np.outer(Be, Be) - B)
        if self.nan_from is not None and n_eval >= self.nan_from:
            g = np.full(6, np.nan)
        return float(score), g, H


def _spd(seed, lo, hi):
    rng = np.random.default_rng(seed)
    Q = _orth(rng)
    return Q @ np.diag(rng.uniform(lo, hi, 6)) @ Q.T


def _case(name, objective, p0, step_size, trans_eps, max_iterations=35):
    return dict(name=name, objective=objective, p0=np.asarray(p0, dtype=np.float64), step_size=float(step_size), trans_eps=float(trans_eps),
                max_iterations=int(max_iterations))


@functools.lru_cache(maxsize=None)
def runs():
    """The scripted runs.  (step_size, trans_eps) with step_size <= trans_eps / 2 open the line-search loop; with the wrapper's
    0.1 / 0.01-type settings it never runs."""
    out = []
    rng = np.random.default_rng(77)
    p_far = rng.uniform(-1, 1, 6)
    p_far *= 2.03 / np.linalg.norm(p_far)
    u = np.array([1, 2, -1, 0.5, 0, 1.0]); u /= np.linalg.norm(u)
    c0 = np.array([0.3, -0.2, 0.5, 0.1, -0.4, 0.2])                   # (an optimum away from the origin: a pose there has a size to be relative to)
    quad = Objective(_spd(1, 0.5, 4.0), c0)
    # wrapper-like settings: the loop has length 0, no Hessian-only evaluation, first steps clamped to step_size
    # (trans_eps 0.05: the run ends with the Newton step that reaches the optimum, before the gradient is rounding noise)
    out.append(_case("quadratic_default", quad, c0 + p_far, 0.1, 0.05))
    out.append(_case("quadratic_default_cap", quad, c0 + p_far, 0.1, 0.01, max_iterations=3))
    out.append(_case("quadratic_cap0", quad, c0 + p_far, 0.1, 0.01, max_iterations=0))
    # the loop runs
    for k, (ss, te) in enumerate([(0.05, 0.1), (0.1, 0.2), (0.1, 0.5), (0.5, 2.0), (1.0, 2.5)]):
        out.append(_case(f"quadratic_loop:{k}", quad, c0 + p_far, ss, te))
        out.append(_case(f"quartic_loop:{k}", Objective(_spd(2, 0.2, 1.0), np.zeros(6), q=3.0, u=u), p_far * 0.7, ss, te))
        g2 = [(2.0, 0.3 * u, _spd(3, 2.0, 6.0)), (1.0, -0.8 * u + 0.1, _spd(4, 1.0, 3.0))]
        out.append(_case(f"gauss_loop:{k}", Objective(_spd(5, 0.01, 0.05), np.zeros(6), gauss=g2), 0.25 * p_far, ss, te))
        out.append(_case(f"gauss_far_loop:{k}", Objective(_spd(5, 0.01, 0.05), np.zeros(6), gauss=g2), 0.6 * p_far, ss, te))
    # long steps over a narrow valley: trial values beyond the minimum (f_t > f_l), interval closed from above
    steep = Objective(_spd(6, 20.0, 60.0), np.zeros(6), q=50.0, u=u)
    for k, (ss, te) in enumerate([(1.0, 2.0), (0.6, 1.2), (2.0, 4.0)]):
        out.append(_case(f"steep_loop:{k}", steep, p_far * 0.4, ss, te))
        out.append(_case(f"steep_quad_loop:{k}", Objective(_spd(7, 1.0, 30.0), np.zeros(6)), p_far * 0.5, ss, te))
    # a score MINIMUM (positive definite Hessian of the score): the Newton direction descends, d_phi_0 > 0, reversed
    out.append(_case("reversal", Objective(-_spd(8, 0.5, 2.0), np.zeros(6)), 0.3 * p_far, 0.1, 0.01, max_iterations=4))
    out.append(_case("reversal_loop", Objective(-_spd(8, 0.5, 2.0), np.zeros(6)), 0.3 * p_far, 0.1, 0.3, max_iterations=4))
    # H = diag(1, -1, 1, ...), g = (1, 1, 0, ...): the Newton step is orthogonal to the gradient, d_phi_0 == 0 exactly
    out.append(_case("d_phi_0_zero", Objective(np.diag([-1.0, 1, -1, -1, -1, -1]), np.zeros(6)), [1.0, -1, 0, 0, 0, 0], 0.1, 0.01))
    # at the optimum: gradient exactly zero, dp_norm == 0 at once
    out.append(_case("dp_norm_zero", quad, c0, 0.1, 0.01))
    # no overlap: score, gradient and Hessian all zero
    out.append(_case("all_zero", Objective(np.zeros((6, 6)), np.zeros(6)), p_far, 0.1, 0.01))
    # a NaN gradient at the first evaluation and after a step.  (Not inside an open line search: there the NaN would enter
    # comparisons, which clears no margin -- and the reference's std::min / std::max would carry a NaN trial value into the pose,
    # where the device's fmin / fmax put it back into [step_min, step_max].)
    out.append(_case("nan_at_init", Objective(_spd(1, 0.5, 4.0), np.zeros(6), nan_from=1), p_far, 0.1, 0.01))
    out.append(_case("nan_after_step", Objective(_spd(1, 0.5, 4.0), np.zeros(6), nan_from=3), p_far, 0.1, 0.01))
    return tuple(out)


# ------------------------------------------------------------------------------------------------------ the helpers alone
@functools.lru_cache(maxsize=None)
def mt_tuples():
    """(a_l, f_l, g_l, a_u, f_u, g_u, a_t, f_t, g_t) for trial_value_mt / update_interval_mt called directly.  Inside a run the
    loop only opens when step_size <= trans_eps / 2, and then every trial value is clamped to trans_eps / 2: the machine cannot
    reach update_interval_mt's second outcome (a_l moves up, the slope still negative) and could reach trial_value_mt's fourth
    case only through a NaN.  The five written tuples take each case and each outcome once; the seeded ones add numbers of every
    sign."""
    base = (0.1, -0.2, -1.0, 0.9, 0.3, 0.5)
    out = [("trial1_update1", base + (0.5, 0.1, 0.7)), ("trial2_update3", base + (0.5, -0.5, 0.4)), ("trial3_update2", base + (0.5, -0.5, -0.6)),
           ("trial4_update2", base + (0.5, -0.5, -1.5)), ("trial3_update4", base + (0.5, -0.5, 0.0))]
    rng = np.random.default_rng(606)
    for k in range(48):
        lo, mid, hi = np.sort(rng.uniform(0.0, 2.0, 3))
        a_l, a_t, a_u = (lo, mid, hi) if k % 2 else (hi, mid, lo)     # the trial value between the interval's ends, either way round
        out.append((f"seeded:{k}", (a_l, rng.uniform(-1, 1), rng.uniform(-2, 2), a_u, rng.uniform(-1, 1), rng.uniform(-2, 2), a_t, rng.uniform(-1, 1),
                                   rng.uniform(-2, 2))))
    return tuple((n, tuple(float(v) for v in t)) for n, t in out)
