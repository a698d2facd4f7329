"""A multi-precision restatement of the serial end of an IcpFast iteration (registrators/icp_fast.cc:204-254, 306-323, 377-405,
455-529), in mpmath at 60 digits: what staticmapping_amd/csrc/icp_tail_math.h, oracle/icp_fast.py and oracle/csrc/smref_icp.c are
measured against.  Nothing here is tuned to any of them.

The decisions (which pivot, which rank, which quaternion branch, which rows are kept) follow the reference's rules and are taken
on the exact values; every number is an mpf until it is handed back.
"""
import mpmath as mp
import numpy as np

mp.mp.dps = 60
EPS = mp.mpf(2) ** -52
SIZE = 6


def M(a):
    """numpy / nested list -> list of rows of mpf (f64 values enter exactly)."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        return [mp.mpf(float(v)) for v in a]
    return [[mp.mpf(float(v)) for v in r] for r in a]


def to_np(a):
    return np.array([[float(v) for v in r] for r in a]) if isinstance(a[0], list) else np.array([float(v) for v in a])


def matmul(A, B):
    return [[mp.fsum(A[i][k] * B[k][j] for k in range(len(B))) for j in range(len(B[0]))] for i in range(len(A))]


def matvec(A, x):
    return [mp.fsum(a * v for a, v in zip(r, x)) for r in A]


def norm(x):
    return mp.sqrt(mp.fsum(v * v for v in x))


def eye(n):
    return [[mp.mpf(int(i == j)) for j in range(n)] for i in range(n)]


# ------------------------------------------------------------------------------------------- normal equations
def normal_equations(P, Qm, N):
    """A = sum F F^T, b = -sum F ((p - q) . n) with F = [p x n; n] (icp_fast.cc:267-302).  P, Qm, N: rows of 3 mpf."""
    A = [[mp.mpf(0)] * 6 for _ in range(6)]
    b = [mp.mpf(0)] * 6
    for p, q, n in zip(P, Qm, N):
        F = (p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2])
        r = (p[0] - q[0]) * n[0] + (p[1] - q[1]) * n[1] + (p[2] - q[2]) * n[2]
        for i in range(6):
            if F[i] == 0:
                continue
            Ai = A[i]
            for j in range(i, 6):
                Ai[j] = Ai[j] + F[i] * F[j]
            b[i] = b[i] - F[i] * r
    for i in range(6):
        for j in range(i):
            A[i][j] = A[j][i]
    return A, b


# ------------------------------------------------------------------------------------------- Eigen's FullPivHouseholderQR
def fullpiv_qr_pivots(A, stop=True):
    """|R_kk| of the full-pivot Householder QR (Eigen/src/QR/FullPivHouseholderQR.h): the largest entry of the remaining corner
    is brought to the corner at every step.  The elimination stops at a corner that is negligible against the first one
    (eps * size); the pivots after it are zero.  stop=False eliminates to the end: the pivots the stop hides."""
    n = len(A)
    W = [list(r) for r in A]
    piv = [mp.mpf(0)] * n
    prec = EPS * n
    biggest = mp.mpf(0)
    for k in range(n):
        big, pr, pc = mp.mpf(-1), k, k
        for i in range(k, n):
            for j in range(k, n):
                if abs(W[i][j]) > big:
                    big, pr, pc = abs(W[i][j]), i, j
        if k == 0:
            biggest = big
        if stop and not big > biggest * prec:
            break
        if big == 0:
            break
        W[k], W[pr] = W[pr], W[k]
        for r in W:
            r[k], r[pc] = r[pc], r[k]
        tail2 = mp.fsum(W[i][k] ** 2 for i in range(k + 1, n))
        c0 = W[k][k]
        beta = c0
        if tail2 > 0:
            beta = mp.sqrt(c0 * c0 + tail2)
            if c0 >= 0:
                beta = -beta
            v = [mp.mpf(1)] + [W[i][k] / (c0 - beta) for i in range(k + 1, n)]
            tau = (beta - c0) / beta
            for j in range(k + 1, n):
                s = tau * mp.fsum(v[i - k] * W[i][j] for i in range(k, n))
                for i in range(k, n):
                    W[i][j] -= s * v[i - k]
        piv[k] = abs(beta)
    return piv


def qr_rank(A):
    """(rank, pivots, min pivot / threshold): Eigen's rank() counts the pivots above eps * size * the largest; isInvertible() is
    rank == size.  The ratio (of the smallest pivot of the elimination carried to its end) is how far the decision `invertible` is
    from flipping (1 = on the threshold)."""
    piv = fullpiv_qr_pivots(A)
    pmax = max(piv)
    thresh = EPS * len(A) * pmax
    rank = sum(1 for p in piv if p > thresh)
    raw = fullpiv_qr_pivots(A, stop=False)
    ratio = (min(raw) / thresh) if pmax > 0 else mp.mpf(0)
    return rank, piv, ratio


def solve_full(A, b):
    return list(mp.lu_solve(mp.matrix(A), mp.matrix(b)))


def eigsy(A):
    w, V = mp.eigsy(mp.matrix(A))
    n = len(A)
    return [w[i] for i in range(n)], [[V[i, j] for j in range(n)] for i in range(n)]


def solve_min_norm(A, b, rank):
    """The minimum-norm solution of the system reduced to its `rank` largest eigenvalues (what R1^T (R1 R1^T)^-1 Q1^T b of
    icp_fast.cc:216-229 is when the dropped part is zero)."""
    w, V = eigsy(A)
    order = sorted(range(len(w)), key=lambda k: -abs(w[k]))[:rank]
    x = [mp.mpf(0)] * len(w)
    for k in order:
        c = mp.fsum(V[i][k] * b[i] for i in range(len(w))) / w[k]
        for i in range(len(w)):
            x[i] += c * V[i][k]
    return x


def eig_gap(A, rank):
    """smallest kept |eigenvalue| / largest dropped one (inf when nothing is dropped or the dropped ones are zero)."""
    w = sorted((abs(v) for v in eigsy(A)[0]), reverse=True)
    if rank >= len(w) or rank == 0:
        return mp.inf
    return mp.inf if w[rank] == 0 else w[rank - 1] / w[rank]


def solve_reference(A, b):
    """SolvePossiblyUnderdeterminedLinearSystem -> (x, rank)."""
    rank, _, _ = qr_rank(A)
    if rank == len(A):
        return solve_full(A, b), rank
    return solve_min_norm(A, b, rank), rank


# ------------------------------------------------------------------------------------------- rotations
def angle_axis(x):
    """AngleAxis(|x|, x / |x|).toRotationMatrix(); the exact value at x = 0 is the identity (the f64 code gets there through its
    NaN guard)."""
    ang = norm(x[:3])
    if ang == 0:
        return eye(3)
    a = [v / ang for v in x[:3]]
    c, s = mp.cos(ang), mp.sin(ang)
    v = 1 - c
    return [[c + v * a[0] * a[0], v * a[0] * a[1] - s * a[2], v * a[0] * a[2] + s * a[1]],
            [v * a[0] * a[1] + s * a[2], c + v * a[1] * a[1], v * a[1] * a[2] - s * a[0]],
            [v * a[0] * a[2] - s * a[1], v * a[1] * a[2] + s * a[0], c + v * a[2] * a[2]]]


def quat_from_rot(R):
    """Eigen::Quaterniond(Matrix3d) -> (branch 0..3, (w, x, y, z))."""
    t = R[0][0] + R[1][1] + R[2][2]
    if t > 0:
        s = mp.sqrt(t + 1) * 2
        return 0, [s / 4, (R[2][1] - R[1][2]) / s, (R[0][2] - R[2][0]) / s, (R[1][0] - R[0][1]) / s]
    i = 0
    if R[1][1] > R[0][0]:
        i = 1
    if R[2][2] > R[i][i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    s = mp.sqrt(R[i][i] - R[j][j] - R[k][k] + 1) * 2
    q = [mp.mpf(0)] * 4
    q[1 + i] = s / 4
    q[0] = (R[k][j] - R[j][k]) / s
    q[1 + j] = (R[j][i] + R[i][j]) / s
    q[1 + k] = (R[k][i] + R[i][k]) / s
    return 1 + i, q


def angular_distance(a, c):
    """Eigen::Quaternion::angularDistance: the angle of a * conj(c), 2 atan2(|vec|, |w|)."""
    w = a[0] * c[0] + a[1] * c[1] + a[2] * c[2] + a[3] * c[3]
    x = -a[0] * c[1] + a[1] * c[0] - a[2] * c[3] + a[3] * c[2]
    y = -a[0] * c[2] + a[2] * c[0] - a[3] * c[1] + a[1] * c[3]
    z = -a[0] * c[3] + a[3] * c[0] - a[1] * c[2] + a[2] * c[1]
    return 2 * mp.atan2(mp.sqrt(x * x + y * y + z * z), abs(w))


def sigma_max3(D):
    """The largest singular value of a 3x3."""
    S = matmul([[D[j][i] for j in range(3)] for i in range(3)], D)
    w, _ = eigsy(S)
    return mp.sqrt(max(max(w), mp.mpf(0)))


def check_convergence(quats, trans):
    """icp_fast.cc:377-405 over the whole history (the identity start included) -> (converged, mean rot step, mean trans step)."""
    if len(quats) <= 4:
        return False, None, None
    rd = mp.fsum(abs(angular_distance(quats[i], quats[i - 1])) for i in range(len(quats) - 4, len(quats))) / 4
    td = mp.fsum(norm([a - b for a, b in zip(trans[i], trans[i - 1])]) for i in range(len(quats) - 4, len(quats))) / 4
    return bool(rd < mp.mpf("1e-3") and td < mp.mpf("1e-2")), rd, td


# ------------------------------------------------------------------------------------------- one step, k steps
def quantile_keep(d2, ratio_f32):
    """GetDistsQuantile's rank rule (icp_fast.cc:65-90) on f64 d2 -> (limit, keep mask).  ratio is the float option widened."""
    vals = d2[np.isfinite(d2)]
    rho = float(np.float32(ratio_f32))
    limit = float(vals.max()) if rho == 1.0 else float(np.partition(vals, int(vals.size * rho))[int(vals.size * rho)])
    return limit, (d2 <= limit) & np.isfinite(d2)


def icp_step(P, Qm, N, force_rank=None):
    """One ComputePointToPlane on matched rows of mpf -> (dT 4x4, A, b, x, rank).  force_rank: the rank to solve at instead of
    the rule's (for a matrix so close to the threshold that an f64 QR cannot tell)."""
    A, b = normal_equations(P, Qm, N)
    x, rank = solve_reference(A, b)
    if force_rank is not None and force_rank != rank:
        rank = force_rank
        x = solve_full(A, b) if rank == 6 else solve_min_norm(A, b, rank)
    R = angle_axis(x)
    dT = eye(4)
    for i in range(3):
        for j in range(3):
            dT[i][j] = R[i][j]
        dT[i][3] = x[3 + i]
    return dT, A, b, x, rank


def icp_driver(source, target, normals, guess=None, max_iteration=5, ratio=1.0, early_exit=False, nn=None, force_rank=None):
    """IcpFast::Align (icp_fast.cc:455-529).  The neighbour search is brute force in f64 on the f64 rounding of the exact step
    cloud (the scenes keep every runner-up far away, which the caller asserts through `nn`'s third return value).
    -> dict(results {iteration count: 4x4 of mpf, for every count up to the stop}, iterations, kept [per iteration], ranks,
            min_gap (smallest runner-up distance minus nearest distance met), A [per iteration])."""
    from icp_tail_cases import nn_bruteforce
    nn = nn or nn_bruteforce
    S, Q, Nn = M(source), M(target), M(normals)
    n = len(Q)
    mu = [mp.fsum(q[c] for q in Q) / n for c in range(3)]
    Qc = [[q[c] - mu[c] for c in range(3)] for q in Q]
    Qc64 = to_np(Qc)
    G = M(np.eye(4) if guess is None else guess)
    Tm_inv = eye(4); Tm = eye(4)
    for c in range(3):
        Tm_inv[c][3] = -mu[c]; Tm[c][3] = mu[c]
    G = matmul(Tm_inv, G)
    P0 = [[mp.fsum(G[r][c] * s[c] for c in range(3)) + G[r][3] for r in range(3)] for s in S]
    T = eye(4)
    quats, trans = [[mp.mpf(1), mp.mpf(0), mp.mpf(0), mp.mpf(0)]], [[mp.mpf(0)] * 3]
    out = dict(results={}, kept=[], ranks=[], A=[], b=[], min_gap=np.inf, min_quantile_gap=np.inf)
    it = 0
    while True:
        ident = all(T[i][j] == (1 if i == j else 0) for i in range(4) for j in range(4))
        P = P0 if ident else [[mp.fsum(T[r][c] * p[c] for c in range(3)) + T[r][3] for r in range(3)] for p in P0]
        ids, d1, d2nd = nn(to_np(P), Qc64)
        out["min_gap"] = min(out["min_gap"], float((np.sqrt(d2nd) - np.sqrt(d1)).min()))
        limit, keep = quantile_keep(d1, ratio)
        srt = np.sort(d1)
        k = int(len(srt) * float(np.float32(ratio)))
        if 0 < k < len(srt) - 1:
            out["min_quantile_gap"] = min(out["min_quantile_gap"], float(min(srt[k] - srt[k - 1], srt[k + 1] - srt[k]) / srt[k]))
        rows = np.nonzero(keep)[0]
        dT, A, b, x, rank = icp_step([P[i] for i in rows], [Qc[ids[i]] for i in rows], [Nn[ids[i]] for i in rows], force_rank)
        out["kept"].append(int(keep.sum())); out["ranks"].append(rank); out["A"].append(A); out["b"].append(b)
        T = matmul(dT, T)
        it += 1
        _, q = quat_from_rot(T)
        quats.append(q); trans.append([T[0][3], T[1][3], T[2][3]])
        out["results"][it] = matmul(Tm, matmul(T, G))
        if (early_exit and check_convergence(quats, trans)[0]) or it >= max_iteration:
            break
    out["iterations"] = it
    return out


_RUNS = {}


def scene_run(name, max_iteration=5, ratio=1.0, early_exit=False, force_rank=None):
    """icp_driver on a scene of icp_tail_cases, computed once per process and shared by every test that needs it (treat as
    read-only)."""
    import icp_tail_cases as cases
    key = (name, max_iteration, float(ratio), bool(early_exit), force_rank)
    if key not in _RUNS:
        s = cases.get_scene(name)
        _RUNS[key] = icp_driver(s["source"].astype(np.float64), s["target"], s["normals"], max_iteration=max_iteration, ratio=ratio,
                                early_exit=early_exit, force_rank=force_rank)
    return _RUNS[key]


# ------------------------------------------------------------------------------------------- the decision ladder, judged once
_LADDER = {}


def ladder_reference():
    """Every matrix of the decision ladder (icp_tail_cases.ladder() and the first iteration's A, b of the eps-corridors) with what
    the reference rule says about it, computed once per process:
      rows: dict(name, A, b [f64], rank, ratio, x [mpf: full solution at rank 6, minimum norm below], gap, oracle_x, oracle_err,
                 tol, in_band)
      band: B = 4 x the largest relative error of the smallest pivot of oracle/icp_fast.py's f64 QR against the exact one, over the
            rungs the exact rule calls invertible; a rung is inside the band when 1 / (1 + B) <= ratio <= 1 + B.
    tol is 8 x |oracle_x - x| with a floor of 64 eps |x| (the margin convention of test_normals_exact_gpu.py)."""
    if _LADDER:
        return _LADDER
    import scipy.linalg
    import icp_tail_cases as cases
    from oracle import icp_fast as py_oracle
    rows = [dict(name=c["name"], A=c["A"], b=c["b"]) for c in cases.ladder()]
    for e in cases.EPSILONS:
        run = scene_run(f"eps_corridor:{e:g}")
        rows.append(dict(name=f"scene:eps_corridor:{e:g}", A=to_np(run["A"][0]), b=to_np(run["b"][0])))
    worst = 0.0
    for r in rows:
        A, b = M(r["A"]), M(r["b"])
        rank, piv, ratio = qr_rank(A)
        r["rank"], r["ratio"] = rank, float(ratio)
        r["x"] = solve_full(A, b) if rank == 6 else solve_min_norm(A, b, rank)
        r["gap"] = float(eig_gap(A, rank))
        with np.errstate(all="ignore"):
            ox = py_oracle.solve_possibly_underdetermined(r["A"], r["b"]) if np.abs(r["A"]).max() > 0 else np.zeros(6)
        r["oracle_x"] = ox
        r["oracle_err"] = float(norm([mp.mpf(float(a)) - v for a, v in zip(ox, r["x"])]))
        r["tol"] = max(8.0 * r["oracle_err"], 64.0 * float(EPS) * float(norm(r["x"])))
        if rank == 6:
            p64 = np.abs(np.diag(scipy.linalg.qr(r["A"], pivoting=True)[1])).min()
            pmin = min(piv)
            worst = max(worst, float(abs(mp.mpf(float(p64)) - pmin) / pmin))
    band = 4.0 * worst
    for r in rows:
        r["in_band"] = bool(1.0 / (1.0 + band) <= r["ratio"] <= 1.0 + band)
    _LADDER.update(rows=rows, band=band, worst_pivot_error=worst)
    return _LADDER
