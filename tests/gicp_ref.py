"""Constructed inputs and a float64 reference for the GICP side of registrators::NdtWithGicp: the neighbour sets and
covariances of computeCovariances (pclomp/gicp_omp_impl.hpp:59-131), the correspondence filter with its Mahalanobis matrices
(:441-463) and the sums of OptimizationFunctorWithIndices (:250-377).  CPU only: numpy, scipy and oracle.ndt_gicp, nothing of
the device.

Coordinates.  A lattice cloud has every coordinate a multiple of Q = 2^-4 m with |x| < 64, so the float products p.x * p.y and
every squared distance are exact whatever the FMA contraction, and it is point-symmetric about a lattice point (or closes its
sum with one last point), so its mean and every centred coordinate float(double(p) - mean) are exact too: the device, which
searches the centred cloud, sees the distances the reference sees, ties included.  `check_lattice` asserts all of that.  The point
order is shuffled with a fixed seed: index order says nothing about position.

Neighbour set.  The brute-force k smallest by (exact squared distance, index in the caller's cloud), the point itself included.
The covariance follows oracle.ndt_gicp.gicp_covariances: float products, double sums (here in index order), c / k - mean mean^T,
then I - (1 - eps) u u^T with u the eigenvector of the smallest |eigenvalue|.

Covariance tolerance.  Per point K_COV * 2^-53 * lmax / (l2 - l1) on the entries of C, l1 <= l2 <= lmax the |eigenvalues| of that
point's k-neighbour covariance in the reference.  K_COV is not chosen: RHO_COV is the largest such ratio between two legitimate
CPU evaluations of the reference over every committed (cloud, k) -- eigh and index-order sums against SVD and math.fsum, and
c / k - mean mean^T with every operation rounded against the same with the product contracted into a fused multiply-add --
and K_COV = 4 max(1, RHO_COV) rounded up to a power of two.  tests/test_gicp_ref.py re-measures RHO_COV.  (The contraction is
what sets it: off the lattice the single-pass covariance cancels |p|^2 against a neighbourhood's extent, 445 at k = 3 on the
generic cloud; eigh against SVD on the lattice clouds, whose sums are exact, gives 60.)

Functor tolerance.  For f and the six gradient entries the reference returns A_c, the sum of the absolute addends, and N_c, the
largest change over 16 seeded re-evaluations with every transformed coordinate moved by -1, 0 or +1 float ulp (N_c = 0 at
x = 0, where the float transform of lattice points is exact).  S_c = 2^-53 A_c + N_c and a device is allowed K_F S_c.  RHO_F is
the largest |alternative - reference| / S_c over the committed cases, the alternatives being the three transform_modes of
oracle.ndt_gicp.GicpFunctor's transform (nofma is the reference; fma and blas) and a second evaluation of the Mahalanobis
matrices (SVD covariances, cofactor inverse instead of eigh and LAPACK); K_F = 4 max(1, RHO_F) rounded up to a power of two.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np
from scipy.spatial import cKDTree

from oracle import ndt_gicp as ong

F = np.float32
Q = 2.0 ** -4
KS = (3, 19, 20, 21, 32)
EPS = 1e-3                      # gicp_epsilon
KMAX = 32
U53 = 2.0 ** -53

# measured by `python -m pytest tests/test_gicp_ref.py -q -s -k measured` (it prints them and asserts they still bound what it
# measures); K = 4 * max(1, RHO) rounded up to a power of two
RHO_COV = 445.5
K_COV = 2048.0
RHO_F = 1166.0
K_F = 8192.0


def _pow2_above(v):
    return float(2.0 ** math.ceil(math.log2(v)))


def k_from_rho(rho):
    return _pow2_above(4.0 * max(1.0, rho))


# ---------------------------------------------------------------------------------------------
# clouds
# ---------------------------------------------------------------------------------------------
def check_lattice(cloud):
    """Every coordinate a multiple of Q below 64 m, the mean exact in double, every centred coordinate exact in float."""
    p = np.asarray(cloud, dtype=F)[:, :3].astype(np.float64)
    u = p / Q
    assert (u == np.round(u)).all() and (np.abs(p) < 64).all()
    n = len(p)
    s = np.round(u).astype(np.int64).sum(axis=0)
    for d in range(3):
        mu = Fraction(int(s[d]), n) / 16
        assert Fraction(float(mu)) == mu and mu * 2 ** 24 == int(mu * 2 ** 24), (d, mu)     # exact, and p - mu is exact in double
        c = p[:, d] - float(mu)
        assert (c.astype(F).astype(np.float64) == c).all(), d
    return True


def height_field(nx, ny, step, seed, hmax=4, flat=False):
    """nx * ny points over an x / y lattice of `step`, z = Q h with h a seeded integer in 0..hmax, point-symmetric about
    (0, 0, Q hmax / 2): h(-x, -y) = hmax - h(x, y).  Returns the shuffled float32 cloud and, per point, the index of its mirror."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    h = rng.integers(0, hmax + 1, size=i.shape)
    flip = h[::-1, ::-1]
    first = (i * ny + j) < ((nx - 1 - i) * ny + (ny - 1 - j))
    h = np.where(first, h, hmax - flip)
    if (nx * ny) % 2:
        assert hmax % 2 == 0
        h[nx // 2, ny // 2] = hmax // 2
    if flat:
        h = np.zeros_like(h)
    pts = np.stack([(i - (nx - 1) / 2) * step, (j - (ny - 1) / 2) * step, Q * h], axis=-1).reshape(-1, 3)
    mirror_flat = ((nx - 1 - i) * ny + (ny - 1 - j)).reshape(-1)
    perm = rng.permutation(len(pts))                     # cloud[r] = pts[perm[r]]
    inv = np.empty_like(perm); inv[perm] = np.arange(len(perm))
    return pts[perm].astype(F), inv[mirror_flat[perm]]


def closed_sum_cloud(n, seed):
    """n distinct lattice points: n - 1 seeded ones in a small box and one that closes the sum, so the mean is the origin."""
    for s in range(seed, seed + 1000):
        rng = np.random.default_rng(s)
        a = np.stack([rng.integers(-10, 11, n - 1) * 4, rng.integers(-10, 11, n - 1) * 4, rng.integers(-2, 3, n - 1)], axis=1)
        pts = np.concatenate([a, -a.sum(axis=0, keepdims=True)])
        if len(np.unique(pts, axis=0)) == n and np.abs(pts).max() * Q < 64:
            return (pts[rng.permutation(n)] * Q).astype(F)
    raise AssertionError("no seed gives distinct points")


def generic_cloud(seed=77):
    """Not on a lattice: a dense cluster and a handful of points 30-80 m away (shell doubling, r > rmax, chord pruning)."""
    rng = np.random.default_rng(seed)
    cluster = rng.normal(0.0, 1.0, (1500, 3)) * np.array([1.0, 0.8, 0.15])
    d = rng.normal(0.0, 1.0, (9, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    far = d * rng.uniform(30.0, 80.0, (9, 1))
    pts = np.concatenate([cluster, far])
    return pts[rng.permutation(len(pts))].astype(F)


TIES_SEED = 11


@functools.lru_cache(maxsize=None)
def cloud(name):
    if name == "ties":                                   # 2048 points, 0.25 m lattice
        return height_field(64, 32, 0.25, TIES_SEED)[0]
    if name == "dups":                                   # every point present twice
        base = height_field(32, 32, 0.25, 12)[0]
        both = np.concatenate([base, base])
        return both[np.random.default_rng(13).permutation(len(both))]
    if name == "plane":                                  # z = const: diag(1, 1, eps) in the plane's frame
        p = height_field(32, 32, 0.25, 14, flat=True)[0].copy()
        p[:, 2] = 0.5
        return p
    if name == "generic":
        return generic_cloud()
    if name.startswith("n"):                             # n<k>+<d>: k + d points; n127 ...: that many
        return closed_sum_cloud(cloud_size(name), 100 + cloud_size(name))
    raise KeyError(name)


def cloud_size(name):
    if "+" in name:
        a, b = name[1:].split("+")
        return int(a) + int(b)
    return int(name[1:])


LATTICE_CLOUDS = ("ties", "dups", "plane", "n127", "n128", "n129") + tuple(f"n{k}+{d}" for k in KS for d in (0, 1))


def is_lattice(name):
    return name != "generic"


def cloud_ks(name):
    """The k a cloud is used with: every k that its size allows; a cloud of exactly k or k + 1 points with that k."""
    if "+" in name:
        return (int(name[1:].split("+")[0]),)
    # k = 3 on a square lattice picks collinear triples (two opposite lattice neighbours): a rank-one covariance, whose
    # smallest two |eigenvalues| are both zero, so that C is not defined.  k = 3 is pinned on the clouds where it is: the
    # clouds of 3 and 4 points and the generic cloud.
    # k = 21 completes a distance class of the 0.25 m lattice for most points of the ties cloud (6 % tied, 124 covariances
    # that depend on the rule): that cloud is used with the k that cut through a class, k = 21 with the others -- every
    # point of the doubled cloud is tied at k = 21.
    return KS if name == "generic" else (19, 20, 32) if name == "ties" else KS[1:]


COV_CASES = tuple((c, k) for c in LATTICE_CLOUDS + ("generic",) for k in cloud_ks(c))
GENERIC_CAP = 0.02


# ---------------------------------------------------------------------------------------------
# neighbour sets and covariances
# ---------------------------------------------------------------------------------------------
def neighbour_order(pts, kmax=KMAX + 1, largest=False):
    """Brute force: per point the first kmax others (itself included) by (exact squared distance, index) -- or by
    (distance, -index) with largest=True, the wrong rule.  Returns indices [N, m] and squared distances [N, m]."""
    p = np.asarray(pts, dtype=F)[:, :3].astype(np.float64)
    n = len(p)
    m = min(kmax, n)
    idx = np.empty((n, m), dtype=np.int64); d2 = np.empty((n, m))
    for a in range(0, n, 256):
        d = ((p[a:a + 256, None, :] - p[None, :, :]) ** 2).sum(axis=2)
        if largest:
            o = n - 1 - np.argsort(d[:, ::-1], axis=1, kind="stable")[:, :m]
        else:
            o = np.argsort(d, axis=1, kind="stable")[:, :m]
        idx[a:a + 256] = o
        d2[a:a + 256] = np.take_along_axis(d, o, axis=1)
    return idx, d2


@functools.lru_cache(maxsize=None)
def cloud_order(name, largest=False):
    return neighbour_order(cloud(name), largest=largest)


def tied(d2, k):
    """Points whose k-th and (k + 1)-th neighbours are at the same distance."""
    if d2.shape[1] <= k:
        return np.zeros(len(d2), dtype=bool)
    return d2[:, k - 1] == d2[:, k]


def generic_excused(pts, d2, k):
    """Generic cloud only: points whose k-th and (k + 1)-th squared distances are closer than what the rounding of the centred
    coordinates can move them by: 8 ulp of the largest coordinate times the k-th distance."""
    ulp = float(np.spacing(F(np.abs(np.asarray(pts, dtype=F)[:, :3]).max())))
    dk = np.sqrt(d2[:, k - 1])
    return (d2[:, k] - d2[:, k - 1]) < 8.0 * ulp * np.maximum(dk, ulp)


def _sym_eig_abs(A):
    w = np.linalg.eigvalsh(A)
    return np.sort(np.abs(w), axis=1)


def covariances(pts, nn, eps=EPS, method="eigh", fsum=False, contract=False):
    """gicp_omp_impl.hpp:59-131 over the neighbour sets nn [N, k].  Returns C [N, 3, 3] and the sorted |eigenvalues| [N, 3].
    contract: c / k - mean_a mean_b with the product unrounded, as a compiler that contracts it into a fused multiply-add
    leaves it (through the 64-bit significand of long double)."""
    pf = np.asarray(pts, dtype=F)[:, :3]
    nn = np.sort(nn, axis=1)                                 # summed in index order
    n, k = nn.shape
    P = pf[nn]
    pairs = [(0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (2, 2)]
    prod = np.stack([P[:, :, a] * P[:, :, b] for a, b in pairs], axis=2).astype(np.float64)       # float products
    Pd = P.astype(np.float64)
    if fsum:
        mean = np.array([[math.fsum(Pd[i, :, a]) for a in range(3)] for i in range(n)])
        c = np.array([[math.fsum(prod[i, :, e]) for e in range(6)] for i in range(n)])
    else:
        mean = np.zeros((n, 3)); c = np.zeros((n, 6))
        for m in range(k):
            mean += Pd[:, m]; c += prod[:, m]
    mean = mean / k
    A = np.zeros((n, 3, 3))
    for e, (a, b) in enumerate(pairs):
        if contract:
            L = np.longdouble
            A[:, a, b] = A[:, b, a] = ((c[:, e] / k).astype(L) - mean[:, a].astype(L) * mean[:, b].astype(L)).astype(np.float64)
        else:
            A[:, a, b] = A[:, b, a] = c[:, e] / k - mean[:, a] * mean[:, b]
    if method == "eigh":
        w, U = np.linalg.eigh(A)
        col = np.argmin(np.abs(w), axis=1)
        u3 = np.take_along_axis(U, col[:, None, None], axis=2)[:, :, 0]
    else:
        U, _, _ = np.linalg.svd(A)
        u3 = U[:, :, 2]
    C = np.eye(3)[None] - (1.0 - eps) * u3[:, :, None] * u3[:, None, :]
    return C, _sym_eig_abs(A)


def cov_scale(lam):
    """2^-53 lmax / (l2 - l1) per point (inf where the two smallest |eigenvalues| coincide)."""
    with np.errstate(divide="ignore"):
        return U53 * lam[:, 2] / (lam[:, 1] - lam[:, 0])


def eigen_gap(lam):
    return (lam[:, 1] - lam[:, 0]) / lam[:, 2]


@functools.lru_cache(maxsize=None)
def cov_reference(name, k):
    """(C, scale, checked) of cloud `name`: the reference covariances, 2^-53 lmax / (l2 - l1) and the points that are compared
    (all of a lattice cloud)."""
    idx, d2 = cloud_order(name)
    C, lam = covariances(cloud(name), idx[:, :k])
    checked = np.ones(len(C), dtype=bool) if is_lattice(name) else ~generic_excused(cloud(name), d2, k)
    return C, cov_scale(lam), checked


def cov_ratio(got, name, k):
    """Worst |got - reference| / scale over the compared points, and where."""
    C, scale, checked = cov_reference(name, k)
    err = np.abs(np.asarray(got) - C).max(axis=(1, 2))
    r = np.where(err == 0, 0.0, err / scale)
    r[~checked] = 0.0
    i = int(np.argmax(r))
    return float(r[i]), i


def measure_rho_cov(cases=COV_CASES):
    worst = 0.0
    for name, k in cases:
        idx, _ = cloud_order(name)
        for method, fsum, contract in (("svd", True, False), ("svd", True, True), ("eigh", False, True)):
            alt, _ = covariances(cloud(name), idx[:, :k], method=method, fsum=fsum, contract=contract)
            worst = max(worst, cov_ratio(alt, name, k)[0])
    return worst


# ---------------------------------------------------------------------------------------------
# correspondences, Mahalanobis matrices, functor
# ---------------------------------------------------------------------------------------------
PERM = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], dtype=np.float64)      # x -> y -> z -> x: entries 0 / 1, R != R^T


def guess_matrix(t, rotate):
    G = np.eye(4, dtype=F)
    if rotate:
        G[:3, :3] = PERM
    G[:3, 3] = np.asarray(t, dtype=F)
    return G


def transform_f32(pts, T, mode="nofma"):
    """The float 4x4 * point product of :263-268 in the written order; mode as oracle.ndt_gicp.GicpFunctor's transform_mode."""
    x = np.asarray(pts, dtype=F)[:, :3]
    T = np.asarray(T, dtype=F)
    if mode == "blas":
        x4 = np.concatenate([x, np.ones((len(x), 1), dtype=F)], axis=1)
        return (x4 @ T.T).astype(F)[:, :3]
    out = np.empty((len(x), 3), dtype=F)
    for r in range(3):
        a, b, c, d = T[r]
        if mode == "nofma":
            out[:, r] = ((a * x[:, 0] + b * x[:, 1]) + c * x[:, 2]) + d
        else:
            t = (np.float64(a) * x[:, 0].astype(np.float64) + np.float64(d)).astype(F)
            t = (np.float64(b) * x[:, 1].astype(np.float64) + t.astype(np.float64)).astype(F)
            out[:, r] = (np.float64(c) * x[:, 2].astype(np.float64) + t.astype(np.float64)).astype(F)
    return out


def apply_state_f32(T, x):
    """applyState (:516-527) with every float product and sum rounded in turn: Rz Ry, then (Rz Ry) Rx, then R * T.topLeft."""
    a, b, c = F(x[3]), F(x[4]), F(x[5])
    cs = lambda v: (F(np.cos(np.float64(v))), F(np.sin(np.float64(v))))
    (ca, sa), (cb, sb), (cc, sc) = cs(a), cs(b), cs(c)
    o, z = F(1), F(0)
    Rx = [[o, z, z], [z, ca, -sa], [z, sa, ca]]
    Ry = [[cb, z, sb], [z, o, z], [-sb, z, cb]]
    Rz = [[cc, -sc, z], [sc, cc, z], [z, z, o]]

    def mul(A, B):
        M = [[z] * 3 for _ in range(3)]
        for i in range(3):
            for j in range(3):
                s = F(0)
                for k in range(3):
                    s = F(s + F(A[i][k] * B[k][j]))
                M[i][j] = s
        return M
    T = np.asarray(T, dtype=F)
    R = mul(mul(Rz, Ry), Rx)
    out = np.array(T, dtype=F)
    out[:3, :3] = np.array(mul(R, [[T[i, j] for j in range(3)] for i in range(3)]), dtype=F)
    for i in range(3):
        out[i, 3] = F(T[i, 3] + F(x[i]))
    return out


def cofactor_inverse(T):
    """The symmetric 3x3 inverse by cofactors (what a device does), vectorised."""
    a = T
    c00 = a[:, 1, 1] * a[:, 2, 2] - a[:, 1, 2] * a[:, 1, 2]
    c01 = a[:, 0, 2] * a[:, 1, 2] - a[:, 0, 1] * a[:, 2, 2]
    c02 = a[:, 0, 1] * a[:, 1, 2] - a[:, 0, 2] * a[:, 1, 1]
    det = a[:, 0, 0] * c00 + a[:, 0, 1] * c01 + a[:, 0, 2] * c02
    o = np.empty_like(a)
    o[:, 0, 0] = c00 / det; o[:, 0, 1] = o[:, 1, 0] = c01 / det; o[:, 0, 2] = o[:, 2, 0] = c02 / det
    o[:, 1, 1] = (a[:, 0, 0] * a[:, 2, 2] - a[:, 0, 2] ** 2) / det
    o[:, 1, 2] = o[:, 2, 1] = (a[:, 0, 1] * a[:, 0, 2] - a[:, 0, 0] * a[:, 1, 2]) / det
    o[:, 2, 2] = (a[:, 0, 0] * a[:, 1, 1] - a[:, 0, 1] ** 2) / det
    return o


XS = (np.zeros(6), np.array([0.05, -0.02, 0.01, 0.0, 0.0, 0.0]), np.array([-0.1, 0.03, 0.02, 0.002, -0.003, 0.004]))
NEAREST_MARGIN = Q * Q          # the second nearest target is at least this much farther (squared), asserted


@dataclass
class FunctorCase:
    name: str
    src: np.ndarray              # [ns, 3] float32 lattice
    tgt: np.ndarray              # [nt, 3] float32 lattice
    guess: np.ndarray            # [4, 4] float32, exact on the lattice
    k: int = 20
    threshold: float = 0.5
    planes: tuple | None = None  # (source normal, target normal) when both clouds are flat: the covariances need no neighbour sets
    notes: dict = field(default_factory=dict)


def plane_covariances(n, normal, eps=EPS):
    u = np.asarray(normal, dtype=np.float64)
    return np.broadcast_to(np.eye(3) - (1.0 - eps) * np.outer(u, u), (n, 3, 3)).copy()


def case_covariances(case: FunctorCase, method="eigh", fsum=False):
    if case.planes is not None:
        return plane_covariances(len(case.src), case.planes[0]), plane_covariances(len(case.tgt), case.planes[1])
    out = []
    for pts in (case.src, case.tgt):
        idx, _ = _order_of(pts)
        out.append(covariances(pts, idx[:, :case.k], method=method, fsum=fsum)[0])
    return tuple(out)


_ORDERS = {}


def _order_of(pts):
    key = (pts.shape, pts.tobytes())
    if key not in _ORDERS:
        _ORDERS[key] = neighbour_order(pts)
    return _ORDERS[key]


def correspondences(case: FunctorCase):
    """Per source point the nearest target of its transformed position (exact squared distances), the gap to the second
    nearest, and the kept mask d2 < threshold^2."""
    q = transform_f32(case.src, case.guess).astype(np.float64)
    t = case.tgt.astype(np.float64)
    _, j2 = cKDTree(t).query(q, k=2)
    d = ((q[:, None, :] - t[j2]) ** 2).sum(axis=2)           # exact on the lattice
    sw = d[:, 1] < d[:, 0]
    j = np.where(sw, j2[:, 1], j2[:, 0])
    dmin, dsec = d.min(axis=1), d.max(axis=1)
    thr2 = float(F(case.threshold * case.threshold))
    return j, dmin, dsec - dmin, dmin.astype(F) < F(thr2)


class FunctorRef:
    """The functor over the first outer iteration's correspondences (transformation_ = I), in float64."""

    def __init__(self, case: FunctorCase, alt=False):
        self.case = case
        j, d2, gap, keep = correspondences(case)
        self.j, self.d2, self.gap, self.keep = j, d2, gap, keep
        self.m = int(keep.sum())
        Cs, Ct = case_covariances(case, method="svd" if alt else "eigh", fsum=alt)
        R = case.guess[:3, :3].astype(np.float64)
        Tm = R[None] @ Cs[keep] @ R.T[None] + Ct[j[keep]]
        self.maha = cofactor_inverse(Tm) if alt else (np.linalg.inv(Tm) if self.m else Tm)
        self.src = case.src[keep]
        self.tgt = case.tgt[j[keep]]
        self.pbase = transform_f32(self.src, case.guess).astype(np.float64)

    def evaluate(self, x, mode="nofma", pp=None):
        """(values[7], A[7], pp): f and the gradient, the sums of their absolute addends, the transformed points."""
        x = np.asarray(x, dtype=np.float64)
        if pp is None:
            pp = transform_f32(self.src, apply_state_f32(self.case.guess, x), mode)
        m = float(self.m)
        res = (pp - self.tgt).astype(F).astype(np.float64)
        terms = self.maha * res[:, None, :]                  # [m, a, b] = M_ab r_b
        temp = terms.sum(axis=2)
        atemp = np.abs(terms).sum(axis=2)
        vals = np.zeros(7); A = np.zeros(7)
        vals[0] = (res * temp).sum() / m
        A[0] = np.abs(res[:, :, None] * terms).sum() / m
        vals[1:4] = temp.sum(axis=0) * (2.0 / m)
        A[1:4] = atemp.sum(axis=0) * (2.0 / m)
        Rm = (self.pbase[:, :, None] * temp[:, None, :]).sum(axis=0) * (2.0 / m)
        Ra = (np.abs(self.pbase)[:, :, None] * atemp[:, None, :]).sum(axis=0) * (2.0 / m)
        vals[4:] = ong.r_derivative(x, Rm)
        for a in range(3):                                   # the rotational entries are linear in R
            for b in range(3):
                E = np.zeros((3, 3)); E[a, b] = 1.0
                A[4:] += np.abs(ong.r_derivative(x, E)) * Ra[a, b]
        return vals, A, pp

    def reference(self, x):
        """(values[7], S[7]) with S = 2^-53 A + N."""
        vals, A, pp = self.evaluate(x)
        N = np.zeros(7)
        if np.any(np.asarray(x) != 0):
            for t in range(16):
                rng = np.random.default_rng(9000 + t)
                step = rng.integers(-1, 2, size=pp.shape)
                moved = np.where(step > 0, np.nextafter(pp, F(np.inf)), np.where(step < 0, np.nextafter(pp, F(-np.inf)), pp)).astype(F)
                N = np.maximum(N, np.abs(self.evaluate(x, pp=moved)[0] - vals))
        return vals, U53 * A + N


def functor_ratio(got7, vals, S):
    diff = np.abs(np.asarray(got7, dtype=np.float64) - vals)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0, 0.0, diff / S)
    c = int(np.argmax(r))
    return float(r[c]), c


# ---- the functor cases -------------------------------------------------------------------------
F_STEP = 1.25                                   # target spacing: an offset of 0.5 m along an axis has one nearest target
IN_OFF = np.array([(7, 0, 0), (0, -7, 0), (3, 2, 1), (-2, 5, -1), (1, 1, 0), (-4, -4, 2), (0, 0, 3), (5, -4, 0)]) * Q      # d2 < 0.25
AT_OFF = np.array([(8, 0, 0), (0, 8, 0), (0, 0, 8)]) * Q                                                                    # d2 = 0.25 exactly
OUT_OFF = np.array([(9, 0, 0), (0, -9, 0), (6, 6, 0), (0, 3, 9)]) * Q                                                       # d2 > 0.25
G_TRANS = (0.5, -0.25, 0.125)


@functools.lru_cache(maxsize=None)
def functor_target(flat=False):
    return height_field(64, 64, F_STEP, 21, flat=flat)


def _to_source(q, guess):
    G = guess.astype(np.float64)
    return ((np.asarray(q, dtype=np.float64) - G[:3, 3]) @ G[:3, :3]).astype(F)          # R^T (q - t): exact on the lattice


def _closing_triple(tgt, centre, rng, cands):
    """Three positions beyond the gate, each with one nearest target, that sum to three times `centre`."""
    tree = cKDTree(tgt.astype(np.float64))
    for _ in range(10000):
        a = tgt[rng.integers(len(tgt))] + cands[rng.integers(len(cands))]
        b = tgt[rng.integers(len(tgt))] + cands[rng.integers(len(cands))]
        c = 3.0 * centre - a - b
        if np.abs(c).max() >= 60:
            continue
        d, _ = tree.query(np.stack([a, b, c]), k=2)
        if (d[:, 0] ** 2 > 0.3).all() and (d[:, 1] ** 2 - d[:, 0] ** 2 > 4 * NEAREST_MARGIN).all():
            return np.stack([a, b, c])
    raise AssertionError("no closing triple")


def make_source(tgt, mirror, ns, guess, pattern, seed, offsets=None):
    """ns transformed positions around target points, point-symmetric about the target's centre (pairs of mirrored targets with
    opposite offsets; an odd ns closes with three unmatched points), mapped back through the guess.  pattern: 'all' kept,
    'mix' (inside / exactly at / beyond the gate), 'four' (two pairs kept), 'blocks' (kept only where x y > 0), 'none'."""
    rng = np.random.default_rng(seed)
    t = tgt.astype(np.float64)
    centre = np.array([0.0, 0.0, (t[:, 2].max() + t[:, 2].min()) / 2])
    half = np.flatnonzero(np.arange(len(t)) < mirror)            # one of every mirrored pair
    npairs = (ns - (3 if ns % 2 else 0)) // 2
    reps = -(-npairs // len(half))
    inn, at, out = (IN_OFF, AT_OFF, OUT_OFF) if offsets is None else offsets
    pos = []
    used = set()
    order = np.concatenate([rng.permutation(half) for _ in range(reps)])[:npairs]
    for n, j in enumerate(order):
        if pattern == "all":
            pool = inn
        elif pattern == "none":
            pool = np.concatenate([at, out])
        elif pattern == "four":
            pool = inn if n < 2 else np.concatenate([at, out])
        elif pattern == "blocks":
            pool = np.concatenate([inn, at]) if t[j, 0] * t[j, 1] > 0 else out
        else:
            pool = np.concatenate([inn, at, out])
        for _ in range(100):
            o = pool[rng.integers(len(pool))]
            if (int(j), tuple(o)) not in used:
                break
        else:
            raise AssertionError("offsets exhausted")
        used.add((int(j), tuple(o)))
        pos.append(t[j] + o)
        pos.append(t[mirror[j]] - o)
    if ns % 2:
        pos.extend(_closing_triple(t, centre, rng, out))
    pos = np.array(pos)
    pos = pos[rng.permutation(len(pos))]
    assert len(pos) == ns
    return _to_source(pos, guess)


FUNCTOR_CASES = (
    # name, ns, rotate, pattern
    ("ns20/all/t", 20, False, "all"), ("ns255/mix/r", 255, True, "mix"), ("ns256/mix/t", 256, False, "mix"),
    ("ns257/mix/r", 257, True, "mix"), ("ns257/mix/t", 257, False, "mix"), ("ns4097/all/r", 4097, True, "all"),
    ("ns4097/four/t", 4097, False, "four"), ("ns4097/blocks/r", 4097, True, "blocks"), ("ns4097/blocks/t", 4097, False, "blocks"),
    ("ns4097/none/r", 4097, True, "none"),
)
BIG_NS = 262144 + 1                             # the smallest ns with ceil(ns / 256) > 1024: nblk is capped, a second grid-stride trip


@functools.lru_cache(maxsize=None)
def functor_case(name):
    if name == "big":
        tgt, mirror = functor_target(flat=True)
        guess = guess_matrix((0.5, -0.25, 0.0), True)
        ab = [(a, b) for a in range(-9, 10) for b in range(-9, 10)]
        sel = np.random.default_rng(31).permutation(len(ab))[:80]
        offs = np.array([(ab[i][0], ab[i][1], 0) for i in sel] + [(8, 0, 0), (0, 8, 0), (0, -8, 0)]) * Q
        d2 = (offs ** 2).sum(axis=1)
        offsets = (offs[d2 < 0.25], offs[d2 == 0.25], offs[d2 > 0.25])
        src = make_source(tgt, mirror, BIG_NS, guess, "mix", 32, offsets)
        # both clouds are flat: the target in z = 0, the source in the plane the guess maps onto it
        n_src = PERM.T @ np.array([0.0, 0.0, 1.0])
        return FunctorCase(name, src, tgt, guess, planes=(n_src, (0.0, 0.0, 1.0)))
    spec = {c[0]: c for c in FUNCTOR_CASES}[name]
    tgt, mirror = functor_target()
    guess = guess_matrix(G_TRANS, spec[2])
    src = make_source(tgt, mirror, spec[1], guess, spec[3], 40 + FUNCTOR_CASES.index(spec))
    return FunctorCase(name, src, tgt, guess)


# ---- covariances on demand -----------------------------------------------------------------------
LAZY_OFF = np.array([(1, 0, 0), (0, 1, 0), (-1, 0, 1), (0, -1, -1), (1, 1, 0)]) * Q
LAZY_SHIFT = (0.25, 0.0, 0.0)                   # the second batch's guess: every source point meets the next column's target


@functools.lru_cache(maxsize=None)
def _lazy_source():
    tgt, mirror = height_field(64, 32, 0.25, TIES_SEED)
    t = tgt.astype(np.float64)
    rng = np.random.default_rng(51)
    tree = cKDTree(t)
    patch = np.flatnonzero((np.abs(t[:, 0]) < 2.5) & (np.abs(t[:, 1]) < 2.0) & (np.arange(len(t)) < mirror))

    def unique_under_both(pos):                  # one nearest target under the first guess and under the shifted one
        for sh in ((0.0, 0.0, 0.0), LAZY_SHIFT):
            d, _ = tree.query(np.asarray(pos) + np.array(sh), k=2)
            if not (d[:, 1] ** 2 - d[:, 0] ** 2 >= 2 * NEAREST_MARGIN).all():
                return False
        return True
    pos, triple = [], False
    for j in patch:
        for offs in ([LAZY_OFF[:3]] if not triple else []) + [LAZY_OFF[rng.integers(len(LAZY_OFF))][None]]:
            cand = [p for o in offs for p in (t[j] + o, t[mirror[j]] - o)]
            if unique_under_both(cand):
                pos.extend(cand)
                triple = triple or len(offs) == 3
                break
    assert triple
    if len(pos) % 64 == 0:
        pos = pos[:-2]
    pos = np.array(pos)
    return tgt, pos[rng.permutation(len(pos))]


@functools.lru_cache(maxsize=None)
def lazy_case(second=False):
    """Job 0 of the on-demand batch: the ties cloud as target; a patch of it with small offsets as source (only positions with
    one nearest target under both guesses), three source points on each of two targets, a count that is no multiple of 64."""
    tgt, pos = _lazy_source()
    src = _to_source(pos, guess_matrix(G_TRANS, True))
    guess = guess_matrix(np.array(G_TRANS) + (np.array(LAZY_SHIFT) if second else 0.0), True)
    return FunctorCase("lazy/second" if second else "lazy/first", src, tgt, guess, threshold=0.5)


def small_pair(seed):
    """A small lattice pair for the other jobs of the batch: (source, target, guess)."""
    tgt, _ = height_field(16, 16, 0.25, seed)
    guess = guess_matrix((0.25, 0.5, -0.125), False)
    src = _to_source(tgt.astype(np.float64) + np.array([Q, 0.0, Q]), guess)
    return src, tgt, guess


def measure_rho_f(names):
    worst = 0.0
    for name in names:
        case = functor_case(name) if not name.startswith("lazy") else lazy_case(name.endswith("second"))
        ref, alt = FunctorRef(case), FunctorRef(case, alt=True)
        if ref.m == 0:
            continue
        for x in XS:
            vals, S = ref.reference(x)
            for got in (ref.evaluate(x, "fma")[0], ref.evaluate(x, "blas")[0], alt.evaluate(x)[0]):
                worst = max(worst, functor_ratio(got, vals, S)[0])
    return worst


RHO_F_CASES = tuple(c[0] for c in FUNCTOR_CASES) + ("lazy/first", "lazy/second")
