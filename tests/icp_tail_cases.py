"""The cases that pin the serial end of an IcpFast iteration (staticmapping_amd/csrc/icp_tail_math.h), shared by the reference
tests (test_icp_tail_ref.py), the host program (test_icp_tail_cpp.py) and the device tests (test_icp_tail_gpu.py).

numpy only.  Every scene lies on a 0.25 m lattice whose coordinates are odd multiples of 2^-3 (so multiples of 2^-6) and
symmetric about the origin: the target mean is exactly zero and the device's float centring is exact.  Normals are given, and are
float32 values, as are the source points: what the device stores is what the reference reads.
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
EPSILONS = (1e-3, 1e-5, 3e-6, 1e-6, 3e-7, 1e-8)


# ---------------------------------------------------------------------------------------------- scenes
def _axis(n):
    """n lattice coordinates, symmetric: (k + 0.5) * 0.25."""
    return (np.arange(-n // 2, n // 2) + 0.5) * 0.25


def _plane(axis, value, na, nb, normal_sign=1.0):
    a, b = np.meshgrid(_axis(na), _axis(nb), indexing="ij")
    o = [i for i in range(3) if i != axis]
    p = np.zeros((a.size, 3))
    p[:, o[0]] = a.ravel(); p[:, o[1]] = b.ravel(); p[:, axis] = value
    n = np.zeros((a.size, 3)); n[:, axis] = normal_sign
    return p, n


def _join(parts):
    return np.concatenate([p for p, _ in parts]), np.concatenate([n for _, n in parts])


def make_pose(rotvec=(0, 0, 0), t=(0, 0, 0)):
    v = np.asarray(rotvec, dtype=np.float64)
    ang = float(np.linalg.norm(v))
    T = np.eye(4)
    if ang > 0:
        k = v / ang
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        T[:3, :3] = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    T[:3, 3] = t
    return T


MOTION = make_pose((0.0011, -0.0017, 0.0013), (0.011, -0.017, 0.013))      # 0.0024 rad, 0.024 m
# The eps-corridors move by a translation alone, of multiples of 2^-10: the source is then exact in float and the residuals are
# exactly linear in the step, so b is consistent and the weak direction's 1 / lambda amplifies no rounding and no second-order term
# (with MOTION, 1e-5 m of second-order residual over eps = 1e-6 is a 10 m slide along the corridor, and no neighbour is certain).
MOTION_EPS = make_pose(t=(11 / 1024, -17 / 1024, 13 / 1024))                # 0.024 m


def scene(name):
    """-> dict(target [N,3] f64, normals [N,3] f64 (float32 values), source [N,3] f32, motion 4x4, rank)"""
    if name == "box":
        parts = [_plane(2, -1.5, 20, 20), _plane(2, 1.5, 20, 20, -1.0), _plane(0, -2.5, 20, 12), _plane(0, 2.5, 20, 12, -1.0),
                 _plane(1, -2.5, 20, 12), _plane(1, 2.5, 20, 12, -1.0)]
        rank = 6
    elif name == "plane":
        parts = [_plane(2, 0.0, 40, 40)]
        rank = 3
    elif name == "two_planes":
        parts = [_plane(2, -1.5, 28, 28), _plane(2, 1.5, 28, 28, -1.0)]
        rank = 3
    elif name == "corridor" or name.startswith("eps_corridor"):
        parts = [_plane(2, -1.5, 32, 12), _plane(2, 1.5, 32, 12, -1.0), _plane(1, -1.5, 32, 12), _plane(1, 1.5, 32, 12, -1.0)]
        rank = 5
    else:
        raise KeyError(name)
    tgt, nrm = _join(parts)
    motion = MOTION
    if name.startswith("eps_corridor"):
        e = float(name.split(":")[1])
        # a quarter of the floor (the first plane: x > 0, y > 0) leans by e toward x, the axis nothing else holds
        q = (np.arange(len(tgt)) < 32 * 12) & (tgt[:, 0] > 0) & (tgt[:, 1] > 0)
        nrm[q, 0] = np.sin(e); nrm[q, 2] = np.cos(e)
        rank = None
        motion = MOTION_EPS
    nrm = nrm.astype(np.float32).astype(np.float64)
    inv = np.linalg.inv(motion)
    src = (tgt @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    return dict(name=name, target=tgt, normals=nrm, source=src, motion=motion, rank=rank)


SCENES = ["box", "plane", "two_planes", "corridor"] + [f"eps_corridor:{e:g}" for e in EPSILONS]


def z_shift_plane(shift=0.015625):
    """The single plane with the source a pure z-shift (2^-6: exact in float) of it: x[0:3] is exactly zero."""
    s = scene("plane")
    s["source"] = (s["target"] + np.array([0.0, 0.0, shift])).astype(np.float32)
    s["motion"] = make_pose(t=(0, 0, -shift))
    s["shift"] = shift
    return s


def box_ratio_07():
    """The box whose source rows are pushed along their own plane's normal by offsets in three groups -- most small, a few in steps of 1 mm round the quantile's
    rank, the rest large --: the d^2 round the 0.7 quantile's rank are far apart (asserted on the CPU by the tests)."""
    s = scene("box")
    n = len(s["target"])
    rng = np.random.default_rng(7)
    k = int(n * float(np.float32(0.7)))                               # the quantile's rank (GetDistsQuantile)
    off = np.concatenate([rng.uniform(0.005, 0.010, k - 2), [0.0120, 0.0130, 0.0140, 0.0150, 0.0160], rng.uniform(0.018, 0.025, n - k - 3)])
    rng.shuffle(off)
    s["source"] = (s["target"] + off[:, None] * np.abs(s["normals"])).astype(np.float32)
    s["motion"] = None
    return s


def nn_bruteforce(P, Q):
    """f64 brute force: ids, d2 of the nearest and d2 of the runner-up, for every row of P."""
    ids = np.empty(len(P), np.int64); d1 = np.empty(len(P)); d2nd = np.empty(len(P))
    for a in range(0, len(P), 512):
        D = ((P[a:a + 512, None, :] - Q[None, :, :]) ** 2).sum(-1)
        o = np.argpartition(D, 1, axis=1)[:, :2]
        da = np.take_along_axis(D, o, 1)
        sw = da[:, 0] > da[:, 1]
        o[sw] = o[sw][:, ::-1]; da[sw] = da[sw][:, ::-1]
        ids[a:a + 512] = o[:, 0]; d1[a:a + 512] = da[:, 0]; d2nd[a:a + 512] = da[:, 1]
    return ids, d1, d2nd


# ---------------------------------------------------------------------------------------------- the 6x6 ladder
def _orth(rng, n=6):
    Q, R = np.linalg.qr(rng.standard_normal((n, n)))
    return Q * np.sign(np.diag(R))


def ladder():
    """-> list of dict(name, A 6x6, b 6, x0 6, lam): symmetric PSD A = Q diag(lam) Q^T and b = A x0 (consistent up to rounding).
    `dense` rungs have a seeded orthogonal Q; `diag` rungs a seeded signed permutation, whose A holds lam exactly (a dense f64
    matrix cannot hold a ratio below ~1e-16: its rounding is of that size)."""
    rng = np.random.default_rng(20240611)
    out = []

    def add(name, Q, lam):
        lam = np.asarray(lam, dtype=np.float64)
        A = (Q * lam) @ Q.T
        A = 0.5 * (A + A.T)
        x0 = rng.uniform(-1, 1, 6)
        out.append(dict(name=name, A=A, b=A @ x0, x0=x0, lam=lam))

    def perm():
        P = np.eye(6)[rng.permutation(6)]
        return P * rng.choice([-1.0, 1.0], 6)

    for r in range(7):                                               # ranks 0..6 with exact zeros
        lam = np.concatenate([rng.uniform(1.0, 100.0, r), np.zeros(6 - r)])
        add(f"rank{r}:dense", _orth(rng), lam)
        add(f"rank{r}:diag", perm(), lam)
    for k in range(0, 37):                                           # lam_min / lam_max = 10^(-k/2), k/2 = 0 .. 18
        ratio = 10.0 ** (-0.5 * k)
        mid = 10.0 ** rng.uniform(np.log10(max(ratio, 1e-3)), 0.0, 4)
        scale = 10.0 ** rng.uniform(-3, 6)
        lam = scale * np.concatenate([[1.0], mid, [ratio]])
        add(f"full:1e-{0.5 * k:g}:dense", _orth(rng), lam)
        add(f"full:1e-{0.5 * k:g}:diag", perm(), lam)
    return out


def special_matrices():
    """Non-finite and all-zero A (name, A, b)."""
    rng = np.random.default_rng(5)
    A = _orth(rng); A = A @ np.diag([1, 2, 3, 4, 5, 6.0]) @ A.T
    b = rng.uniform(-1, 1, 6)
    out = [("zero", np.zeros((6, 6)), b)]
    for nm, v in (("nan_diag", np.nan), ("inf_diag", np.inf)):
        B = A.copy(); B[2, 2] = v; out.append((nm, B, b))
    B = A.copy(); B[1, 4] = B[4, 1] = np.nan; out.append(("nan_off", B, b))
    B = A.copy(); b2 = b.copy(); b2[3] = np.nan; out.append(("nan_rhs", B, b2))
    return out


# ---------------------------------------------------------------------------------------------- rotations
def rotations():
    """(name, R 3x3) for quat_from_rot: the listed angles about five axes, and matrices that make each branch the chosen one."""
    axes = {"x": (1, 0, 0), "y": (0, 1, 0), "z": (0, 0, 1), "o1": (1, 2, 3), "o2": (-2, 1, 0.5)}
    out = []
    for an, ax in axes.items():
        ax = np.asarray(ax, dtype=np.float64); ax /= np.linalg.norm(ax)
        for deg in (0.0, 90.0, 119.0, 121.0, 179.9, 180.0):
            out.append((f"{an}:{deg:g}", make_pose(ax * np.deg2rad(deg))[:3, :3]))
    # trace <= 0 with each diagonal entry the largest, and the exact ties the `>=` of the branches decide
    d = lambda a, b, c: np.diag([float(a), float(b), float(c)])
    out += [("pi_x", d(1, -1, -1)), ("pi_y", d(-1, 1, -1)), ("pi_z", d(-1, -1, 1)),
            ("tie_xy", make_pose(np.array([1.0, 1.0, 0.0]) / np.sqrt(2) * np.pi)[:3, :3]),
            ("tie_yz", make_pose(np.array([0.0, 1.0, 1.0]) / np.sqrt(2) * np.pi)[:3, :3]),
            ("tie_xyz", make_pose(np.array([1.0, 1.0, 1.0]) / np.sqrt(3) * np.pi)[:3, :3])]
    T = np.array([[0.0, 1, 0], [1, 0, 0], [0, 0, -1]])                # r00 == r11 == 0 exactly, r22 = -1: pi about (1, 1, 0)
    out.append(("tie_exact_00_11", T))
    T = np.array([[-1.0, 0, 0], [0, 0, 1], [0, 1, 0]])                # r11 == r22 == 0 exactly
    out.append(("tie_exact_11_22", T))
    out.append(("trace_zero_120", np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]])))   # trace exactly 0: not the first branch
    return out


def potential_pairs(n=2000):
    """(M_old, M_new) 3x4 f64 pairs: relative angles log-uniform in [1e-12, 3] rad; every second pair is a product of 50 f64
    rotations (slightly non-orthogonal)."""
    rng = np.random.default_rng(99)
    out = []
    for i in range(n):
        if i % 2:
            R = np.eye(3)
            for _ in range(50):
                R = make_pose(rng.standard_normal(3))[:3, :3] @ R
        else:
            R = make_pose(rng.standard_normal(3) * rng.uniform(0, 2))[:3, :3]
        ang = 10.0 ** rng.uniform(-12, np.log10(3.0))
        ax = rng.standard_normal(3); ax /= np.linalg.norm(ax)
        if i % 7 == 0:
            ax = np.eye(3)[i % 3]                                     # axis-aligned steps: two equal singular values, exactly
        dR = make_pose(ax * ang)[:3, :3]
        t0 = rng.uniform(-50, 50, 3)
        dt = rng.standard_normal(3) * 10.0 ** rng.uniform(-9, 0)
        M0 = np.hstack([R, t0[:, None]])
        M1 = np.hstack([dR @ R, (dR @ t0 + dt)[:, None]])
        out.append((M0, M1))
    return out


def get_scene(name):
    """Every scene by name: SCENES, and `z_shift`, `box07`, `identical_box`, `box_offset` (the box from a 0.03 m offset)."""
    if name == "z_shift":
        return z_shift_plane()
    if name == "box07":
        return box_ratio_07()
    if name == "identical_box":
        s = scene("box"); s["source"] = s["target"].astype(np.float32); s["motion"] = np.eye(4)
        return s
    if name == "box_offset":
        s = scene("box")
        t = np.array([0.02, -0.02, 0.01])                           # |t| = 0.03
        s["source"] = (s["target"] - t).astype(np.float32); s["motion"] = make_pose(t=t)
        return s
    return scene(name)
