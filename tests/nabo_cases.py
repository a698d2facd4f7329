"""The fixtures of tests/test_nabo_exact_gpu.py, built with numpy alone so that tests/test_nabo_ref.py can check on the CPU what
the GPU tests rely on: that the lattice fixtures satisfy nabo_ref.check_lattice, that the off-lattice ones are decidable but for a
small share, and that the queries are sharp enough to tell six wrong walks from the right one.

Lattice clouds: every target coordinate is OFFSET + an even multiple of the quantum Q, every query coordinate OFFSET + a multiple
of Q (the midpoint of two target points is a query), and every cloud is point-symmetric about OFFSET, so its mean is OFFSET exactly
in whatever order the device adds."""
import numpy as np

from tests import nabo_ref

Q = 0.5
OFFSET = np.array([12.0, -7.0, 3.0])
LATTICE_EPS = (0.0, 1.0, 3.0)                 # (1 + eps)^2 = 1, 4, 16
TREE_SIZES = (1, 8, 9, 16, 17, 33, 64, 65, 1023, 1024, 1025, 4097)
QUERY_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1025)
VELO_TAKE = slice(0, None, 5)                 # the queries of the 20 k scan pair the reference walks (4 000 of them)
SHALLOW_MAX = 8 << 12                         # the largest target the 12-level stack instantiation takes (icp_plan.h)
SEGMENT_THRESHOLD = 69633                     # smallest cloud with a level of more than kKdHistWords / 2 segments (asserted on the CPU)
DEEP_SIZES = (SHALLOW_MAX + 1, SEGMENT_THRESHOLD)
TWO_BIT_SIZE = 8192 * 64 + 1                  # a level of 8 192 segments one of which holds 65 points: more than a wave ranks by counting
ONE_BIT_SIZE = 16384 * 64 + 1                # a level of 16 384 such segments: 1-bit digits, fill counters in global memory


def kd_hist_words():
    """kKdHistWords as csrc/kd_median_tree.h states it"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "staticmapping_amd", "csrc", "kd_median_tree.h")).read()
    return int(re.search(r"constexpr int kKdHistWords = (\d+);", text).group(1))


def _symmetric(P, n, rng):
    """n points: the integer rows P, their mirror images and, for odd n, the centre; shuffled; as raw float32 coordinates"""
    P = np.asarray(P, dtype=np.int64).reshape(-1, 3)[: n // 2]
    rows = [P, -P] + ([np.zeros((1, 3), np.int64)] if n % 2 else [])
    c = np.concatenate(rows)
    assert len(c) == n
    c = c[rng.permutation(n)]
    return (c * (2 * Q) + OFFSET).astype(np.float32)


def latin(n, seed=1):
    """tie-free: on every axis the n coordinates are distinct"""
    rng = np.random.default_rng(seed)
    h = n // 2
    P = np.stack([rng.permutation(h) + 1 for _ in range(3)], axis=1) * rng.choice([-1, 1], size=(h, 3))
    return _symmetric(P, n, rng)


def coarse(n, seed=2):
    """a coarse lattice: 13 x 11 x 5 distinct places, so every median is tied and most points have exact duplicates"""
    rng = np.random.default_rng(seed)
    return _symmetric(rng.integers([-6, -5, -2], [7, 6, 3], size=(n // 2, 3)), n, rng)


def duplicates(n, seed=3):
    """exact duplicates, some threefold and more, of otherwise spread points"""
    rng = np.random.default_rng(seed)
    h = n // 2
    base = rng.integers(-40, 41, size=(h // 2 + 1, 3))
    return _symmetric(base[rng.integers(0, len(base), size=h)], n, rng)


def plane(n, seed=4):
    rng = np.random.default_rng(seed)
    P = rng.integers(-30, 31, size=(n // 2, 3)); P[:, 2] = 0
    return _symmetric(P, n, rng)


def line(n, seed=5):
    rng = np.random.default_rng(seed)
    P = rng.integers(-50, 51, size=(n // 2, 3)); P[:, 1:] = 0
    return _symmetric(P, n, rng)


LATTICE_CLOUDS = dict(latin=latin, coarse=coarse, duplicates=duplicates, plane=plane, line=line)


def tree_stage_cases():
    """(cloud, size) of the lattice clouds the tree stage builds: the tie-free one up to 1 025 points (beyond, its squared
    distances leave the range float32 holds exactly)"""
    return [(name, n) for name in LATTICE_CLOUDS for n in TREE_SIZES if not (name == "latin" and n > 1025)]


def normal_cloud(n, seed=11):
    """the large targets: a seeded normal cloud, tie-free on every axis (asserted)"""
    rng = np.random.default_rng(seed)
    t = untie((rng.normal(0, 1, (n, 3)) * [40, 30, 2.0]).astype(np.float32))
    assert tie_free(t)
    return t


def normal_cloud_with_ties(n, seed=13):
    """the same draw left as float32 made it: some 7 500 coordinates per axis repeat (the million-point target, checked by the rules)"""
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, (n, 3)) * [40, 30, 2.0]).astype(np.float32)


def untie(t):
    """float32 draws of tens of thousands of points repeat a coordinate here and there: the later of two equal coordinates
    moves to the next float up until every axis is tie-free"""
    t = np.array(t, dtype=np.float32)
    for d in range(3):
        while True:
            _, first = np.unique(t[:, d], return_index=True)
            if len(first) == len(t):
                break
            again = np.ones(len(t), bool); again[first] = False
            t[again, d] = np.nextafter(t[again, d], np.float32(np.inf))
    return t


def normal_queries(n=4096, seed=12):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, (n, 3)) * [42, 31, 2.2]).astype(np.float32)


BATCH_SLOTS, BATCH_NS, BATCH_CHECKED = 32, 7700, (0, 13, 31)


STRIDED_SHIFT = 0.25          # extra forward offset of the guesses where most queries are to be walked again


def batch_case(nt, shift=0.0):
    """(target, its normals, source, guesses) of the Align cases: a scan of the same scene -- a sample of the target with a centimetre of
    noise -- under 32 small poses (`shift` metres further off along x)"""
    from staticmapping_amd import synth
    t = normal_cloud(nt)
    rng = np.random.default_rng(21)
    src = (t[rng.choice(nt, BATCH_NS, replace=False)] + rng.normal(0, 0.01, (BATCH_NS, 3))).astype(np.float32)
    guesses = [synth.make_pose(t=(shift + 0.05 + 0.01 * (k % 5), 0.02 * (k % 3), 0.0), rpy_deg=(0, 0, 0.1 * (k % 4))) for k in range(BATCH_SLOTS)]
    nrm = rng.normal(size=(nt, 3))                   # normals in every direction: the point-to-plane step sees the whole offset
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return t, nrm, src, guesses


def tie_free(points):
    p = np.asarray(points)
    return all(len(np.unique(p[:, d])) == len(p) for d in range(3))


def lattice_queries(target, count=1025, seed=7):
    """Raw float32 queries for a lattice target, the special rows first: NaN / Inf rows (3), one 1 km away, outside the root box
    on each of its six faces, ON cut planes (and one quantum to either side), on target points, equidistant from the first two
    entries of buckets, then seeded lattice points in and around the box up to `count` rows."""
    rng = np.random.default_rng(seed)
    tgt = np.asarray(target, dtype=np.float32)
    c = np.round((tgt.astype(np.float64) - OFFSET) / Q).astype(np.int64)          # centred, in quanta
    nodes, order = nabo_ref.build((c * Q).astype(np.float32))
    lo, hi = c.min(axis=0), c.max(axis=0)
    mid = ((lo + hi) // 2)
    rows = []
    for d in range(3):                                                              # outside the box, each face
        for v in (lo[d] - 3, hi[d] + 5):
            r = rng.integers(lo, hi + 1); r[d] = v; rows.append(r)
            r = mid.copy(); r[d] = v; rows.append(r)
    inner = [v for v in range(len(nodes)) if (nodes[v, 1] & 3) != 3]
    for v in (inner[:40] + inner[-40:]):                                            # on cut planes and beside them
        cd = int(nodes[v, 1] & 3)
        cut = int(round(float(nodes[v, 0:1].view(np.float32)[0]) / Q))
        base = c[rng.integers(0, len(c))].copy()
        for dv in (0, -1, 1):
            r = base.copy(); r[cd] = cut + dv; rows.append(r)
    for k in rng.integers(0, len(c), size=64):                                      # on target points
        rows.append(c[k])
    leaves = [v for v in range(len(nodes)) if (nodes[v, 1] & 3) == 3 and (nodes[v, 1] >> 2) >= 2]
    for v in (leaves[:40] + leaves[-40:]):                                          # equidistant from two bucket entries
        f = int(nodes[v, 0])
        rows.append((c[order[f]] + c[order[f + 1]]) // 2)                           # (targets sit on even quanta)
    rows = np.array(rows, dtype=np.int64).reshape(-1, 3)
    fill = max(0, count - 4 - len(rows))
    rows = np.concatenate([rows, rng.integers(lo - 4, hi + 5, size=(fill, 3))])
    q = np.empty((4 + len(rows), 3), np.float32)
    q[4:] = (rows * Q + OFFSET).astype(np.float32)
    q[0] = (np.nan, OFFSET[1], OFFSET[2]); q[1] = (OFFSET[0], np.inf, OFFSET[2]); q[2] = (OFFSET[0], OFFSET[1], -np.inf)
    q[3] = OFFSET + (1000.0, 0.0, 0.0)
    return q[:count] if count < len(q) else q


def walk_fixtures():
    """(name, raw float32 target, raw float32 queries) of the lattice fixtures the walk stage runs"""
    out = []
    for name, n in (("latin", 1025), ("coarse", 1025), ("duplicates", 1024), ("plane", 1023), ("line", 65),
                    ("latin", 1), ("coarse", 8), ("latin", 9), ("duplicates", 17)):
        t = LATTICE_CLOUDS[name](n)
        out.append((f"{name}{n}", t, lattice_queries(t, 1025 if n == 1025 and name == "latin" else 400)))
    return out
