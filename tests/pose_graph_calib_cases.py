"""Graphs with odometry (HANDEYE) factors shared by the CPU, C++ and device tests, all against tests/pose_graph_calib_ref.py.  Fixed
ingredients: pose_graph_ref.circle_drive re-based so that the truth's node 0 is the identity (the factor's model assumes that the
first odometer reading is taken there); the true calibration T_TRUE; Z_k = T_TRUE^-1 truth_k T_TRUE times N(0, 0.002) rad /
N(0, 0.02) m of noise drawn in node order from default_rng(seed + 200); a HANDEYE of sigmas (0.2, 0.2, 0.2, 1.5, 1.5, 2) and threshold
1 on every node; the calibration node after the chain (adjacent to its last node) and before a GPS frame node.  Every case exists
twice: "_held", the calibration node fixed at T_TRUE, and "_free", started at T_START -- 0.10 rad / 0.077 m off -- under a PRIOR of
(0.5, 0.5, 1.5, 0.1, 0.1, 0.1) around T_START.  The restatement's results are computed once per process and left unchanged."""
import functools

import numpy as np

import pose_graph_calib_ref as calib
import pose_graph_cases as base
import pose_graph_gps_cases as gps_cases
import pose_graph_gps_ref as gps
import pose_graph_ref as ref

T_TRUE = ref.make_pose((0.02, -0.01, 0.3), (1.2, 0.3, -0.8))
_OFF = np.eye(4)
_OFF[:3, :3] = ref.exp_so3(0.10 * np.array([0.6, -0.5, 0.6245]) / np.linalg.norm([0.6, -0.5, 0.6245]))
_OFF[:3, 3] = (0.05, -0.04, 0.043)                                       # 0.077 m
T_START = T_TRUE @ _OFF
CHAIN_START_NOISE = 0.05


def rebased(drive):
    """the drive moved as a whole so that the truth's node 0 is the identity; the measurements are relative and stay"""
    back = ref.inv(drive["truth"][0])
    out = dict(drive)
    out["truth"] = np.stack([back @ X for X in drive["truth"]])
    out["poses"] = np.stack([back @ X for X in drive["poses"]])
    return out


def odom_of(truth, seed, rot_noise=0.002, trans_noise=0.02):
    rng = np.random.default_rng(seed + 200)
    out = []
    for X in truth:
        noise = np.eye(4)
        noise[:3, :3] = ref.exp_so3(rng.normal(size=3) * rot_noise)
        noise[:3, 3] = rng.normal(size=3) * trans_noise
        out.append(ref.inv(T_TRUE) @ X @ T_TRUE @ noise)
    return np.stack(out)


def calib_errors(T):
    """(rotation angle in rad, translation distance in m) of a calibration from T_TRUE"""
    D = ref.inv(T_TRUE) @ T
    return float(np.linalg.norm(ref.log_so3(D[:3, :3]))), float(np.linalg.norm(D[:3, 3]))


def _shaken(drive, seed, amount):
    """the free nodes' start moved by N(0, amount) rad / m, drawn in node order from default_rng(seed + 300)"""
    rng = np.random.default_rng(seed + 300)
    out = dict(drive)
    poses = drive["poses"].copy()
    for k in range(len(poses)):
        if not drive["fixed"][k]:
            poses[k] = ref.retract(poses[k], rng.normal(size=6) * amount)
    out["poses"] = poses
    return out


def _finish(drive, seed, free, start_noise=0.0):
    drive = rebased(drive)
    if start_noise:
        drive = _shaken(drive, seed, start_noise)
    odom = odom_of(drive["truth"], seed)
    g = calib.with_odom(drive, odom, T_START if free else T_TRUE, free)
    g.update(odom=odom, calib_node=len(drive["poses"]))
    return g


def chain_odom(n, seed, free):
    """n nodes of an open circle (no loop edge, node 0 fixed, started CHAIN_START_NOISE off the chained odometry) and the calibration
    node.  (Started from the chained odometry itself a short chain begins so close to its minimum that the cost rule stops it before
    the gradient has fallen by nine orders: chain2 did not qualify at any of 18 seeds.)"""
    if n == 1:                                        # (circle_drive needs an edge)
        truth = np.stack([ref.make_pose((0.01, -0.02, 0.3), (1.0, 2.0, 0.5))])
        return _finish(dict(truth=truth, poses=truth.copy(), fixed=np.ones(1, np.uint8), edges=np.zeros((0, 2), np.int32), Z=np.zeros((0, 4, 4))), seed, free)
    return _finish(ref.circle_drive(n, seed, loops=(), overlap=0), seed, free, CHAIN_START_NOISE)


def ring_odom(n, seed, free):
    """circle_drive's ring with its three loop edges"""
    return _finish(ref.circle_drive(n, seed), seed, free)


def gps_odom(n, seed, free):
    """a chain with both extra vertices: nodes 0..n-1, the calibration node n, the GPS frame node n + 1 (last); factors: the BETWEENs, the
    calibration node's PRIOR (free), the frame node's PRIOR, the HANDEYEs, a POINT for every node"""
    drive = _shaken(rebased(ref.circle_drive(n, seed, loops=(), overlap=0)), seed, CHAIN_START_NOISE)
    odom = odom_of(drive["truth"], seed)
    enu = gps_cases.enu_of(drive["truth"], seed)
    m = min(25, n)
    frame, _ = gps.alone_solve(drive["poses"][:m], enu[:m], gps_cases.LEVER)
    factors = [(calib.BETWEEN, int(i), int(j), gps.between_data(Z), ref.DEFAULT_SIGMAS, 0.0) for (i, j), Z in zip(drive["edges"], drive["Z"])]
    T0 = T_START if free else T_TRUE
    if free:
        factors.append((calib.PRIOR, n, n, gps.prior_data(T0), calib.CALIB_PRIOR_SIGMAS, 0.0))
    factors.append((calib.PRIOR, n + 1, n + 1, gps.prior_data(frame), gps.FRAME_SIGMAS, 0.0))
    factors += [(calib.HANDEYE, k, n, calib.handeye_data(odom[k]), calib.ODOM_SIGMAS, calib.ODOM_HUBER) for k in range(n)]
    factors += [(calib.POINT, n + 1, k, gps.point_data(gps_cases.LEVER, enu[k]), gps.GPS_SIGMAS, 0.0) for k in range(n)]
    g = calib.make_graph(list(drive["poses"]) + [T0, frame], list(drive["fixed"]) + [0 if free else 1, 0], factors)
    g.update(truth=drive["truth"], odom=odom, calib_node=n)
    return g


CHAIN_SIZES = (1, 2, 4, 23, 62, 63, 64)          # + the calibration node: 63 / 64 / 65 nodes straddle a level of the cyclic reduction
RING_SIZES = (16, 64)
GPS_SIZE = 24
# A case qualifies when the restatement's own direct and PCG solves take the same accepted / rejected counts, end within 1e-10 of each
# other, and its direct solve ends with a gradient below 1e-9 of the start's (or starts at a zero gradient: the one-node chains).  The
# seed of a case is the first of 200 + n, 300 + n, ... at which both its _held and its _free form qualify (the tests assert it).
# Passed over: chain2's 202, 302, ... 1102 (its _free form ends at 1.2e-9 .. 1.3e-8 of the start's gradient: the cost rule stops a graph of
# three factors there), ring16's 216 and 316 (1.2e-9, 1.1e-9), ring64's 264 (1.01e-9).  The 1e-9 on these graphs therefore holds by this
# choice, not by the stop rule, as in pose_graph_gps_cases.py.
SEEDS = {"chain1": 201, "chain2": 1202, "chain4": 204, "chain23": 223, "chain62": 262, "chain63": 263, "chain64": 264, "ring16": 416, "ring64": 364,
         "gps24": 224}
LARGE_SEED = 7


def names():
    return [stem + mode for stem in SEEDS for mode in ("_held", "_free")]


@functools.lru_cache(maxsize=None)
def graph(name):
    stem, mode = name.rsplit("_", 1)
    free = {"held": False, "free": True}[mode]
    seed = SEEDS[stem]
    if stem.startswith("chain"):
        return chain_odom(int(stem[5:]), seed, free)
    if stem.startswith("ring"):
        return ring_odom(int(stem[4:]), seed, free)
    if stem.startswith("gps"):
        return gps_odom(int(stem[3:]), seed, free)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, solver="direct"):
    """(graph, the restatement's poses, its stats) -- computed once"""
    g = graph(name)
    poses, st = calib.optimize(g, solver=solver)
    poses.setflags(write=False)
    return g, poses, st


def gradient_ratio(g, poses):
    """the restatement's gradient norm at `poses` over the one at the graph's start; 0 when the start's is zero"""
    start = calib.gradient_norm(g, g["poses"])
    return calib.gradient_norm(g, poses) / start if start > 1e-12 else 0.0       # (chain1: B = B_h (I - Ad(h^-1)) at h = I is rounding alone)


def qualifies(name):
    """(same accepted / rejected counts, largest pose difference, gradient ratio of the direct solve) of the restatement's own solves"""
    g, a, sa = reference(name, "direct")
    _, b, sb = reference(name, "pcg")
    return (sa["accepted"], sa["rejected"]) == (sb["accepted"], sb["rejected"]), max(base.pose_difference(a, b)), gradient_ratio(g, a)


@functools.lru_cache(maxsize=None)
def large_drive(free):
    """1 100 nodes, sixteen laps of a 44 m circle with no loop edge (pose_graph_gps_cases.large_drive's shape) and a HANDEYE on each:
    more factors than the workgroup has threads, and a calibration node of degree 1 100 (1 101 with its PRIOR).  Solved with scipy's
    sparse LU, and for the qualification with the sparse PCG."""
    g = _finish(ref.circle_drive(1100, LARGE_SEED, loops=(), overlap=1031), LARGE_SEED, free)
    poses, st = calib.optimize(g, solver="sparse")
    other, so = calib.optimize(g, solver="sparse_pcg")
    poses.setflags(write=False)
    st["own"] = ((st["accepted"], st["rejected"]) == (so["accepted"], so["rejected"]), max(base.pose_difference(poses, other)), max(so["pcg_each"]))
    return g, poses, st


def truth_error(g, poses):
    """the largest distance of a chain node from the truth, in m"""
    n = len(g["truth"])
    return float(np.linalg.norm(np.asarray(poses)[:n, :3, 3] - g["truth"][:, :3, 3], axis=1).max())


def check_stage_parity(g, got, v):
    """pose_graph_robust_cases.check_stage_parity's rules on the four kinds: residuals, A, B -- weighted where w < 1 -- within 1e-12
    relative; the gradient within 1e-12 of 6 x 4 products scaled by max(1, largest degree / 4), as pose_graph_gps_cases does for the
    frame node (the calibration node has a factor per chain node); M^-1 v within 100 eps cond(M) of a dense solve and with a backward
    residual at rounding level; the upper right 3 x 3 blocks of a HANDEYE's A and B exactly zero, as the rows 3..5 of a POINT and a
    PRIOR's B."""
    r, A, B, w = calib.linearize(g, g["poses"])
    for name, want, have in (("r", r, got["r"]), ("A", A, got["A"]), ("B", B, got["B"])):
        err = np.abs(have - want) / np.maximum(1.0, np.abs(want))
        print(name, "worst relative difference", err.max() if err.size else 0.0)
        assert (err <= 1e-12).all(), (name, err.max())
    print("weights below 1:", int((w < 1.0).sum()))
    pt, pr, he = g["kinds"] == calib.POINT, g["kinds"] == calib.PRIOR, g["kinds"] == calib.HANDEYE
    assert (got["r"][pt, 3:] == 0.0).all() and (got["A"][pt, 3:] == 0.0).all() and (got["B"][pt, 3:] == 0.0).all()
    assert (got["B"][pr] == 0.0).all()
    assert he.any() and (got["A"][he][:, :3, 3:] == 0.0).all() and (got["B"][he][:, :3, 3:] == 0.0).all()
    n = len(g["poses"])
    H, grad = calib.assemble(g, g["poses"])
    scale = max(np.abs(A).max() * np.abs(r).max() * 6 * 4, 1.0)
    deg = np.bincount(np.concatenate([g["ij"][:, 0], g["ij"][~pr, 1]]), minlength=n).max()
    print("g worst difference", np.abs(got["g"].ravel() - grad).max(), "scale", scale, "largest degree", deg)
    assert np.abs(got["g"].ravel() - grad).max() <= 1e-12 * scale * max(1.0, deg / 4.0)
    M = ref.chain_part(H)
    fx = np.repeat(np.asarray(g["fixed"]).astype(bool), 6)
    vv = np.where(fx, 0.0, v.ravel())
    want = np.linalg.solve(M, vv)
    cond = np.linalg.cond(M)
    have = got["minv_v"].ravel()
    print("M^-1 v worst difference", np.abs(have - want).max(), "bound", 100 * base.EPS * cond * np.abs(want).max(), "cond", cond)
    assert np.abs(have - want).max() <= 100 * base.EPS * cond * np.abs(want).max()
    back = np.abs(M @ have - vv)
    assert (back <= 1e-12 * (np.abs(M) @ np.abs(have) + np.abs(vv))).all(), back.max()
    assert (have[fx] == 0.0).all()
