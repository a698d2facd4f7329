"""Graphs with GPS (ENU) factors shared by the CPU, C++ and device tests, all against tests/pose_graph_gps_ref.py.  Fixed ingredients:
the truth frame G, the lever arm, enu_k = G (truth_k l) + N(0, 0.05) drawn in node order from default_rng(seed + 100), the frame
node last with its prior at the alone-solve result of the first min(25, n) poses started from identity.  The restatement's results are
computed once per process and left unchanged."""
import functools

import numpy as np

import pose_graph_cases as base
import pose_graph_gps_ref as gps
import pose_graph_ref as ref

G = ref.make_pose((0.01, -0.02, 0.4), (350.0, -120.0, 12.0))
LEVER = np.array([0.3, -0.2, 1.1])
EPS = np.finfo(np.float64).eps


def enu_of(truth, seed, frame=G, lever=LEVER):
    rng = np.random.default_rng(seed + 100)
    return np.stack([frame[:3, :3] @ (T[:3, :3] @ lever + T[:3, 3]) + frame[:3, 3] + rng.normal(0.0, 0.05, 3) for T in truth])


def enu_positions(poses, frame, lever=LEVER):
    """where `frame` puts the antenna of every pose"""
    return np.stack([frame[:3, :3] @ (P[:3, :3] @ lever + P[:3, 3]) + frame[:3, 3] for P in poses])


def _finish(drive, seed, which):
    n = len(drive["poses"])
    enu = enu_of(drive["truth"], seed)
    m = min(25, n)
    frame, st = gps.alone_solve(drive["poses"][:m], enu[:m], LEVER)
    g = gps.with_gps(drive, enu, LEVER, frame, which)
    g.update(enu=enu, alone=st)
    return g


def circle_gps(n, seed, loops=((0, None), (1, None), (2, None)), every=1, **kw):
    return _finish(ref.circle_drive(n, seed, loops, **kw), seed, range(0, n, every))


def chain_gps(n, seed, mode):
    """a chain of pose_graph_cases (node 0 fixed, the free nodes started 0.1 off the truth) plus the frame node; mode: "all", "second"
    (every second node, counted from the last) or "last".  The frame node is adjacent to the last chain node."""
    if n == 1:
        truth = np.stack([ref.make_pose((0.01, -0.02, 0.3), (1.0, 2.0, 0.5))])
        drive = dict(truth=truth, poses=truth.copy(), fixed=np.ones(1, np.uint8), edges=np.zeros((0, 2), np.int32), Z=np.zeros((0, 4, 4)))
    else:
        drive = base.chain_graph(n, seed, start_noise=0.1)
    which = {"all": range(n), "second": range(n - 1, -1, -2), "last": [n - 1]}[mode]
    return _finish(drive, seed, sorted(which))


CHAIN_SIZES = (1, 2, 4, 23, 62, 63, 64)
# The residuals at the minimum are not zero (0.05 m of ENU noise against sigma 0.15), so Gauss-Newton converges linearly and the cost
# rule may stop it a step short of a gradient 1e-9 of the start's.  The seed of a size is the first of 200 + n, 300 + n, ... at which
# the restatement's own direct solve ends below that in all three modes (the tests assert it), so that the device can be held to it.
# (Passed over: three seeds at n = 2 and two at n = 23.  The 1e-9 on these graphs therefore holds by this choice, not by the stop rule.)
CHAIN_SEEDS = {1: 201, 2: 502, 4: 204, 23: 423, 62: 262, 63: 263, 64: 264}


def chain_cases():
    return {"chain%d_%s" % (n, mode): (n, CHAIN_SEEDS[n], mode) for n in CHAIN_SIZES for mode in ("all", "second", "last")}


def alone_case(seed=5):
    """the 25 + 1 alone graph of the seed-5 drive, started from identity: no chain edge at all"""
    d = ref.circle_drive(240, seed)
    enu = enu_of(d["truth"], seed)
    g = gps.alone_graph(d["poses"][:25], enu[:25], LEVER)
    g.update(truth=d["truth"][:25], enu=enu[:25])
    return g


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "alone":
        return alone_case()
    if name == "drive240":
        return circle_gps(240, 5, every=2)         # the qualifying drive
    if name == "drive240_seed3":
        return circle_gps(240, 3, every=2)         # the documented example that does not qualify
    if name == "drive64_all":                      # no revisit: GPS alone bounds the drift
        return circle_gps(64, 5, loops=())
    if name == "drive240_all":
        return circle_gps(240, 5, loops=())
    if name == "drive240_all_loops":
        return circle_gps(240, 5)
    return chain_gps(*chain_cases()[name])


@functools.lru_cache(maxsize=None)
def reference(name, solver="direct"):
    """(graph, the restatement's poses, its stats) -- computed once"""
    g = graph(name)
    poses, st = gps.optimize(g, solver=solver, max_iterations=100 if name == "alone" else 50)
    poses.setflags(write=False)
    return g, poses, st


@functools.lru_cache(maxsize=None)
def large_drive():
    """1 100 nodes, sixteen laps of a 44 m circle with no loop edge, a factor on each: 2 200 factors, more than the workgroup has
    threads, and a frame node of degree 1 101.  Solved with scipy's sparse LU, and for the qualification with the sparse PCG.
    (One lap of 1 100 nodes does not do: a single antenna does not see a roll about the driving direction that a sideways shift of
    l_z x roll makes up for, only the chain's curvature holds that mode, 0.006 rad a node on one lap, and with 0.05 m of ENU noise
    Gauss-Newton then converges linearly at 0.5 a step and worse -- the restatement itself runs into max_iterations there,
    DESIGN.md section 6 "GPS".  Four laps of 275 converge in 17 steps, but the restatement's own two solves end 3.4e-9 m apart along
    that mode, which does not qualify; at 0.091 rad a node they take 8 steps and end 5.1e-11 m apart.)"""
    g = circle_gps(1100, 7, loops=(), every=1, overlap=1031)
    poses, st = gps.optimize(g, solver="sparse")
    other, so = gps.optimize(g, solver="sparse_pcg")
    poses.setflags(write=False)
    st["own"] = ((st["accepted"], st["rejected"]) == (so["accepted"], so["rejected"]), max(base.pose_difference(poses, other)), max(so["pcg_each"]))
    return g, poses, st


def qualifies(name):
    """(same accepted / rejected counts, largest pose difference) of the restatement's own direct and PCG solves"""
    _, a, sa = reference(name, "direct")
    _, b, sb = reference(name, "pcg")
    return (sa["accepted"], sa["rejected"]) == (sb["accepted"], sb["rejected"]), max(base.pose_difference(a, b))


def check_stage_parity(g, got, v):
    """pose_graph_cases.check_stage_parity for factors of any kind: residuals, A, B within 1e-12 relative, M^-1 v within 100 eps cond(M)
    of a dense solve and with a backward residual at rounding level, all as there; plus rows 3..5 of a POINT and a PRIOR's B exactly
    zero.  One tolerance differs and is wider: the gradient.  The base rule, 1e-12 of 6 x 4 products |A| |r|, assumes a node of about
    four factors; the frame node sums 6 x degree of them (degree up to 65 here), so the bound is scaled by max(1, degree / 4) of the
    graph's largest degree -- still ~1e4 roundings of margin per product."""
    r, A, B = gps.linearize(g, g["poses"])
    for name, want, have in (("r", r, got["r"]), ("A", A, got["A"]), ("B", B, got["B"])):
        err = np.abs(have - want) / np.maximum(1.0, np.abs(want))
        print(name, "worst relative difference", err.max() if err.size else 0.0)
        assert (err <= 1e-12).all(), (name, err.max())
    pt, pr = g["kinds"] == gps.POINT, g["kinds"] == gps.PRIOR
    assert (got["r"][pt, 3:] == 0.0).all() and (got["A"][pt, 3:] == 0.0).all() and (got["B"][pt, 3:] == 0.0).all()
    assert (got["B"][pr] == 0.0).all()
    n = len(g["poses"])
    H, grad = gps.assemble(g, g["poses"])
    scale = max(np.abs(A).max() * np.abs(r).max() * 6 * 4, 1.0)
    deg = np.bincount(np.concatenate([g["ij"][:, 0], g["ij"][~pr, 1]]), minlength=n).max()
    print("g worst difference", np.abs(got["g"].ravel() - grad).max(), "scale", scale, "largest degree", deg)
    assert np.abs(got["g"].ravel() - grad).max() <= 1e-12 * scale * max(1.0, deg / 4.0)      # (6 x degree products; the base rule assumes 4)
    M = ref.chain_part(H)
    fx = np.repeat(np.asarray(g["fixed"]).astype(bool), 6)
    vv = np.where(fx, 0.0, v.ravel())
    want = np.linalg.solve(M, vv)
    cond = np.linalg.cond(M)
    have = got["minv_v"].ravel()
    print("M^-1 v worst difference", np.abs(have - want).max(), "bound", 100 * EPS * cond * np.abs(want).max(), "cond", cond)
    assert np.abs(have - want).max() <= 100 * EPS * cond * np.abs(want).max()
    back = np.abs(M @ have - vv)
    assert (back <= 1e-12 * (np.abs(M) @ np.abs(have) + np.abs(vv))).all(), back.max()
    assert (have[fx] == 0.0).all()


def gradient_ratio(g, poses):
    return gps.gradient_norm(g, poses) / gps.gradient_norm(g, g["poses"])


def enu_error(g, poses):
    """the largest distance of the antenna positions, mapped by the frame node, from the truth's ENU positions (without noise)"""
    n = len(poses) - 1
    return float(np.linalg.norm(enu_positions(poses[:n], poses[n]) - enu_positions(g["truth"], G), axis=1).max())
