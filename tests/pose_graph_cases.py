"""Graphs and comparisons shared by the pose-graph tests: the same cases run through the kernel's loop compiled for the CPU
(test_pose_graph_cpp.py) and through the device (test_pose_graph_gpu.py), both against tests/pose_graph_ref.py.  Every graph is
generated from a seed; the restatement's results are computed once per process and left unchanged."""
import functools

import numpy as np

import pose_graph_ref as ref

EPS = np.finfo(np.float64).eps


def chain_graph(n, seed, loops=(), missing=(), fixed=(0,), step=4.0, rot_noise=0.002, trans_noise=0.02, start_noise=0.0):
    """n nodes on a random walk (steps of about `step` m, turning up to 0.4 rad), odometry edges (k, k + 1) except those whose k is in
    `missing`, loop edges `loops`; every measurement is the truth with N(0, rot_noise) rad / N(0, trans_noise) m noise.  Initial
    poses: the truth moved by N(0, start_noise) rad / m at every free node (0: the truth itself)."""
    rng = np.random.default_rng(seed)
    truth = [ref.make_pose((0.01, -0.02, 0.3), (1.0, 2.0, 0.5))]
    for _ in range(n - 1):
        truth.append(truth[-1] @ ref.make_pose(rng.normal(size=3) * (0.02, 0.02, 0.2), (step + rng.normal() * 0.3, rng.normal() * 0.3, rng.normal() * 0.05)))
    truth = np.stack(truth)

    def noise(r, t):
        X = np.eye(4)
        X[:3, :3] = ref.exp_so3(rng.normal(size=3) * r)
        X[:3, 3] = rng.normal(size=3) * t
        return X
    edges = [(k, k + 1) for k in range(n - 1) if k not in missing] + list(loops)
    Z = [ref.inv(truth[i]) @ truth[j] @ noise(rot_noise, trans_noise) for i, j in edges]
    fx = np.zeros(n, np.uint8)
    fx[list(fixed)] = 1
    poses = np.stack([truth[k] if fx[k] or start_noise == 0.0 else truth[k] @ noise(start_noise, start_noise) for k in range(n)])
    return dict(truth=truth, poses=poses, fixed=fx, edges=np.array(edges, np.int32).reshape(-1, 2), Z=np.stack(Z))


# Stage parity: the sizes at which the cyclic reduction changes shape -- 2 (one level, no coupling left), 3 and 5 (a last node
# without a right neighbour at some level), 63 / 64 / 65 (around a power of two: 6, 6 and 7 levels), a missing chain edge (M falls
# into two blocks; the loop edges keep the graph connected), a fixed node in the middle (an identity block inside M), and a graph
# whose edges include reversed chain edges (j = i - 1) and two edges between the same pair.
def stage_cases():
    return {
        "n2": chain_graph(2, 2, start_noise=0.05),
        "n3": chain_graph(3, 3, loops=[(0, 2)], start_noise=0.05),
        "n5": chain_graph(5, 5, loops=[(0, 4), (1, 3)], start_noise=0.05),
        "n63": chain_graph(63, 63, loops=[(0, 62), (5, 40)], start_noise=0.03),
        "n64": chain_graph(64, 64, loops=[(0, 63), (1, 62), (20, 50)], start_noise=0.03),
        "n65": chain_graph(65, 65, loops=[(0, 64), (64, 3)], start_noise=0.03),
        "missing_chain_edge": chain_graph(40, 7, loops=[(0, 39), (10, 30), (18, 22)], missing=(19,), start_noise=0.03),
        "fixed_in_the_middle": chain_graph(21, 8, loops=[(2, 19)], fixed=(0, 9), start_noise=0.05),
        "reversed_and_double": _reversed_and_double(),
    }


def _reversed_and_double():
    g = chain_graph(12, 9, loops=[(0, 11)], start_noise=0.04)
    e, Z = g["edges"].copy(), g["Z"].copy()
    for k in (3, 7):                                   # edge k is (k, k + 1): turn it round
        e[k] = e[k][::-1]
        Z[k] = ref.inv(Z[k])
    e = np.concatenate([e, e[[5]]])                    # a second factor on (5, 6)
    Z = np.concatenate([Z, Z[[5]] @ ref.make_pose((0.001, 0, 0.002), (0.01, -0.02, 0))[None]])
    g.update(edges=e, Z=Z)
    return g


def angle_cases():
    """near_pi: the loop edge's residual rotation starts 1e-3 below pi; near_pi_6: 1e-6 below, where w = vee(R - R^T) / 2 is a
    thousand times smaller and the axis comes from the symmetric part alone; near_zero: every residual rotation is about 1e-9 rad;
    two_nodes: one edge, the minimum has cost 0; triangle: a loop that contradicts the two chain edges."""
    near_pi = chain_graph(6, 11, loops=[(0, 5)], rot_noise=0.0, trans_noise=0.0)
    a = np.array([0.3, -0.5, 0.81])
    a /= np.linalg.norm(a)
    turn = np.eye(4)
    turn[:3, :3] = ref.exp_so3((np.pi - 1e-3) * a)
    near_pi["Z"][-1] = near_pi["Z"][-1] @ turn
    near_pi_6 = chain_graph(6, 11, loops=[(0, 5)], rot_noise=0.0, trans_noise=0.0)
    turn6 = np.eye(4)
    turn6[:3, :3] = ref.exp_so3((np.pi - 1e-6) * a)
    near_pi_6["Z"][-1] = near_pi_6["Z"][-1] @ turn6
    near_zero = chain_graph(6, 12, loops=[(0, 5)], rot_noise=1e-9, trans_noise=1e-9)
    two = chain_graph(2, 13, start_noise=0.2)
    tri = chain_graph(3, 14, loops=[(0, 2)], rot_noise=0.0, trans_noise=0.0)
    tri["Z"][-1] = tri["Z"][-1] @ ref.make_pose((0.0, 0.0, 0.2), (0.8, -0.5, 0.1))
    return {"near_pi": near_pi, "near_pi_6": near_pi_6, "near_zero": near_zero, "two_nodes": two, "triangle": tri}


def circle_cases():
    return {"circle64": ref.circle_drive(64, 1), "circle240": ref.circle_drive(240, 1)}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(graph, restatement's poses by its direct solve, its stats) -- computed once"""
    g = {**stage_cases(), **angle_cases(), **circle_cases()}[name]
    poses, st = ref.optimize(g["poses"], g["fixed"], g["edges"], g["Z"])
    poses.setflags(write=False)
    return g, poses, st


@functools.lru_cache(maxsize=None)
def large_circle():
    """1 500 nodes: more nodes than the workgroup has threads, so every strided loop of the kernel takes a second round and the
    cyclic reduction has 11 levels.  The restatement solves it with scipy's sparse LU (the dense H would be 9 000 x 9 000)."""
    g = ref.circle_drive(1500, seed=3, loops=[(k, None) for k in range(6)], overlap=8)
    poses, st = ref.optimize(g["poses"], g["fixed"], g["edges"], g["Z"], solver="sparse")
    poses.setflags(write=False)
    return g, poses, st


def probe_vector(n, seed=99):
    return np.random.default_rng(seed).normal(size=(n, 6))


def check_stage_parity(g, got, v):
    """got: dict(r, A, B, g, minv_v) of the first linearisation at g["poses"].  Tolerances: the residual and Jacobian entries are a
    few dozen f64 operations on numbers up to |x| = max(1, the entry), so 1e-12 |x| is ~50 roundings of margin each.  The gradient
    sums up to 6 x (edges of a node) products A^T r: 1e-12 of the largest |A| |r| sum.  M^-1 v: cyclic reduction and LAPACK's
    solve are both backward stable for a positive definite M, so each is within ~ n eps cond(M) |x| of the solution; the bound is 100 eps
    cond(M) max|x|, and independently the residual M x - v must be at rounding level, 1e-12 (|M| |x| + |v|)."""
    r, A, B = ref.linearize(g["poses"], g["edges"], g["Z"])
    for name, want, have in (("r", r, got["r"]), ("A", A, got["A"]), ("B", B, got["B"])):
        err = np.abs(have - want) / np.maximum(1.0, np.abs(want))
        print(name, "worst relative difference", err.max() if err.size else 0.0)
        assert (err <= 1e-12).all(), (name, err.max())
    n = len(g["poses"])
    H, grad = ref.assemble(n, g["fixed"], g["edges"], r, A, B)
    scale = max(np.abs(A).max() * np.abs(r).max() * 6 * 4, 1.0)
    print("g worst difference", np.abs(got["g"].ravel() - grad).max(), "scale", scale)
    assert np.abs(got["g"].ravel() - grad).max() <= 1e-12 * scale
    M = ref.chain_part(H)
    vv = np.where(np.repeat(g["fixed"].astype(bool), 6), 0.0, v.ravel())
    want = np.linalg.solve(M, vv)
    cond = np.linalg.cond(M)
    have = got["minv_v"].ravel()
    print("M^-1 v worst difference", np.abs(have - want).max(), "bound", 100 * EPS * cond * np.abs(want).max(), "cond", cond)
    assert np.abs(have - want).max() <= 100 * EPS * cond * np.abs(want).max()
    back = np.abs(M @ have - vv)
    assert (back <= 1e-12 * (np.abs(M) @ np.abs(have) + np.abs(vv))).all(), back.max()
    assert (have[np.repeat(g["fixed"].astype(bool), 6)] == 0.0).all()


def pose_difference(a, b):
    """(largest translation difference in m, largest rotation-entry difference)"""
    return float(np.abs(a[:, :3, 3] - b[:, :3, 3]).max()), float(np.abs(a[:, :3, :3] - b[:, :3, :3]).max())


def gradient_ratio(g, poses):
    """the restatement's gradient norm at `poses` over the one at the graph's start"""
    return ref.gradient_norm(poses, g["fixed"], g["edges"], g["Z"]) / ref.gradient_norm(g["poses"], g["fixed"], g["edges"], g["Z"])


def check_costs(stats, st):
    """The costs against the restatement's.  A whitened residual carries an absolute rounding error of ~ eps x 20 m / 0.1 ~ 1e-13 whatever
    its size, so a sum of squares c moves by up to 2 sqrt(c) sqrt(6 E) 1e-13 < 1e-11 sqrt(c) on top of 1e-12 c for the sum itself; the
    final cost also moves with the poses (1e-9 relative is far above what a 1e-9 m difference does at a minimum)."""
    for key, rel in (("initial_cost", 1e-12), ("final_cost", 1e-9)):
        c = st[key]
        assert abs(stats[key] - c) <= rel * c + 1e-11 * np.sqrt(c) + 1e-24, (key, stats[key], c)
