"""The text the device's libnabo mode (nn_mode = NN_NABO: kd_build / nn_nabo of csrc/nabo_kernels.hip, kd_median_build of
csrc/kd_median_tree.h) is tested against: libnabo 1.0.7's buildNodes and recurseKnn as oracle/nabo.py restates them, with

  build   one definite partition -- a segment ordered by (coordinate on the cut dimension, caller index), the first
          count - count / 2 go left, cutVal = the coordinate of the next one -- where std::nth_element leaves the order of equal
          keys open.  On tie-free input it is oracle.nabo.NaboTree's tree; on tied input the rule kd_median_tree.h documents.
  legal   the rule check of ANY libnabo tree: whatever nth_element did with equal keys, these hold.
  walk    recurseKnn, recursive, in float64 over the arrays handed to it (the device's own, or build's), with nothing of the
          device's stack scheme: no pending-sibling words, no re-derivation, no pre-filter.  It says for every query whether the
          device's float32 walk is BOUND to agree (decidable) and how far the query may move before any decision changes (slack).
  check_lattice   the conditions under which float32 and float64 arithmetic coincide on a fixture, so that every query is decidable.

Arrays are in the layout the device keeps (csrc/nabo_tree.h) so that both sides can be compared node for node:
  nodes [n_nodes, 2] uint32   inner {cut value's float32 bits, (left child << 2) | cut dimension}, the right child behind the left;
                              leaf {first, (count << 2) | 3}; level order, a level's splitting nodes numbering their children in turn
  order [n] int               caller index of the point at every position; a leaf's points are positions [first, first + count)
"""
from __future__ import annotations

import math

import numpy as np

BUCKET = 8
U = 2.0 ** -24            # unit roundoff of float32


# ----------------------------------------------------------------------------------------------------------------------
# build
# ----------------------------------------------------------------------------------------------------------------------
def _arg_max(extent):
    """libnabo's argMax: starts from (index 0, value 0), strict '>'."""
    best, cd = np.float32(0.0), 0
    for d in range(3):
        if extent[d] > best:
            best, cd = extent[d], d
    return cd


def build(points_f32_centred):
    """(nodes, order) of the centred float32 cloud.  The box extents are float32 differences (libnabo computes in the cloud's
    scalar type; kd_median_tree.h says the same of its libnabo instantiation)."""
    pts = np.asarray(points_f32_centred, dtype=np.float32).reshape(-1, 3)
    n = len(pts)
    order = np.arange(n, dtype=np.int64)
    if n == 0:
        return np.zeros((0, 2), np.uint32), order
    nodes = [None]
    level = [(0, 0, n, pts.min(axis=0), pts.max(axis=0))]          # (node, first, count, inherited box min, max)
    while level:
        nxt = []
        for node, first, count, mn, mx in level:
            if count <= BUCKET:
                order[first:first + count] = np.sort(order[first:first + count])     # a bucket's entries in caller-index order
                nodes[node] = (first, (count << 2) | 3)
                continue
            cd = _arg_max(mx - mn)
            left = count - count // 2
            seg = order[first:first + count]
            seg = seg[np.lexsort((seg, pts[seg, cd]))]              # by (coordinate, caller index)
            order[first:first + count] = seg
            cut = pts[seg[left], cd]
            child = len(nodes)
            nodes[node] = (int(np.float32(cut).view(np.uint32)), (child << 2) | cd)
            nodes += [None, None]
            lmx = mx.copy(); lmx[cd] = cut
            rmn = mn.copy(); rmn[cd] = cut
            nxt.append((child, first, left, mn, lmx))
            nxt.append((child + 1, first + left, count - left, rmn, mx))
        level = nxt
    return np.array(nodes, dtype=np.uint32).reshape(-1, 2), order


def from_oracle(tree):
    """oracle.nabo.NaboTree (left child behind its parent, depth first) renumbered into the layout above; buckets as it left them."""
    if not tree.nodes:
        return np.zeros((0, 2), np.uint32), np.asarray(tree.perm, dtype=np.int64)
    nodes = [None]
    level = [(0, 0)]
    while level:
        nxt = []
        for mine, theirs in level:
            nd = tree.nodes[theirs]
            if nd[0] == 3:
                nodes[mine] = (nd[1], (nd[2] << 2) | 3)
                continue
            child = len(nodes)
            nodes[mine] = (int(np.float32(nd[1]).view(np.uint32)), (child << 2) | nd[0])
            nodes += [None, None]
            nxt += [(child, theirs + 1), (child + 1, nd[2])]
        level = nxt
    return np.array(nodes, dtype=np.uint32).reshape(-1, 2), np.asarray(tree.perm, dtype=np.int64)


# ----------------------------------------------------------------------------------------------------------------------
# legal
# ----------------------------------------------------------------------------------------------------------------------
def legal(nodes, order, points_f32_centred):
    """The violations (a list of strings; empty = a legal libnabo tree of the cloud) of the rules every buildNodes result obeys:
    cut dimension = argMax of the inherited box, left count = count - count / 2, every left value <= cutVal <= every right value,
    cutVal attained on the right, leaves of <= 8 entries (and inner nodes of more), every point exactly once."""
    pts = np.asarray(points_f32_centred, dtype=np.float32).reshape(-1, 3)
    nodes = np.asarray(nodes, dtype=np.uint32).reshape(-1, 2)
    order = np.asarray(order)
    n = len(pts)
    bad = []
    if len(order) != n or not np.array_equal(np.sort(order), np.arange(n)):
        return ["order is no permutation of the cloud"]
    if n == 0:
        return [] if len(nodes) == 0 else ["an empty cloud with nodes"]
    if len(nodes) == 0:
        return ["no nodes"]
    seen = np.zeros(len(nodes), dtype=bool)

    def rec(v, mn, mx):
        """-> (first, count) of the subtree, or None when it cannot be read"""
        if v >= len(nodes) or seen[v]:
            bad.append(f"node {v}: out of range or reached twice"); return None
        seen[v] = True
        x, y = int(nodes[v, 0]), int(nodes[v, 1])
        if (y & 3) == 3:
            first, count = x, y >> 2
            if count > BUCKET or (count < 1) or first + count > n:
                bad.append(f"leaf {v}: first {first} count {count}")
            return first, count
        cd, child = y & 3, y >> 2
        cut = np.uint32(x).view(np.float32)
        if cd != _arg_max(mx - mn):
            bad.append(f"node {v}: cut dimension {cd}, the inherited box asks for {_arg_max(mx - mn)}")
        lmx = mx.copy(); lmx[cd] = cut
        rmn = mn.copy(); rmn[cd] = cut
        a = rec(child, mn, lmx)
        b = rec(child + 1, rmn, mx)
        if a is None or b is None:
            return None
        if b[0] != a[0] + a[1]:
            bad.append(f"node {v}: the children's points are not side by side"); return None
        count = a[1] + b[1]
        if count <= BUCKET:
            bad.append(f"node {v}: {count} points split")
        if a[1] != count - count // 2:
            bad.append(f"node {v}: {a[1]} of {count} points on the left")
        lv = pts[order[a[0]:a[0] + a[1]], cd]
        rv = pts[order[b[0]:b[0] + b[1]], cd]
        if len(lv) and len(rv):
            if not (lv.max() <= cut <= rv.min()):
                bad.append(f"node {v}: cut value {cut} not between the sides ({lv.max()}, {rv.min()})")
            elif rv.min() != cut:
                bad.append(f"node {v}: cut value {cut} not attained on the right")
        return a[0], count

    root = rec(0, pts.min(axis=0), pts.max(axis=0))
    if root is not None and root != (0, n):
        bad.append(f"the root holds {root}, not (0, {n})")
    if not seen.all():
        bad.append("unreachable nodes")
    return bad


# ----------------------------------------------------------------------------------------------------------------------
# walk
# ----------------------------------------------------------------------------------------------------------------------
class Tree:
    """The arrays as Python lists of float64 / int (the walk is scalar code)."""

    def __init__(self, nodes, tq_xyz, ids):
        nodes = np.asarray(nodes, dtype=np.uint32).reshape(-1, 2)
        self.n_nodes = len(nodes)
        y = nodes[:, 1].astype(np.int64)
        self.dim = (y & 3).tolist()
        self.arg = (y >> 2).tolist()                                     # inner: left child; leaf: count
        self.first = nodes[:, 0].astype(np.int64).tolist()               # leaf: first position
        self.cut = nodes[:, 0].copy().view(np.float32).astype(np.float64).tolist()
        p = np.asarray(tq_xyz, dtype=np.float32).reshape(-1, 3).astype(np.float64)
        self.x, self.y, self.z = p[:, 0].tolist(), p[:, 1].tolist(), p[:, 2].tolist()
        self.ids = np.asarray(ids).astype(np.int64).tolist()


def tree_of_build(points_f32_centred):
    pts = np.asarray(points_f32_centred, dtype=np.float32).reshape(-1, 3)
    nodes, order = build(pts)
    return Tree(nodes, pts[order], order)


def max_error2(eps):
    """(1 + eps)^2 as the device forms it: in float32."""
    e = np.float32(1.0) + np.float32(eps)
    return float(np.float32(e * e))


class Walk:
    __slots__ = ("id", "pos", "d2", "leaves", "decidable", "slack", "slack_by", "second", "second_pos")


def walk(tree, q_f32, eps, u=U):
    """recurseKnn(k = 1, epsilon = eps, ALLOW_SELF_MATCH) of one float32 query.  Returns a Walk:

    id, pos     caller index and position of the winner (-1 for a non-finite query or an empty tree), d2 its squared distance
    leaves      the leaf nodes visited, in order
    decidable   whether every comparison of the walk keeps its outcome under the roundings of the device's float32 expressions.
                Beside every value x goes A, the sum of its absolute addends, and r, the number of float roundings on the longest
                chain into it, so that |x_float - x| <= (r + 1) u A to first order:
                  a point distance   fma(dz, dz, fma(dy, dy, dx * dx)) with d. = q. - p.: a subtraction (twice into its square), a
                                     product, two fused adds: r = 5, A = the distance itself
                  rd                 kd_rd_step per far step k: new_off (twice into its square), the squares, the inner and the
                                     outer add (r = 5), one more outer add per later step; the product with (1 + eps)^2: one more.
                                     A = the sum of old_off^2 + new_off^2 over the steps
                A comparison x < y is undecidable when |x - y| <= (r_x + 1) u A_x + (r_y + 1) u A_y.  Side decisions new_off > 0
                compare two floats -- a float subtraction has the exact sign -- and are always decidable.  With u = 0 (a fixture
                check_lattice accepted: float32 and float64 coincide) every comparison is decidable, an exact tie included.
    slack       how far (in the query's units) the query may move before a decision of THIS walk can change, in float64: the
                smallest of |new_off| over the inner nodes entered, |sqrt(rd E2) - sqrt(best)| / (2 + eps) over the prune decisions
                and half the winner / runner-up gap in sqrt.  slack_by = (kind, node, dimension) of the decision that set it.
    """
    t = tree
    w = Walk()
    q = [float(q_f32[0]), float(q_f32[1]), float(q_f32[2])]
    w.id, w.pos, w.d2, w.leaves, w.decidable, w.slack, w.slack_by, w.second = -1, -1, math.inf, [], True, 0.0, None, math.inf
    w.second_pos = -1
    if t.n_nodes == 0 or not (math.isfinite(q[0]) and math.isfinite(q[1]) and math.isfinite(q[2])):
        return w
    E2 = max_error2(eps)
    inv = 1.0 / (1.0 + math.sqrt(E2))
    off = [0.0, 0.0, 0.0]
    st = [math.inf, -1, math.inf, True, math.inf, None, -1]   # best, its position, second, decidable, slack, slack_by, second's position
    tx, ty, tz, dim, arg, first, cut, leaves = t.x, t.y, t.z, t.dim, t.arg, t.first, t.cut, w.leaves

    def rec(n, rd, a_rd, steps):
        if dim[n] == 3:
            leaves.append(n)
            for e in range(first[n], first[n] + arg[n]):
                dx, dy, dz = q[0] - tx[e], q[1] - ty[e], q[2] - tz[e]
                d = dz * dz + (dy * dy + dx * dx)
                best = st[0]
                if u > 0.0 and best < math.inf and abs(d - best) <= 6.0 * u * (d + best):
                    st[3] = False
                if d < best:
                    st[2], st[6] = best, st[1]
                    st[0], st[1] = d, e
                elif d < st[2]:
                    st[2], st[6] = d, e
            return
        cd = dim[n]
        old_off, new_off = off[cd], q[cd] - cut[n]
        if abs(new_off) < st[4]:
            st[4], st[5] = abs(new_off), ("side", n, cd)
        near, far = (arg[n] + 1, arg[n]) if new_off > 0 else (arg[n], arg[n] + 1)
        rec(near, rd, a_rd, steps)
        rd = rd + (-old_off * old_off + new_off * new_off)
        a_rd = a_rd + (old_off * old_off + new_off * new_off)
        steps = steps + 1
        x, best = rd * E2, st[0]
        if u > 0.0 and abs(x - best) <= (6.0 + steps) * u * a_rd * E2 + 6.0 * u * best:
            st[3] = False
        gap = abs(math.sqrt(max(x, 0.0)) - math.sqrt(best)) * inv
        if gap < st[4]:
            st[4], st[5] = gap, ("prune", n, cd)
        if x < best:
            off[cd] = new_off
            rec(far, rd, a_rd, steps)
            off[cd] = old_off

    rec(0, 0.0, 0.0, 0)
    w.pos, w.d2, w.second, w.decidable, w.second_pos = st[1], st[0], st[2], st[3], st[6]
    w.id = t.ids[st[1]]
    w.slack, w.slack_by = st[4], st[5]
    if st[2] < math.inf:
        win = 0.5 * (math.sqrt(st[2]) - math.sqrt(st[0]))
        if win < w.slack:
            w.slack, w.slack_by = win, ("win", -1, -1)
        if u > 0.0 and st[2] - st[0] <= 6.0 * u * (st[2] + st[0]):
            w.decidable = False                                  # the winner itself hangs on a rounding
    return w


def displaced(tree, q_f32, w, lb, rng):
    """The float32 queries at 0.9 lb, less two ulp of the query's largest coordinate, from q along: + and - the axis of the
    decision that set the walk's slack (for the winner's gap: the line from the winner to the runner-up), towards the winner,
    towards the runner-up, and one random direction.  Empty when that distance is not positive."""
    q = np.asarray(q_f32, dtype=np.float32).astype(np.float64)
    step = 0.9 * float(lb) - 2.0 * float(np.spacing(np.float32(np.abs(q).max())))
    if not (step > 0.0) or w.pos < 0:
        return []
    at = lambda e: np.array([tree.x[e], tree.y[e], tree.z[e]])
    dirs = []
    if w.slack_by is not None and w.slack_by[0] != "win":
        axis = np.zeros(3); axis[w.slack_by[2]] = 1.0
    elif w.second_pos >= 0 and np.any(at(w.second_pos) != at(w.pos)):
        axis = at(w.second_pos) - at(w.pos)
    else:
        axis = np.array([1.0, 0.0, 0.0])
    dirs += [axis, -axis, at(w.pos) - q]
    if w.second_pos >= 0:
        dirs.append(at(w.second_pos) - q)
    dirs.append(rng.normal(size=3))
    out = []
    for d in dirs:
        nrm = float(np.linalg.norm(d))
        if nrm > 0.0:
            out.append((q + d * (step / nrm)).astype(np.float32))
    return out


def walk_all(tree, queries_f32, eps, u=U):
    return [walk(tree, q, eps, u) for q in np.asarray(queries_f32, dtype=np.float32).reshape(-1, 3)]


# ----------------------------------------------------------------------------------------------------------------------
# queries and lattices
# ----------------------------------------------------------------------------------------------------------------------
def queries(src_f32, pose, mu):
    """The float32 queries the device forms from a source cloud: M = T(-mu) * pose in float64, q = float32(M s).  Also `firm`:
    rows whose float32 rounding does not hang on the last bits of the float64 sum (the device fuses its multiply-adds and carries
    its own copy of the pose: under a rotation a float64 value within 2^-44 of the sum of its terms' magnitudes -- five hundred float64 roundings --
    of a float32 rounding boundary may round either way)."""
    s = np.asarray(src_f32, dtype=np.float32)[:, :3].astype(np.float64)
    M = np.asarray(pose, dtype=np.float64)
    t = M[:3, 3] - np.asarray(mu, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if np.array_equal(M[:3, :3], np.eye(3)):         # no rotation: one float64 addition here as there, the same bits
            q64, margin = s + t, 0.0
        else:
            q64 = s @ M[:3, :3].T + t
            margin = 2.0 ** -44 * (np.abs(s) @ np.abs(M[:3, :3]).T + np.abs(t))
        q = q64.astype(np.float32)
        lo, hi = (q64 - margin).astype(np.float32), (q64 + margin).astype(np.float32)
    firm = ((lo == q) & (hi == q)).all(axis=1) | ~np.isfinite(q).all(axis=1)
    return q, firm


def check_lattice(target, queries_raw, mu, quantum, eps):
    """Asserts that float32 and float64 arithmetic coincide on the fixture (so every query is decidable and distance ties are
    decided by bucket order, which the reference reads from the same arrays): every centred coordinate and every centred query
    coordinate is a multiple of the quantum, every squared distance and every rd stays below 2^24 quanta^2, mu is the cloud's
    mean and a lattice point (the sums below are integers, exact in any order), and (1 + eps)^2 is a power of two.
    Rows of queries_raw with a non-finite coordinate are skipped (the search answers them with -1)."""
    tgt = np.asarray(target, dtype=np.float32)[:, :3].astype(np.float64)
    qry = np.asarray(queries_raw, dtype=np.float32)[:, :3].astype(np.float64)
    qry = qry[np.isfinite(qry).all(axis=1)]
    mu = np.asarray(mu, dtype=np.float64)
    for name, a in (("target", tgt), ("queries", qry), ("mu", mu[None, :])):
        k = a / quantum
        assert np.array_equal(k, np.round(k)) and np.abs(k).max(initial=0.0) < 2.0 ** 24, f"{name}: not on the lattice"
    total = np.round(tgt / quantum).astype(np.int64).sum(axis=0)
    assert (total % len(tgt) == 0).all() and np.array_equal(total // len(tgt), np.round(mu / quantum).astype(np.int64)), "mu is not the mean"
    c, p = (tgt - mu) / quantum, (qry - mu) / quantum
    # a distance, and rd (a sum of squared offsets from cut planes inside the box, one per dimension), is at most the squared
    # distance from the query to the farthest corner of the cloud's box
    both = np.concatenate([p, c])
    far = (np.maximum(np.abs(both - c.min(axis=0)), np.abs(both - c.max(axis=0))) ** 2).sum(axis=1).max()
    E2 = max_error2(eps)
    assert far < 2.0 ** 24, f"squared distances reach {far} quanta^2"
    assert math.frexp(E2)[0] == 0.5, f"(1 + eps)^2 = {E2} is no power of two"
    return True
