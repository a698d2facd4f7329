#!/usr/bin/env python3
"""Iteration 0 of nn_ball_lds counted on the host (numpy only: no GPU, no library build) for chosen pairs of bench.py's drive.

For pair k the tool restates what the device does before and in iteration 0:
  * the source's order: morton_keys (prep_normals.hip) -- 6.25 cm quantum from the finite minimum, 21 bits an axis, stable sort;
  * the target grid of grid_setup_pair (icp_kernels.hip) from oracle.icp_fast.calculate_normals of the previous scan: the mean in
    double, the centred points in float32, origin = least centred coordinate - h / 2, floor(extent / h) + 2 cells an axis, the
    cell grown by 2^(1/3) until the 32-cell words fit kMaxGridWords;
  * every query's block of cells from the extrapolated guess (search_round: Rs = R * 1.0001 + 1e-3 h, clipped to the grid).
and prints
  * the path split of the rounds of 256 queries (points staged / row tables only / global lookups) under the caps of smhip_device.h;
  * how many waves (64 queries) and half workgroups (128) of the rounds that are not staged would fit their own box under a quarter
    / a half / all of the caps;
  * the share of the table-only rounds a larger point cap would stage, and the share of the rounds a larger table cap leaves global;
  * per query of the global rounds: rows of the ball visited, rows with a cell in range, candidates, queries without any;
  * dependent global-load levels a wave and global round under three walks of the rows: one row at a time (a level for the words
    if any lane visits the slot's row, one for the run bounds if any lane's row holds a cell in range, one per four points of the
    longest run); every row's lookups in flight together (words, bounds, then the lanes' sweeps side by side); and four rows at a
    time with the four runs swept as one sequence (sweep_rows_global).

    python tools/ball_box_count.py [--pairs 0,30,100,300] [--points 120000]
A pair takes a few seconds (two ray-cast scans, the normals of one)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TABLE_CAP, ROW_CAP, POINT_CAP = 1024, 256, 512             # kLdsTableCap, kLdsRowCap, kLdsPointCap
MAX_GRID_WORDS = 1 << 18                                   # kMaxGridWords
RADIUS, CELL = 0.3, 0.25                                   # ball_radius, grid_cell: the library's defaults
F = np.float32


def bench_pair(k, n_points, n_distinct=512, seed=5):
    """Pair k of bench.py's build_workload: (source rows float32 [n, 4], target scan, extrapolated guess)."""
    from staticmapping_amd import synth
    poses = synth.drive_poses(n_distinct + 2, seed=seed, speed=8.0, speed_spread=2.0, yaw_rate_max=0.2, segment_s=1.0)
    scene = synth.make_drive_scene(poses, seed=seed)
    scan = lambda j: synth.velodyne_scan(synth.scene_near(scene, poses[j + 1][:3, 3]), poses[j + 1], seed=500 + j, n_points=n_points)
    return scan(k + 1), scan(k), np.linalg.inv(poses[k]) @ poses[k + 1]


def spread21(v):
    v = v.astype(np.uint64) & np.uint64(0x1fffff)
    for sh, m in ((32, 0x1f00000000ffff), (16, 0x1f0000ff0000ff), (8, 0x100f00f00f00f00f), (4, 0x10c30c30c30c30c3), (2, 0x1249249249249249)):
        v = (v | (v << np.uint64(sh))) & np.uint64(m)
    return v


def morton_order(src):
    p = src[:, :3].astype(F)
    mn = np.where(np.isfinite(p), p, np.inf).min(axis=0).astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (p - mn) * F(16.0)
        q = np.where(np.isfinite(t), np.clip(t, 0, 2097151.0), 0).astype(np.uint64)
    key = spread21(q[:, 0]) | (spread21(q[:, 1]) << np.uint64(1)) | (spread21(q[:, 2]) << np.uint64(2))
    return p[np.argsort(key, kind="stable")]


def target_grid(q):
    q32 = q.astype(F).astype(np.float64)
    mu = q32.mean(axis=0)
    c = (q32 - mu).astype(F)
    cmin, cmax = c.min(axis=0), c.max(axis=0)
    h = F(CELL)
    while True:
        dims = (np.floor((cmax - cmin) * (F(1.0) / h)) + 2).astype(np.int64)
        if ((dims[0] + 31) >> 5) * dims[1] * dims[2] <= MAX_GRID_WORDS:
            break
        h = F(h * F(1.25992105))
    origin = (cmin - F(0.5) * h).astype(F)
    cell = np.clip(np.floor((c - origin) * (F(1.0) / h)), 0, dims - 1).astype(np.int64)
    return dict(mu=mu, h=h, origin=origin, dims=dims, cell=cell)


def query_blocks(g, pts, guess):
    G = guess.copy(); G[:3, 3] -= g["mu"]                    # T(-mu) * guess
    qd = (pts.astype(np.float64) @ G[:3, :3].T + G[:3, 3]).astype(F)
    h, inv_h = g["h"], F(1.0) / g["h"]
    rs = F(np.sqrt(F(RADIUS) * F(RADIUS))) * F(1.0001) + F(1.0e-3) * h
    cc = lambda v: np.floor(np.clip((v - g["origin"]) * inv_h, -1.0e6, 1.0e6)).astype(np.int64)
    lo = np.maximum(cc(qd - rs), 0); hi = np.minimum(cc(qd + rs), g["dims"] - 1)
    ok = np.isfinite(qd).all(axis=1) & (lo <= hi).all(axis=1)
    return qd, lo, hi, ok


def box_of(lo, hi, ok, tcell):
    """(entries, rows, points) of the box of the lanes `ok`; None without a searching lane."""
    if not ok.any():
        return None
    b0, b1 = lo[ok].min(axis=0), hi[ok].max(axis=0)
    n = (b1 - b0 + (2, 1, 1)).tolist()
    return n[0] * n[1] * n[2], n[1] * n[2], int(((tcell >= b0) & (tcell <= b1)).all(axis=1).sum())


def fits(b, frac=1.0, point_cap=POINT_CAP, table_cap=TABLE_CAP):
    e, r, p = b
    return e <= table_cap * frac, e <= table_cap * frac and r <= ROW_CAP * frac and p <= point_cap * frac


def count_pair(k, n_points):
    src, tgt, guess = bench_pair(k, n_points)
    from oracle import icp_fast
    q, n, _ = icp_fast.calculate_normals(tgt[:, :3].astype(np.float64))
    q = q[np.isfinite(n).all(axis=1)]
    g = target_grid(q)
    nx, ny, nz = g["dims"].tolist()
    pts = morton_order(src)
    qd, lo, hi, ok = query_blocks(g, pts, guess)
    tcell = g["cell"]
    print(f"pair {k}: {len(pts)} queries, {len(q)} target points, grid {nx} x {ny} x {nz} cells of {float(g['h']):.4f} m")
    rounds = [(r, box_of(lo[r:r + 256], hi[r:r + 256], ok[r:r + 256], tcell)) for r in range(0, len(pts), 256)]
    rounds = [(r, b) for r, b in rounds if b is not None]
    staged = [fits(b)[1] for r, b in rounds]
    table = [fits(b)[0] and not fits(b)[1] for r, b in rounds]
    glob = [not fits(b)[0] for r, b in rounds]
    N = len(rounds)
    print(f"  rounds {N}: staged {100 * sum(staged) / N:.1f} %, table only {100 * sum(table) / N:.1f} %, global {100 * sum(glob) / N:.1f} %")
    # the rounds that are not staged, cut into their waves' / half workgroups' boxes
    for lanes, frac, what in ((64, 0.25, "a quarter of the caps"), (128, 0.5, "half of the caps"), (64, 1.0, "the full caps")):
        n_part = n_tab = n_full = n_all = n_rounds = 0
        for (r, b), s in zip(rounds, staged):
            if s:
                continue
            parts = [box_of(lo[a:a + lanes], hi[a:a + lanes], ok[a:a + lanes], tcell) for a in range(r, min(r + 256, len(pts)), lanes)]
            parts = [p for p in parts if p is not None]
            f = [fits(p, frac) for p in parts]
            n_part += len(parts); n_tab += sum(t for t, _ in f); n_full += sum(a for _, a in f)
            n_rounds += 1; n_all += all(a for _, a in f)
        print(f"  boxes of {lanes} queries under {what}: {100 * n_full / n_part:.1f} % stage fully, the table fits for {100 * n_tab / n_part:.1f} %, "
              f"every box of the round fits in {100 * n_all / n_rounds:.1f} % of the {n_rounds} rounds")
    t_rounds = [b for (r, b), t in zip(rounds, table) if t]
    if t_rounds:
        miss_rows = sum(b[1] > ROW_CAP for b in t_rounds)
        print(f"  table-only rounds {len(t_rounds)}: {miss_rows} miss the row cap; a point cap of " +
              ", ".join(f"{c} would stage {100 * sum(fits(b, point_cap=c)[1] for b in t_rounds) / len(t_rounds):.0f} %" for c in (640, 768, 832, 1024)))
    print("  a table cap of " + ", ".join(f"{c} leaves {100 * sum(not fits(b, table_cap=c)[0] for r, b in rounds) / N:.1f} % global" for c in (2048, 4096)))
    # the global rounds query by query: the slots of a lane's walk are the rows (z, y) of its block in ascending order
    occ, cnt = np.unique((tcell[:, 2] * ny + tcell[:, 1]) * nx + tcell[:, 0], return_counts=True)
    cum = np.concatenate([[0], np.cumsum(cnt)])
    sel = np.concatenate([np.arange(r, min(r + 256, len(pts))) for (r, b), gl in zip(rounds, glob) if gl])
    sel = sel[ok[sel]]
    nyr = hi[sel, 1] - lo[sel, 1] + 1
    nrows = nyr * (hi[sel, 2] - lo[sel, 2] + 1)
    S = int(nrows.max())
    s = np.arange(S)[None, :]
    live = s < nrows[:, None]
    z = lo[sel, 2][:, None] + s // nyr[:, None]; y = lo[sel, 1][:, None] + s % nyr[:, None]
    h, o = g["h"], g["origin"]
    slack = F(2.0e-3) * h
    zl = o[2] + z.astype(F) * h; yl = o[1] + y.astype(F) * h
    dz = np.maximum(np.maximum(zl - qd[sel, 2][:, None], qd[sel, 2][:, None] - (zl + h)) - slack, 0)
    dy = np.maximum(np.maximum(yl - qd[sel, 1][:, None], qd[sel, 1][:, None] - (yl + h)) - slack, 0)
    visit = live & ~(dy * dy + dz * dz > F(RADIUS) * F(RADIUS))
    base = (z * ny + y) * nx
    run = cum[np.searchsorted(occ, base + hi[sel, 0][:, None], side="right")] - cum[np.searchsorted(occ, base + lo[sel, 0][:, None], side="left")]
    run = np.where(visit, run, 0)
    print(f"  per query of the global rounds ({len(sel)}): {visit.sum(axis=1).mean():.1f} rows visited, {(run > 0).sum(axis=1).mean():.1f} with a cell in range, "
          f"{run.sum(axis=1).mean():.1f} candidates, {100 * (run.sum(axis=1) == 0).mean():.0f} % without any")
    # dependent levels a wave: lanes of one wave are 64 consecutive queries of a round
    wave = sel // 64
    one, together, four = [], [], []
    g4 = -(-run // 4)                                              # groups of four loads a run
    pad = (-S) % 4
    run4 = np.pad(run, ((0, 0), (0, pad))).reshape(len(sel), -1, 4).sum(axis=2)
    vis4 = np.pad(visit, ((0, 0), (0, pad))).reshape(len(sel), -1, 4).any(axis=2)
    for w in np.unique(wave):
        m = wave == w
        one.append(int(visit[m].any(axis=0).sum() + (run[m] > 0).any(axis=0).sum() + g4[m].max(axis=0).sum()))
        together.append(int(visit[m].any()) + int((run[m] > 0).any()) + int(g4[m].sum(axis=1).max()))
        four.append(int(vis4[m].any(axis=0).sum() + (run4[m] > 0).any(axis=0).sum() + (-(-run4[m] // 4)).max(axis=0).sum()))
    for name, v in (("a row at a time", one), ("all rows in flight together", together), ("four rows at a time, one sequence", four)):
        print(f"  levels a wave and global round, {name}: mean {np.mean(v):.1f}, median {np.median(v):.0f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", default="0,30,100,300")
    ap.add_argument("--points", type=int, default=120_000)
    a = ap.parse_args()
    for k in (int(v) for v in a.pairs.split(",")):
        count_pair(k, a.points)


if __name__ == "__main__":
    main()
