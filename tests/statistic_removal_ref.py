"""numpy restatement of StatisticRemoval -- the yardstick of the device filter (staticmapping_amd/csrc/statistic_removal.hip).

The reference's pre_processors/filter_statistic_removal.cc gives the filter its name, its two parameters and their defaults
(:31-37: point_num_meank = 30, std_mul = 1.0); its Filter (:44-59) holds only a commented-out pcl::StatisticalOutlierRemoval
call (setMeanK(point_num_meank_), setStddevMulThresh(std_mul_)) and a TODO.  What is restated here is therefore this project's
definition ("StatisticRemoval"): the PCL 1.8 algorithm with every operation and its order fixed, brute force.

  1  a row is finite iff x, y and z are; V = number of finite rows
  2  V <= k: every row is kept (`passed_through`)
  3  d2(a, b) = ((dx*dx) + (dy*dy)) + (dz*dz) in float32, every operation rounded on its own
  4  distance[i] = float32(sum over the k smallest d2(i, j), j != i finite, ascending, of sqrt(float64(d2)), in float64) / k)
  5  a non-finite row has distance 0, is no one's neighbour and is not counted in V
  6  sum, sq_sum of float64(distance) over the rows in the device's order (`ordered_sums`), mean = sum / V,
     variance = (sq_sum - sum*sum / V) / (V - 1), threshold = mean + float64(float32(std_mul)) * sqrt(variance)
  7  a row is removed iff it is finite and float64(distance[i]) > threshold
Rows are float32 [N, >= 3]; only x, y, z are read.
"""
from __future__ import annotations

import math

import numpy as np

F = np.float32
STATISTIC_REMOVAL = 9
DEFAULTS = dict(std_mul=1.0, point_num_meank=30)          # filter_statistic_removal.cc:31-37


def config_valid(std_mul: float, point_num_meank: int) -> bool:
    return 1 <= int(point_num_meank) <= 64 and bool(np.isfinite(F(std_mul)))


def finite_rows(rows: np.ndarray) -> np.ndarray:
    return np.isfinite(np.asarray(rows, dtype=F)[:, :3]).all(axis=1)


def d2_float(q: np.ndarray, p: np.ndarray) -> np.ndarray:
    """step 3 for every pair: q [A, 3], p [B, 3] float32 -> [A, B] float32 (numpy rounds every float32 operation on its own)"""
    with np.errstate(over="ignore"):
        dx = q[:, None, 0] - p[None, :, 0]
        dy = q[:, None, 1] - p[None, :, 1]
        dz = q[:, None, 2] - p[None, :, 2]
        return ((dx * dx) + (dy * dy)) + (dz * dz)


def mean_of_sorted(d2_sorted: np.ndarray, k: int) -> np.ndarray:
    """step 4's sum for rows of k ascending float32 d2 values"""
    s = np.zeros(len(d2_sorted), np.float64)
    for m in range(k):
        s = s + np.sqrt(d2_sorted[:, m].astype(np.float64))
    return (s / np.float64(k)).astype(F)


def mean_distances(rows: np.ndarray, k: int, chunk: int | None = None) -> np.ndarray:
    """steps 3-5, brute force in chunks of query rows.  Needs V > k."""
    xyz = np.ascontiguousarray(np.asarray(rows, dtype=F)[:, :3])
    idx = np.flatnonzero(finite_rows(xyz))
    p = xyz[idx]
    v = len(p)
    assert v > k
    if chunk is None:
        chunk = max(16, min(512, 6_000_000 // v))
    dist = np.zeros(len(xyz), F)
    for a in range(0, v, chunk):
        q = p[a:a + chunk]
        d2 = d2_float(q, p)
        d2[np.arange(len(q)), a + np.arange(len(q))] = np.inf          # j != i (a duplicate of i stays, at 0)
        best = np.partition(d2, k - 1, axis=1)[:, :k]                   # the k smallest: one multiset whatever the ties
        best.sort(axis=1)
        dist[idx[a:a + len(q)]] = mean_of_sorted(best, k)
    return dist


def fold64(a: np.ndarray) -> np.ndarray:
    """[..., 64] -> [...]: 64 values become 32 by v[l] + v[l + 32], then 16 by v[l] + v[l + 16], ... (the device's wave fold)"""
    w = 64
    while w > 1:
        h = w // 2
        a = a[..., :h] + a[..., h:w]
        w = h
    return a[..., 0]


def ordered_sums(distance: np.ndarray) -> tuple[float, float]:
    """step 6's sums in the device's order: chunks of 64 consecutive rows folded by fold64 (non-finite rows add their 0), the
    chunk sums dealt to 64 columns (chunk c to column c mod 64), each column summed in ascending c, the columns folded."""
    d = np.asarray(distance, dtype=F).astype(np.float64)
    n = len(d)
    c = (n + 63) // 64
    pad = np.zeros(c * 64, np.float64)
    pad[:n] = d

    def total(chunk_sums):
        r = (c + 63) // 64
        p = np.zeros(r * 64, np.float64)
        p[:c] = chunk_sums
        col = np.zeros(64, np.float64)
        for row in p.reshape(r, 64):
            col = col + row
        return float(fold64(col))

    return total(fold64(pad.reshape(c, 64))), total(fold64((pad * pad).reshape(c, 64)))


def threshold_from_sums(s: float, sq: float, v: int, std_mul: float) -> float:
    mean = s / v
    variance = (sq - s * s / v) / (v - 1)
    stddev = math.sqrt(variance) if variance >= 0 else math.nan       # a NaN threshold removes nothing
    return mean + float(F(std_mul)) * stddev


def decide(rows: np.ndarray, distance: np.ndarray, std_mul: float) -> dict:
    """steps 6-7 for given distances"""
    fin = finite_rows(rows)
    v = int(fin.sum())
    s, sq = ordered_sums(distance)
    thr = threshold_from_sums(s, sq, v, std_mul)
    keep = ~(fin & (distance.astype(np.float64) > thr))
    return dict(keep=keep, distance=distance, sum=s, sq_sum=sq, V=v, threshold=thr, passed_through=False)


def statistic_removal(rows: np.ndarray, std_mul: float = 1.0, point_num_meank: int = 30, distance: np.ndarray | None = None) -> dict:
    """The filter on `rows`.  `distance`: step 4's result when the caller already has it (it depends on k alone)."""
    if not config_valid(std_mul, point_num_meank):
        raise ValueError("ConfigsValid() is false")
    rows = np.asarray(rows, dtype=F)
    v = int(finite_rows(rows).sum())
    if v <= point_num_meank:
        return dict(keep=np.ones(len(rows), bool), distance=None, sum=None, sq_sum=None, V=v, threshold=None, passed_through=True)
    if distance is None:
        distance = mean_distances(rows, point_num_meank)
    return decide(rows, distance, std_mul)
