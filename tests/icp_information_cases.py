"""The pairs tests/test_icp_information_gpu.py runs smhip_icp_information on: the smallest shapes at which the kernel can go wrong.
A workgroup of the kernel takes 2 048 rows, 256 at a time: 63 rows are a partial wave, 257 a partial workgroup round, 1 999 an odd
tail; one pair carries a NaN row, one lies beyond every search, one has no finite row at all.

The seeds are chosen so that no kept query's runner-up lies within 1e-4 (relative, squared distances) of its match: the device
finds its matches in f32, the restatement in f64, and a nearer tie could be broken either way.  near_tie_margin() measures it;
tests/test_icp_information_ref.py asserts it on the CPU, the GPU test again on the device's own values."""
import json
import os

import numpy as np

import icp_information_ref as info

HERE = os.path.dirname(os.path.abspath(__file__))
RATIO = 0.7


def _three_planes():
    from oracle import icp_fast as o
    from staticmapping_amd import synth
    g = json.load(open(os.path.join(HERE, "golden", "icp_three_planes_2000.json")))
    tgt, src, _ = synth.three_planes_pair(2000, seed=11, sigma=0.01)
    q, n, _ = o.calculate_normals(tgt[:, :3].astype(np.float64))
    f = lambda a: a.astype(np.float32).astype(np.float64)
    return dict(name="three_planes_2000", src=src, tgt=f(q), nrm=f(n), T=np.array(g["result"]))


def _surface(name, faces, n_src, n_tgt, seed):
    src, tgt, nrm, T = info.surface_pair(faces, n_src, n_tgt, seed)
    return dict(name=name, src=src, tgt=tgt, nrm=nrm, T=T)


_CACHE = {}


def cases():
    """name -> dict(src [N, 4] f32, tgt / nrm [M, 3] (f32 values as f64), T source -> target); computed once"""
    if _CACHE:
        return _CACHE
    out = [_three_planes(),
           _surface("plane_63", info.PLANE, 63, 300, seed=21),
           _surface("plane_257", info.PLANE, 257, 600, seed=22),
           _surface("corridor_1999", info.CORRIDOR, 1999, 2000, seed=23),
           _surface("corridor_2000_nan_row", info.CORRIDOR, 2000, 1500, seed=24),
           _surface("plane_far", info.PLANE, 300, 300, seed=25),
           _surface("all_nan", info.PLANE, 8, 300, seed=26)]
    by = {c["name"]: c for c in out}
    by["corridor_2000_nan_row"]["src"][1234, 1] = np.nan
    by["plane_far"]["src"][:, 0] += 400.0                  # every match is hundreds of metres away: beyond every bounded search
    by["all_nan"]["src"][:, :3] = np.nan
    _CACHE.update(by)
    return _CACHE


REGULAR = ["three_planes_2000", "plane_63", "plane_257", "corridor_1999", "corridor_2000_nan_row"]


def moved_f32(src, T, mu):
    """the moved, centred source as the searches see it: R s + (t - mu) in f64, rounded to f32"""
    s = src[:, :3].astype(np.float64)
    return (s @ T[:3, :3].T + (T[:3, 3] - mu)).astype(np.float32).astype(np.float64)


def near_tie_margin(moved, centred_tgt, keep=None, ratio=RATIO):
    """(the smallest (d2_runner_up - d2_match) / d2_match over the kept rows, brute-force ids, d2).  keep: the kept mask to use
    (the device's); default: the restatement's own."""
    ids, d2, d2b = info.brute_matches(moved, centred_tgt, second=True)
    if keep is None:
        keep = info.kept_set(d2, ratio)[0]
    k = np.nonzero(keep)[0]
    rel = (d2b[k] - d2[k]) / np.maximum(d2[k], 1e-30)
    return (float(rel.min()) if len(k) else np.inf), ids, d2
