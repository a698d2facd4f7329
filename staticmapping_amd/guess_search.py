"""ctypes view of the device correlative guess search (include/smhip.h, `smhip_guess_search_*`): every transform of a window around a
guess scored by how many source points land in an occupied target voxel, and the best one returned -- what LoopDetector::CloseLoop
can start its ICP from when the drifted poses are metres off.  No compute happens in Python."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _capi

OPTION_NAMES = ("resolution", "max_source_points", "half_xy", "half_z", "yaw_steps", "yaw_step")


def make_options(**options) -> _capi.GuessSearchOptions:
    """The defaults (0.5 m, 4096 points, +-20 x +-20 x +-2 voxels, +-10 steps of 2 degrees; yaw_step is in radians) with `options` set."""
    o = _capi.GuessSearchOptions()
    _capi.load_library().smhip_guess_search_default_options(ctypes.byref(o))
    for name, v in options.items():
        if name not in OPTION_NAMES:
            raise TypeError(f"unknown guess-search option {name!r}")
        setattr(o, name, v)
    return o


def _rows(cloud):
    pts = np.ascontiguousarray(np.asarray(cloud, dtype=np.float32))
    if pts.ndim != 2:
        raise ValueError("a cloud must be a 2-d float32 array of 4 or 5 columns")
    return pts


def search(matcher, target, source, guess, **options) -> dict:
    """target / source: float32 rows [n, 4] (x y z intensity) or [n, 5] (InnerPointType); guess: 4 x 4.  Returns a dict: transform
    (4 x 4 float64), best (a, i, j, k), best_score, guess_score, runner_up_score, n_source_used, n_candidates."""
    o = make_options(**options)
    t, s = _rows(target), _rows(source)
    g = np.ascontiguousarray(np.asarray(guess, np.float64).reshape(4, 4).T)          # column-major
    r = _capi.GuessSearchResult()
    matcher._check(matcher._lib.smhip_guess_search_f32(matcher._h, t.ctypes.data_as(_capi.c_float_p), len(t), t.shape[1], s.ctypes.data_as(_capi.c_float_p),
                                                       len(s), s.shape[1], g.ctypes.data_as(_capi.c_double_p), ctypes.byref(o), ctypes.byref(r)))
    out = dict(transform=np.array(r.transform[:], np.float64).reshape(4, 4).T.copy(), best=(r.best_yaw, r.best_i, r.best_j, r.best_k),
               best_score=r.best_score, guess_score=r.guess_score, runner_up_score=r.runner_up_score, n_source_used=r.n_source_used,
               n_candidates=r.n_candidates, options=o)
    matcher._guess_search_result = out                  # the sizes last() needs
    return out


def last(matcher, result: dict | None = None) -> dict:
    """Parity hook, for the last search() that completed on this matcher (`result`: what it returned; None = the one search() remembers):
    volume int32 [yaws, nz, nxy, nxy] (a, k, j, i), origin and extent of the bitmap's box (voxels, int32 [3]) and voxels int32
    [yaws, n_source_used, 3] -- INT32_MIN for a point that no offset of the window brings into the box."""
    if result is None:
        result = getattr(matcher, "_guess_search_result", None)
        if result is None:
            raise ValueError("no search() has completed on this matcher")
    o = result["options"]
    nyaw, nz, nxy, m = 2 * o.yaw_steps + 1, 2 * o.half_z + 1, 2 * o.half_xy + 1, result["n_source_used"]
    volume = np.zeros((nyaw, nz, nxy, nxy), np.int32)
    origin, extent = np.zeros(3, np.int32), np.zeros(3, np.int32)
    voxels = np.zeros((nyaw, m, 3), np.int32)
    p = _capi.c_int32_p
    matcher._check(matcher._lib.smhip_guess_search_last(matcher._h, volume.ctypes.data_as(p), volume.size, origin.ctypes.data_as(p), extent.ctypes.data_as(p),
                                                        voxels.ctypes.data_as(p), voxels.size))
    return dict(volume=volume, origin=origin, extent=extent, voxels=voxels)
