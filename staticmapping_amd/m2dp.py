"""ctypes view of the device M2DP descriptor (include/smhip.h, `smhip_m2dp_*`): descriptor::M2dp of the reference
(descriptor/m2dp.{h,cc}) -- setInputCloud + getFinalDescriptor on an uploaded cloud or on the filter workspace's current
cloud (a filter chain's output or a built submap), and matchTwoM2dpDescriptors.  No compute happens in Python."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _capi


def make_options(r: float | None = None, max_distance: float | None = None, t: int | None = None, p: int | None = None,
                 q: int | None = None) -> _capi.M2dpOptions:
    """M2dp's constructor arguments (m2dp.h:48-49: 0.1, 100, 16, 4, 16); None = the default."""
    o = _capi.M2dpOptions()
    _capi.load_library().smhip_m2dp_default_options(ctypes.byref(o))
    for name, v in (("r", r), ("max_distance", max_distance), ("t", t), ("p", p), ("q", q)):
        if v is not None:
            setattr(o, name, v)
    return o


def length(options: _capi.M2dpOptions | None = None) -> int:
    """p*q + l*t, or -1 when the device refuses the options"""
    return _capi.load_library().smhip_m2dp_length(ctypes.byref(options or make_options()))


def _out(options):
    n = length(options)
    return np.zeros(max(n, 0), np.float32), n


def m2dp(matcher, points, options: _capi.M2dpOptions | None = None) -> np.ndarray:
    """The descriptor (float32 [p*q + l*t]) of float32 rows [n, 4] (x y z intensity) or [n, 5] (InnerPointType)."""
    options = options or make_options()
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float32))
    if pts.ndim != 2:
        raise ValueError("points must be a 2-d float32 array of 4 or 5 columns")
    out, n = _out(options)
    matcher._check(matcher._lib.smhip_m2dp_f32(matcher._h, pts.ctypes.data_as(_capi.c_float_p), pts.shape[1], len(pts), ctypes.byref(options),
                                               out.ctypes.data_as(_capi.c_float_p), n))
    return out


def m2dp_from_filter_output(matcher, options: _capi.M2dpOptions | None = None) -> np.ndarray:
    """The descriptor of the filter workspace's current cloud, which stays on the device and unchanged."""
    options = options or make_options()
    out, n = _out(options)
    matcher._check(matcher._lib.smhip_m2dp_from_filter_output(matcher._h, ctypes.byref(options), out.ctypes.data_as(_capi.c_float_p), n))
    return out


def last(matcher, n: int, options: _capi.M2dpOptions | None = None):
    """Parity hook: (projected3 float32 [n, 3], kept bool [n], A int32 [p*q, l*t], n_kept) of the last descriptor call, which
    saw n rows and `options`."""
    options = options or make_options()
    views = options.p * options.q
    if length(options) < 0:
        raise ValueError("the device refuses these M2dp options (smhip_m2dp_length is -1)")
    cols = length(options) - views
    proj = np.zeros((n, 3), np.float32)
    kept = np.zeros(n, np.int32)
    A = np.zeros((views, cols), np.int32)
    n_kept = ctypes.c_int()
    matcher._check(matcher._lib.smhip_m2dp_last(matcher._h, proj.ctypes.data_as(_capi.c_float_p), kept.ctypes.data_as(_capi.c_int32_p),
                                                A.ctypes.data_as(_capi.c_int32_p), A.size, ctypes.byref(n_kept)))
    return proj, kept.astype(bool), A, n_kept.value


def match(P, Q) -> float:
    """matchTwoM2dpDescriptors (m2dp.cc:151-169): the score in (0, 1), or -1 for unequal or short (< 10) descriptors."""
    P = np.ascontiguousarray(np.asarray(P, dtype=np.float32).ravel())
    Q = np.ascontiguousarray(np.asarray(Q, dtype=np.float32).ravel())
    if len(P) != len(Q):
        return -1.0
    return float(_capi.load_library().smhip_m2dp_match(P.ctypes.data_as(_capi.c_float_p), Q.ctypes.data_as(_capi.c_float_p), len(P)))
