"""ctypes view of the device pre-filters (include/smhip.h, `smhip_filter_*`): the Python mirror of
pre_processers::filter::{Range, AxisRange, BoundingBoxRemoval, RandomSampler, VoxelGrid, GroundRemoval, GroundRemoval2,
RangeImage, StatisticRemoval, Factory} (the reference's pre_processors/filter_*.cc).  Filters are descriptors set by the
reference's parameter names: `FilterDesc` for the first five, `FilterDescEx` for GroundRemoval, GroundRemoval2, RangeImage and
StatisticRemoval (k-NN outlier removal; the reference ships only its parameters, the definition is in DESIGN.md §6)."""
from __future__ import annotations

import ctypes
import re

import numpy as np

from . import _capi

RANGE, AXIS_RANGE, RANDOM_SAMPLER, VOXEL_GRID, BOUNDING_BOX_REMOVAL = 1, 2, 3, 4, 5
GROUND_REMOVAL, GROUND_REMOVAL2, RANGE_IMAGE = 6, 7, 8
STATISTIC_REMOVAL = 9
NAMES = {"Range": RANGE, "AxisRange": AXIS_RANGE, "RandomSampler": RANDOM_SAMPLER, "VoxelGrid": VOXEL_GRID,
         "BoundingBoxRemoval": BOUNDING_BOX_REMOVAL}
GROUND_NAMES = {"GroundRemoval": GROUND_REMOVAL, "GroundRemoval2": GROUND_REMOVAL2, "RangeImage": RANGE_IMAGE}
STATISTIC_NAMES = {"StatisticRemoval": STATISTIC_REMOVAL}
_PARAMS = {RANGE: ("min_range", "max_range"), AXIS_RANGE: ("min", "max"), RANDOM_SAMPLER: ("sampling_rate",),
           VOXEL_GRID: ("voxel_size",), BOUNDING_BOX_REMOVAL: ("min_x", "min_y", "min_z", "max_x", "max_y", "max_z")}
# the FilterDescEx slots of the new filters (include/smhip.h): name -> ("p" | "i", index)
_PARAMS_EX = {
    GROUND_REMOVAL: {"leaf_size": ("p", 0), "height_threshold": ("p", 1), "min_point_num_in_voxel": ("i", 0)},
    GROUND_REMOVAL2: {"r_max": ("p", 0), "r_min": ("p", 1), "start_ground_height": ("p", 2), "long_line_threshold": ("p", 3),
                      "max_long_line_height": ("p", 4), "max_start_height": ("p", 5), "max_error": ("p", 6), "max_slope": ("p", 7),
                      "max_b": ("p", 8), "max_dist_to_line": ("p", 9), "search_angle": ("p", 10), "bin_num": ("i", 0),
                      "segment_num": ("i", 1), "thread_num": ("i", 2)},
    RANGE_IMAGE: {"top_angle": ("p", 0), "btm_angle": ("p", 1), "offset_x": ("p", 2), "offset_y": ("p", 3), "offset_z": ("p", 4),
                  "vertical_line_num": ("i", 0), "horizontal_line_num": ("i", 1)},
    STATISTIC_REMOVAL: {"std_mul": ("p", 0), "point_num_meank": ("i", 0)}}       # filter_statistic_removal.cc:33-36


def make_filter(name_or_type, **params):
    """A filter with its constructor defaults, then `params` (reference names; plus `axis_index`, `seed`).
    GroundRemoval, GroundRemoval2, RangeImage and StatisticRemoval give a FilterDescEx, the others a FilterDesc."""
    t = {**NAMES, **GROUND_NAMES, **STATISTIC_NAMES}[name_or_type] if isinstance(name_or_type, str) else int(name_or_type)
    if t in _PARAMS_EX:
        d = _capi.FilterDescEx()
        _capi.load_library().smhip_filter_default_ex(t, ctypes.byref(d))
        for k, v in params.items():
            if k not in _PARAMS_EX[t]:
                raise KeyError(f"{k} is not a parameter of filter type {t}")
            arr, slot = _PARAMS_EX[t][k]
            if arr == "i":
                d.i[slot] = int(v)
            else:
                d.p[slot] = float(v)
        return d
    d = _capi.FilterDesc()
    _capi.load_library().smhip_filter_default(t, ctypes.byref(d))
    for k, v in params.items():
        if k == "axis_index":
            d.axis_index = int(v)
        elif k == "seed":
            d.seed = int(v)
        elif k in _PARAMS[t]:
            d.p[_PARAMS[t].index(k)] = float(v)
        else:
            raise KeyError(f"{k} is not a parameter of filter type {t}")       # SetValue -> CHECK(all_right), filter_interface.cc:58
    return d


def config_valid(d) -> bool:
    if isinstance(d, _capi.FilterDescEx):
        return bool(_capi.load_library().smhip_filter_config_valid_ex(ctypes.byref(d)))
    return bool(_capi.load_library().smhip_filter_config_valid(ctypes.byref(d)))


def widen(d) -> _capi.FilterDescEx:
    """A FilterDesc as the FilterDescEx that selects the same filter (axis_index -> i[0])."""
    if isinstance(d, _capi.FilterDescEx):
        return d
    e = _capi.FilterDescEx()
    e.type, e.seed, e.i[0] = d.type, d.seed, d.axis_index
    for k in range(6):
        e.p[k] = d.p[k]
    return e


def chain_from_xml(text: str, seed: int = 0, ground_filters: bool = False, statistic_removal: bool = False) -> list:
    """The <filters> element of the reference's configs (filter_factory.cc:47-81): unsupported names are skipped.
    ground_filters=True also takes GroundRemoval, GroundRemoval2 and RangeImage, and skips <!-- ... --> comments as pugixml
    does (the default keeps the historical parse, which reads filters inside comments too).
    statistic_removal=True also takes StatisticRemoval: opt-in because the reference's own Filter() for that name is a stub that
    leaves its output cloud empty, so a port that lists it gets a different chain here than there."""
    if ground_filters:
        text = re.sub(r"<!--.*?-->", "", text, flags=re.S)
    names = {**NAMES, **GROUND_NAMES} if ground_filters else dict(NAMES)
    if statistic_removal:
        names.update(STATISTIC_NAMES)
    out = []
    for m in re.finditer(r'<filter\s+name="([^"]+)"\s*(?:/>|>(.*?)</filter>)', text, flags=re.S):
        name, body = m.group(1), m.group(2) or ""
        if name not in names:
            continue
        params = {}
        for p in re.finditer(r'<param\s+type="(\d)"\s+name="([^"]+)"\s*>\s*([^<]*?)\s*</param>', body):
            params[p.group(2)] = int(float(p.group(3))) if p.group(1) == "0" else float(p.group(3))
        if names[name] == RANDOM_SAMPLER:
            params.setdefault("seed", seed + len(out))
        out.append(make_filter(name, **params))
    return out


def _launch(matcher, a, chain, n_out):
    """smhip_filter_chain_f32 when every descriptor is a FilterDesc, else smhip_filter_chain_ex_f32 on the widened chain"""
    if all(isinstance(d, _capi.FilterDesc) for d in chain):
        arr = (_capi.FilterDesc * max(1, len(chain)))(*chain)
        fn = matcher._lib.smhip_filter_chain_f32
    else:
        arr = (_capi.FilterDescEx * max(1, len(chain)))(*[widen(d) for d in chain])
        fn = matcher._lib.smhip_filter_chain_ex_f32
    matcher._check(fn(matcher._h, a.ctypes.data_as(_capi.c_float_p), a.shape[1], a.shape[0], arr, len(chain), ctypes.byref(n_out)))


def run_chain(matcher, points, chain):
    """Factory::Filter on the device.  points: float32 [N,4] (KITTI rows) or [N,5] (InnerPointType rows).
    `chain` may mix FilterDesc and FilterDescEx.  Returns (filtered [M,5] float32, source_index [M] int32)."""
    a = np.ascontiguousarray(np.asarray(points, dtype=np.float32))
    n_out = ctypes.c_int()
    _launch(matcher, a, chain, n_out)
    out = np.zeros((n_out.value, 5), np.float32)
    src = np.zeros(n_out.value, np.int32)
    matcher._check(matcher._lib.smhip_filter_get_output(matcher._h, out.ctypes.data_as(_capi.c_float_p),
                                                        src.ctypes.data_as(_capi.c_int32_p), n_out.value))
    return out, src


def statistic_last(matcher, n: int):
    """What the last StatisticRemoval of the last chain computed (smhip_filter_statistic_last).  n = the rows that filter saw
    (the chain's input size when it is the first filter).  Returns (distance [n] float32 in that row order, 0 for a non-finite
    row; {"sum", "sq_sum", "V", "threshold"})."""
    dist = np.zeros(n, np.float32)
    stats = np.zeros(4, np.float64)
    matcher._check(matcher._lib.smhip_filter_statistic_last(matcher._h, dist.ctypes.data_as(_capi.c_float_p), n,
                                                           stats.ctypes.data_as(_capi.c_double_p)))
    return dist, {"sum": float(stats[0]), "sq_sum": float(stats[1]), "V": int(stats[2]), "threshold": float(stats[3])}


def run_chain_resident(matcher, points, chain) -> int:
    """The same without reading the result back: returns the filtered size; follow with output_to_source()."""
    a = np.ascontiguousarray(np.asarray(points, dtype=np.float32))
    n_out = ctypes.c_int()
    _launch(matcher, a, chain, n_out)
    return n_out.value


def output_to_source(matcher, slot: int = 0):
    """The filtered cloud becomes the source of `slot` on the device (output_to_source_compensated de-skews it on the way)."""
    matcher._check(matcher._lib.smhip_filter_output_to_source(matcher._h, slot))


def output_to_source_compensated(matcher, delta, slot: int = 0, download: bool = False):
    """MotionCompensation (builder/map_builder.cc:232-257) of the filtered cloud by the 4x4 `delta` -> source of `slot`, on the
    device; the filter workspace keeps its cloud, so the call can be repeated with another delta.  download=True returns the
    compensated cloud as [M,5] float32 rows in the workspace's row order."""
    d = np.asarray(delta, dtype=np.float64)
    if d.shape != (4, 4):
        raise ValueError("delta must be a 4x4 matrix")
    d = np.ascontiguousarray(d.T)                      # column-major for the C ABI
    if not download:
        matcher._check(matcher._lib.smhip_filter_output_to_source_compensated(matcher._h, slot, d.ctypes.data_as(_capi.c_double_p), None))
        return None
    cap, m = ctypes.c_int(), ctypes.c_int()            # the filtered size is at most max_source_points, or the call refuses
    matcher._check(matcher._lib.smhip_get_capacity(matcher._h, None, ctypes.byref(cap), None))
    out = np.empty((cap.value, 5), np.float32)
    matcher._check(matcher._lib.smhip_filter_output_to_source_compensated(matcher._h, slot, d.ctypes.data_as(_capi.c_double_p),
                                                                         out.ctypes.data_as(_capi.c_float_p)))
    matcher._check(matcher._lib.smhip_get_cloud_sizes(matcher._h, slot, ctypes.byref(m), None, None))
    return out[:m.value].copy()
