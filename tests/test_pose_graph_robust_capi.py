"""smhip_pose_graph_plan_robust -- the host half of smhip_pose_graph_optimize_robust -- and smhip_pose_graph_last_robust's refusals
without a GPU, through ctypes (staticmapping_amd.pose_graph.plan_robust): a threshold that is negative or not finite is refused with
its factor named, beside every refusal of the _factors form, which come in the same words; thresholds change nothing of the plan."""
import ctypes

import numpy as np
import pytest

import pose_graph_robust_cases as cases
from staticmapping_amd import _capi, pose_graph
from test_pose_graph_gps_capi import small

INVALID, CAPACITY = 1, 7


def _plan(g, huber, **change):
    a = {**dict(poses=g["poses"], kinds=g["kinds"], ij=g["ij"], data=g["data"], fixed=g["fixed"], sigmas=g["sigmas"]), **change}
    return pose_graph.plan_robust(a["poses"], a["kinds"], a["ij"], a["data"], fixed=a["fixed"], sigmas=a["sigmas"], huber=huber)


def test_the_symbols_are_exported_with_their_signatures():
    lib = _capi.load_library()
    for name in ("smhip_pose_graph_plan_robust", "smhip_pose_graph_optimize_robust", "smhip_pose_graph_last_robust"):
        assert name in _capi.SIGNATURES and getattr(lib, name) is not None


def test_thresholds_leave_the_plan_as_it_is():
    g = small()
    m = len(g["kinds"])
    want = pose_graph.plan_factors(g["poses"], g["kinds"], g["ij"], g["data"], fixed=g["fixed"], sigmas=g["sigmas"])
    for hub in (None, np.zeros(m), np.full(m, 1.0), 2.5, np.arange(m, dtype=float), np.full(m, 1e300)):
        off, inc = _plan(g, hub)
        assert (off == want[0]).all() and (inc == want[1]).all()
    r = cases.graph("robust16")
    off, inc = _plan(r, r["huber"])
    assert off[-1] == 2 * len(r["kinds"]) and list(inc[off[3]:off[4]]) == [2, 3, 18]       # node 3: its chain edges and the corrupted loop


def test_a_threshold_that_is_negative_or_not_finite_is_refused():
    g = small()
    m = len(g["kinds"])
    for bad in (-1.0, -1e-300, np.nan, np.inf, -np.inf):
        for e in range(m):                                     # BETWEEN, PRIOR and POINT factors alike
            hub = np.ones(m)
            hub[e] = bad
            with pytest.raises(pose_graph.PoseGraphRefused, match="edge %d has a Huber threshold that is negative or not finite" % e) as err:
                _plan(g, hub)
            assert err.value.status == INVALID
    with pytest.raises(pose_graph.PoseGraphRefused, match="edge 0 has a Huber threshold"):
        _plan(g, -2.0)                                         # a scalar stands for every factor


def test_the_refusals_of_the_factors_form_come_first_and_in_their_words():
    g = small()
    m = len(g["kinds"])
    hub = np.full(m, np.nan)                                   # bad thresholds do not hide what is wrong with the graph

    def both(**change):
        a = {**dict(poses=g["poses"], kinds=g["kinds"], ij=g["ij"], data=g["data"], fixed=g["fixed"], sigmas=g["sigmas"]), **change}
        with pytest.raises(pose_graph.PoseGraphRefused) as old:
            pose_graph.plan_factors(a["poses"], a["kinds"], a["ij"], a["data"], fixed=a["fixed"], sigmas=a["sigmas"])
        with pytest.raises(pose_graph.PoseGraphRefused) as new:
            _plan(g, hub[:len(a["kinds"])], **change)
        assert str(new.value) == str(old.value) and new.value.status == old.value.status and str(old.value)
    k = g["kinds"].copy()
    k[1] = 3
    both(kinds=k)
    e = g["ij"].copy()
    e[3] = (4, 2)
    both(ij=e)
    e = g["ij"].copy()
    e[4] = (1, 1)
    both(ij=e)
    e = g["ij"].copy()
    e[0] = (0, 7)
    both(ij=e)
    d = g["data"].copy()
    d[5, 1] = np.nan
    both(data=d)
    d = g["data"].copy()
    d[0, 0] += 1e-3
    both(data=d)
    s = g["sigmas"].copy()
    s[4, 2] = 0.0
    both(sigmas=s)
    both(sigmas=None)
    p = g["poses"].copy()
    p[2, 0, 3] = np.inf
    both(poses=p)
    keep = [0, 1, 2, 4, 5]
    both(kinds=g["kinds"][keep], ij=g["ij"][keep], data=g["data"][keep], sigmas=g["sigmas"][keep])
    both(kinds=g["kinds"][:3], ij=g["ij"][:3], data=g["data"][:3], sigmas=g["sigmas"][:3], poses=g["poses"][:4], fixed=np.zeros(4, np.uint8))


def test_the_sizes_alone_decide_a_capacity_refusal():
    lib = _capi.load_library()
    why = ctypes.create_string_buffer(200)
    one = np.zeros(16)
    p = one.ctypes.data_as(_capi.c_double_p)
    f = np.zeros(1, np.uint8).ctypes.data_as(pose_graph.c_uint8_p)
    i = np.zeros(2, np.int32).ctypes.data_as(_capi.c_int32_p)
    for nodes, factors in ((pose_graph.MAX_NODES + 1, 1), (1, pose_graph.MAX_EDGES + 1)):      # nothing beyond the sizes is read
        assert lib.smhip_pose_graph_plan_robust(nodes, p, f, factors, None, i, p, None, p, None, None, why, len(why)) == CAPACITY
    assert lib.smhip_pose_graph_plan_robust(1, None, f, 0, None, None, None, None, None, None, None, why, len(why)) == INVALID


def test_the_report_needs_a_handle():
    lib = _capi.load_library()
    out = np.zeros(4)
    assert lib.smhip_pose_graph_last_robust(None, 4, out.ctypes.data_as(_capi.c_double_p), None, None) == INVALID
