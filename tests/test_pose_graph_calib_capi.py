"""smhip_pose_graph_plan_calib -- the host half of smhip_pose_graph_optimize_calib -- without a GPU, through ctypes
(staticmapping_amd.pose_graph.plan_calib): every refusal the HANDEYE factor adds, with its reason; the CSR lists; the plan of a graph
without a HANDEYE equal to plan_robust's; and the older entries, which keep refusing kind 3 in their words."""
import ctypes

import numpy as np
import pytest

import pose_graph_calib_cases as cases
import pose_graph_calib_ref as calib
from staticmapping_amd import _capi, pose_graph
from test_pose_graph_gps_capi import small

INVALID, CAPACITY = 1, 7


def _plan(g, entry=None, **change):
    a = {**dict(poses=g["poses"], kinds=g["kinds"], ij=g["ij"], data=g["data"], fixed=g["fixed"], sigmas=g["sigmas"], huber=g.get("huber")), **change}
    return (entry or pose_graph.plan_calib)(a["poses"], a["kinds"], a["ij"], a["data"], fixed=a["fixed"], sigmas=a["sigmas"], huber=a["huber"])


def test_the_symbols_and_the_kind_are_there():
    lib = _capi.load_library()
    for name in ("smhip_pose_graph_plan_calib", "smhip_pose_graph_optimize_calib"):
        assert name in _capi.SIGNATURES and getattr(lib, name) is not None
    assert pose_graph.HANDEYE == calib.HANDEYE == 3
    assert (pose_graph.factor_data(pose_graph.HANDEYE, cases.T_TRUE) == calib.handeye_data(cases.T_TRUE)).all()


@pytest.mark.parametrize("name", ["chain4_held", "chain4_free", "gps24_free"])
def test_the_csr_lists(name):
    g = cases.graph(name)
    off, inc = _plan(g)
    n, j = len(g["poses"]), g["calib_node"]
    prior = g["kinds"] == calib.PRIOR
    assert off[-1] == 2 * len(g["kinds"]) - prior.sum() == len(inc)
    for k in range(n):
        want = [e for e, (a, b) in enumerate(g["ij"]) if k in (a, b)]
        assert list(inc[off[k]:off[k + 1]]) == want
    he = np.flatnonzero(g["kinds"] == calib.HANDEYE)
    assert set(he) <= set(inc[off[j]:off[j + 1]]) and len(he) == len(g["truth"])      # the calibration node lists every HANDEYE


def test_without_a_handeye_the_plan_is_plan_robusts():
    g = small()
    m = len(g["kinds"])
    want = pose_graph.plan_robust(g["poses"], g["kinds"], g["ij"], g["data"], fixed=g["fixed"], sigmas=g["sigmas"], huber=np.ones(m))
    got = pose_graph.plan_calib(g["poses"], g["kinds"], g["ij"], g["data"], fixed=g["fixed"], sigmas=g["sigmas"], huber=np.ones(m))
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    hub = np.ones(m)
    hub[2] = -1.0
    with pytest.raises(pose_graph.PoseGraphRefused, match="edge 2 has a Huber threshold that is negative or not finite"):
        pose_graph.plan_calib(g["poses"], g["kinds"], g["ij"], g["data"], fixed=g["fixed"], sigmas=g["sigmas"], huber=hub)


def test_the_new_refusals_and_their_reasons():
    g = cases.graph("chain4_free")
    he = int(np.flatnonzero(g["kinds"] == calib.HANDEYE)[1])
    pr = int(np.flatnonzero(g["kinds"] == calib.PRIOR)[0])
    j = g["calib_node"]

    def refused(match, **change):
        with pytest.raises(pose_graph.PoseGraphRefused, match=match) as err:
            _plan(g, **change)
        assert err.value.status == INVALID and str(err.value).startswith("pose graph: ")
    keep = [k for k in range(len(g["kinds"])) if k != pr]                              # a free calibration node without its PRIOR
    refused("free node %d is the calibration node of a hand-eye factor and has no prior" % j,
            kinds=g["kinds"][keep], ij=g["ij"][keep], data=g["data"][keep], sigmas=g["sigmas"][keep], huber=g["huber"][keep])
    e = g["ij"].copy()
    e[he] = (1, 1)
    refused("edge %d is a hand-eye factor that joins a node to itself" % he, ij=e)
    e = g["ij"].copy()
    e[he] = (1, 9)
    refused("edge %d names a node out of range" % he, ij=e)
    for at, bad, why in ((0, 1e-3, "has a rotation block further than 1e-6 from orthonormal"), (13, np.nan, "is not finite"), (5, np.inf, "is not finite")):
        d = g["data"].copy()
        d[he, at] += bad
        refused("edge %d's odometer pose %s" % (he, why), data=d)
    d = g["data"].copy()
    d[he, :3] *= -1.0
    refused("edge %d's odometer pose has a reflection" % he, data=d)
    for c in range(6):                                                                 # all six sigmas are read
        for bad in (0.0, -1.0, np.nan, np.inf):
            s = g["sigmas"].copy()
            s[he, c] = bad
            refused("edge %d has a sigma that is not finite and positive" % he, sigmas=s)
    refused("is no BETWEEN and needs its sigmas", sigmas=None)
    k = g["kinds"].copy()
    k[he] = 4
    refused("edge %d has a kind that is none of BETWEEN, PRIOR, POINT and HANDEYE" % he, kinds=k)
    hub = g["huber"].copy()
    hub[he] = -0.5
    refused("edge %d has a Huber threshold that is negative or not finite" % he, huber=hub)


def test_a_handeye_counts_like_a_between_for_its_frame_node_and_connects():
    """two chain nodes without a BETWEEN: the HANDEYE alone holds each (Ad is invertible) and joins it to the calibration node, whose
    fixed flag or PRIOR then anchors the one component; without either nothing does"""
    T, Z = cases.T_TRUE, np.eye(4)
    poses = np.stack([np.eye(4), np.eye(4), T])
    kinds = np.array([calib.HANDEYE, calib.HANDEYE, calib.PRIOR], np.uint8)
    ij = np.array([(0, 2), (1, 2), (2, 2)], np.int32)
    data = np.stack([calib.handeye_data(Z), calib.handeye_data(Z), calib.handeye_data(T)])
    sig = np.stack([calib.ODOM_SIGMAS, calib.ODOM_SIGMAS, calib.CALIB_PRIOR_SIGMAS])
    off, inc = pose_graph.plan_calib(poses, kinds[:2], ij[:2], data[:2], fixed=[0, 0, 1], sigmas=sig[:2])
    assert list(off) == [0, 1, 2, 4] and list(inc) == [0, 1, 0, 1]
    off, inc = pose_graph.plan_calib(poses, kinds, ij, data, fixed=[0, 0, 0], sigmas=sig)
    assert list(off) == [0, 1, 2, 5] and list(inc) == [0, 1, 0, 1, 2]
    with pytest.raises(pose_graph.PoseGraphRefused, match="free node 2 is the calibration node of a hand-eye factor and has no prior"):
        pose_graph.plan_calib(poses, kinds[:2], ij[:2], data[:2], fixed=[1, 0, 0], sigmas=sig[:2])
    with pytest.raises(pose_graph.PoseGraphRefused, match="free node 1 has no edge"):
        pose_graph.plan_calib(poses, kinds[[0, 2]], ij[[0, 2]], data[[0, 2]], fixed=[0, 0, 0], sigmas=sig[[0, 2]])


def test_the_older_entries_keep_refusing_kind_3_in_their_words():
    g = cases.graph("chain4_held")
    for entry in (pose_graph.plan_robust, lambda *a, huber=None, **kw: pose_graph.plan_factors(*a, **kw)):
        with pytest.raises(pose_graph.PoseGraphRefused, match="has a kind that is none of BETWEEN, PRIOR and POINT$") as err:
            _plan(g, entry=entry)
        assert err.value.status == INVALID
    s = small()
    k = s["kinds"].copy()
    k[1] = 7
    with pytest.raises(pose_graph.PoseGraphRefused, match="edge 1 has a kind that is none of BETWEEN, PRIOR, POINT and HANDEYE"):
        pose_graph.plan_calib(s["poses"], k, s["ij"], s["data"], fixed=s["fixed"], sigmas=s["sigmas"])


def test_the_sizes_alone_decide_a_capacity_refusal():
    lib = _capi.load_library()
    why = ctypes.create_string_buffer(200)
    one = np.zeros(16)
    p = one.ctypes.data_as(_capi.c_double_p)
    f = np.zeros(1, np.uint8).ctypes.data_as(pose_graph.c_uint8_p)
    i = np.zeros(2, np.int32).ctypes.data_as(_capi.c_int32_p)
    for nodes, factors in ((pose_graph.MAX_NODES + 1, 1), (1, pose_graph.MAX_EDGES + 1)):
        assert lib.smhip_pose_graph_plan_calib(nodes, p, f, factors, None, i, p, None, p, None, None, why, len(why)) == CAPACITY
    assert lib.smhip_pose_graph_optimize_calib(None, 1, p, f, 0, None, None, None, None, None, None, None) == INVALID
