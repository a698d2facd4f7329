"""smhip_pose_graph_plan_factors -- the host half of smhip_pose_graph_optimize_factors -- without a GPU, through
staticmapping_amd.pose_graph.plan_factors: every refusal the PRIOR and POINT kinds add, each with its reason, the CSR order with a
PRIOR listed once, and kinds == NULL giving the plan of smhip_pose_graph_plan.  (non_chain_edges and pcg_cap are not part of the
ABI's plan call: tests/cpp/test_pose_graph_gps.cc checks them on the Plan itself.)"""
import numpy as np
import pytest

import pose_graph_cases as base
import pose_graph_gps_ref as gps
import pose_graph_ref as ref
from staticmapping_amd import pose_graph

INVALID = 1


def small():
    """a chain 0 - 1 - 2 - 3 (node 0 fixed), the frame node 4 with a PRIOR, POINT factors on nodes 1 and 3"""
    d = base.chain_graph(4, 5)
    enu = np.array([[1.0, 2.0, 3.0]] * 4)
    return gps.with_gps(d, enu, np.array([0.3, -0.2, 1.1]), np.eye(4), [1, 3])


def _plan(g, **change):
    a = {**dict(poses=g["poses"], kinds=g["kinds"], ij=g["ij"], data=g["data"], fixed=g["fixed"], sigmas=g["sigmas"]), **change}
    return pose_graph.plan_factors(a["poses"], a["kinds"], a["ij"], a["data"], fixed=a["fixed"], sigmas=a["sigmas"])


def test_factor_kinds_match_the_header_and_the_restatement():
    assert (pose_graph.BETWEEN, pose_graph.PRIOR, pose_graph.POINT) == (gps.BETWEEN, gps.PRIOR, gps.POINT) == (0, 1, 2)
    Z = ref.make_pose((0.1, 0.2, 0.3), (1, 2, 3))
    assert (pose_graph.factor_data(pose_graph.BETWEEN, Z) == gps.between_data(Z)).all()
    assert (pose_graph.factor_data(pose_graph.POINT, [1, 2, 3], [4, 5, 6]) == gps.point_data([1, 2, 3], [4, 5, 6])).all()


def test_csr_order_with_a_prior_listed_once():
    g = small()
    # factors: 0 (0,1)  1 (1,2)  2 (2,3)  3 PRIOR (4,4)  4 POINT (4,1)  5 POINT (4,3)
    assert [tuple(x) for x in g["ij"]] == [(0, 1), (1, 2), (2, 3), (4, 4), (4, 1), (4, 3)]
    off, inc = _plan(g)
    assert list(off) == [0, 1, 4, 6, 8, 11]
    assert list(inc) == [0, 0, 1, 4, 1, 2, 2, 5, 3, 4, 5]
    for k in range(5):
        assert list(inc[off[k]:off[k + 1]]) == [e for e, (i, j) in enumerate(g["ij"]) if k in (i, j)]


def test_null_kinds_give_the_old_plan():
    d = base.stage_cases()["reversed_and_double"]
    data = np.stack([gps.between_data(Z) for Z in d["Z"]])
    old = pose_graph.plan(d["poses"], d["edges"], d["Z"], fixed=d["fixed"])
    for sig in (None, ref.DEFAULT_SIGMAS):
        new = pose_graph.plan_factors(d["poses"], None, d["edges"], data, fixed=d["fixed"], sigmas=sig)
        assert (old[0] == new[0]).all() and (old[1] == new[1]).all()
    zeros = pose_graph.plan_factors(d["poses"], np.zeros(len(data), np.uint8), d["edges"], data, fixed=d["fixed"])
    assert (old[1] == zeros[1]).all()
    with pytest.raises(pose_graph.PoseGraphRefused, match="no fixed node"):          # the old refusals, in the old words
        pose_graph.plan_factors(d["poses"], None, d["edges"], data, fixed=np.zeros(len(d["poses"]), np.uint8))


def test_every_new_refusal_has_its_reason():
    g = small()

    def refused(word, **change):
        with pytest.raises(pose_graph.PoseGraphRefused, match=word) as err:
            _plan(g, **change)
        assert err.value.status == INVALID
    _plan(g)
    k = g["kinds"].copy()
    k[1] = 3
    refused("edge 1 has a kind", kinds=k)
    e = g["ij"].copy()
    e[3] = (4, 2)
    refused("edge 3 is a prior whose j is not its i", ij=e)
    d = g["data"].copy()
    d[3, 0] += 1e-5
    refused("edge 3's prior pose .*orthonormal", data=d)
    d = g["data"].copy()
    d[3, 13] = np.inf
    refused("edge 3's prior pose is not finite", data=d)
    e = g["ij"].copy()
    e[4] = (1, 1)
    refused("edge 4 is a point factor that joins a node to itself", ij=e)
    for c in (1, 4):                                   # the lever arm, the point
        d = g["data"].copy()
        d[5, c] = np.nan
        refused("edge 5 has a lever arm or a point that is not finite", data=d)
    d = g["data"].copy()
    d[5, 6:] = np.nan                                  # the rest of a POINT's data is not read
    _plan(g, data=d)
    for bad in (0.0, -1.0, np.nan, np.inf):
        s = g["sigmas"].copy()
        s[4, 2] = bad
        refused("edge 4 has a sigma", sigmas=s)
        s = g["sigmas"].copy()
        s[3, 5] = bad
        refused("edge 3 has a sigma", sigmas=s)
        s = g["sigmas"].copy()
        s[4, 3:] = bad                                 # sigmas[3..5] of a POINT are not read
        _plan(g, sigmas=s)
    refused("edge 3 is no BETWEEN and needs its sigmas", sigmas=None)
    # a free node with POINT factors only: the frame node without its PRIOR
    keep = [0, 1, 2, 4, 5]
    refused("free node 4 has point factors only", kinds=g["kinds"][keep], ij=g["ij"][keep], data=g["data"][keep], sigmas=g["sigmas"][keep])
    # ... and an observed node without its chain edges
    lone = gps.make_graph(list(g["poses"]), [1, 0, 0, 0, 0], [tuple([g["kinds"][f], *g["ij"][f], g["data"][f], g["sigmas"][f]]) for f in (0, 1, 3, 4, 5)])
    with pytest.raises(pose_graph.PoseGraphRefused, match="free node 3 has point factors only"):
        _plan(lone)
    # a component with neither a fixed node nor a PRIOR: nothing fixed, the frame's PRIOR holds all of it through the POINT factors
    _plan(g, fixed=np.zeros(5, np.uint8))
    free = gps.make_graph(list(g["poses"][:4]), [0, 0, 0, 0], [tuple([g["kinds"][f], *g["ij"][f], g["data"][f], g["sigmas"][f]]) for f in (0, 1, 2)])
    with pytest.raises(pose_graph.PoseGraphRefused, match="no fixed node and no prior"):
        _plan(free)
    # a PRIOR does not connect: two chains, one with the fixed node, the other with nothing
    two = gps.make_graph(list(g["poses"]), [1, 0, 0, 0, 0],
                         [(gps.BETWEEN, 0, 1, g["data"][0], ref.DEFAULT_SIGMAS), (gps.BETWEEN, 3, 4, g["data"][0], ref.DEFAULT_SIGMAS),
                          (gps.BETWEEN, 2, 3, g["data"][0], ref.DEFAULT_SIGMAS)])
    with pytest.raises(pose_graph.PoseGraphRefused, match="the component of node 2 has no fixed node and no prior"):
        _plan(two)
    two["kinds"] = np.append(two["kinds"], gps.PRIOR).astype(np.uint8)
    two["ij"] = np.vstack([two["ij"], [[3, 3]]]).astype(np.int32)
    two["data"] = np.vstack([two["data"], gps.prior_data(np.eye(4))[None]])
    two["sigmas"] = np.vstack([two["sigmas"], np.full((1, 6), 0.1)])
    _plan(two)
