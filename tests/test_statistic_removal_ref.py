"""The conditions on the StatisticRemoval fixtures that let the restatement (tests/statistic_removal_ref.py) alone settle the GPU
tests, and the filter's defaults and ConfigsValid() through the C ABI.  No GPU."""
import ctypes
import math

import numpy as np
import pytest
from scipy.spatial import cKDTree

import statistic_removal_cases as cases
import statistic_removal_ref as sr

F = np.float32


def kept_by_kdtree(rows, k, std_mul, brute):
    """An independent route to the kept set: the k + 1 nearest other rows from a float64 k-d tree, step 3's float d2 recomputed
    for them; where the k-th and (k + 1)-th float d2 tie or come out of order the brute-force distance is taken."""
    xyz = np.asarray(rows, dtype=F)[:, :3]
    idx = np.flatnonzero(sr.finite_rows(xyz))
    p = xyz[idx]
    _, nb = cKDTree(p.astype(np.float64)).query(p.astype(np.float64), k=k + 2)
    dist = np.zeros(len(xyz), F)
    fallbacks = 0
    for i in range(len(p)):
        others = [j for j in nb[i] if j != i][:k + 1]            # the query itself leaves; more than k + 2 copies of it: any one does
        d2 = sr.d2_float(p[i:i + 1], p[others])[0]               # in the tree's (float64) order
        if d2[:k].max() >= d2[k]:
            dist[idx[i]] = brute[idx[i]]
            fallbacks += 1
        else:
            dist[idx[i]] = sr.mean_of_sorted(np.sort(d2[:k])[None, :], k)[0]
    return sr.decide(rows, dist, std_mul)["keep"], fallbacks


@pytest.mark.parametrize("cloud", ["B", "D"])
def test_kept_set_equals_the_kdtree_route(cloud):
    rows = cases.CLOUDS[cloud]()
    ref = cases.reference(cloud, 30, 1.0)
    keep, fallbacks = kept_by_kdtree(rows, 30, 1.0, ref["distance"])
    assert np.array_equal(keep, ref["keep"])
    assert fallbacks < ref["V"]                                   # the route stands on its own for most rows
    assert 0 < int((~ref["keep"]).sum()) < len(rows)              # and the filter does something on this cloud


@pytest.mark.parametrize("cloud,k,std_mul", cases.GPU_CASES)
def test_threshold_does_not_depend_on_the_summation_order(cloud, k, std_mul):
    """(b): the restatement's order against math.fsum, and the cancellation factor that bounds every other order"""
    ref = cases.reference(cloud, k, std_mul)
    d = ref["distance"].astype(np.float64)[sr.finite_rows(cases.CLOUDS[cloud]())]
    v = ref["V"]
    s, sq = math.fsum(d), math.fsum(d * d)
    exact = sr.threshold_from_sums(s, sq, v, std_mul)
    assert abs(ref["threshold"] - exact) <= 1e-9 * abs(exact)
    variance = (sq - s * s / v) / (v - 1)
    assert sq / ((v - 1) * variance) <= 10.0


@pytest.mark.parametrize("cloud,k,std_mul", cases.GPU_CASES)
def test_no_distance_sits_on_the_threshold(cloud, k, std_mul):
    """(c): a float ulp is 6e-8; with no distance within 1e-6 relative of the threshold the kept set is the same under any
    summation order"""
    ref = cases.reference(cloud, k, std_mul)
    d = ref["distance"].astype(np.float64)[sr.finite_rows(cases.CLOUDS[cloud]())]
    assert np.abs(d - ref["threshold"]).min() > 1e-6 * abs(ref["threshold"])


def test_fixture_b_holds_what_it_promises():
    rows = cases.cloud_b()
    fin = sr.finite_rows(rows)
    assert len(rows) == 2503 and len(rows) % 64 != 0 and int((~fin).sum()) == 3
    d30 = cases.distances("B", 30)
    assert np.all(d30[~fin] == 0)
    assert int((d30[fin] == 0).sum()) == 40                       # the 40 copies: more than k + 1 zeros
    assert int((d30 > 5.0).sum()) >= 25                           # the isolated rows
    ref = cases.reference("B", 30, 1.0)
    assert ref["keep"][~fin].all() and ref["V"] == 2500


def test_pass_through_when_no_more_than_k_rows_are_finite():
    rows = cases.cloud_a(30)
    out = sr.statistic_removal(rows, 1.0, 30)
    assert out["passed_through"] and out["keep"].all() and out["V"] == 30


def test_restatement_chunking_does_not_change_the_answer():
    rows = cases.cloud_b()
    assert np.array_equal(sr.mean_distances(rows, 30, chunk=37), cases.distances("B", 30))


def test_defaults_and_config_valid_through_the_c_abi():
    """(d): needs the library, no GPU"""
    from staticmapping_amd import _capi, filters as df
    lib = _capi.load_library()
    d = _capi.FilterDescEx()
    lib.smhip_filter_default_ex(9, ctypes.byref(d))
    assert d.type == 9 == df.STATISTIC_REMOVAL and d.p[0] == 1.0 and d.i[0] == 30

    def valid(**kw):
        return df.config_valid(df.make_filter("StatisticRemoval", **kw))

    assert valid()
    assert not valid(point_num_meank=0) and not valid(point_num_meank=65)
    assert not valid(std_mul=math.nan) and not valid(std_mul=math.inf) and not valid(std_mul=-math.inf)
    assert valid(point_num_meank=1) and valid(point_num_meank=64) and valid(std_mul=0.0) and valid(std_mul=-0.5)
    for k, s in [(0, 1.0), (65, 1.0), (1, 1.0), (64, -0.5), (30, math.nan)]:
        assert sr.config_valid(s, k) == valid(point_num_meank=k, std_mul=s)
    with pytest.raises(KeyError):
        df.make_filter("StatisticRemoval", mean_k=3)


def test_chain_from_xml_takes_the_filter_only_when_asked():
    from staticmapping_amd import filters as df
    xml = ('<filters><filter name="Range"><param type="1" name="min_range"> 1. </param></filter>'
           '<filter name="StatisticRemoval"><param type="0" name="point_num_meank"> 12 </param>'
           '<param type="1" name="std_mul"> 2.5 </param></filter></filters>')
    assert [d.type for d in df.chain_from_xml(xml)] == [df.RANGE]
    assert [d.type for d in df.chain_from_xml(xml, ground_filters=True)] == [df.RANGE]
    chain = df.chain_from_xml(xml, statistic_removal=True)
    assert [d.type for d in chain] == [df.RANGE, df.STATISTIC_REMOVAL]
    assert chain[1].i[0] == 12 and chain[1].p[0] == 2.5
