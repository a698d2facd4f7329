"""Device StatisticRemoval (smhip_filter_chain_ex_f32, id 9) against the restatement (tests/statistic_removal_ref.py): distance[]
and the statistics through the parity hook, the output rows and source_index, all bit for bit.  The clouds and what they
guarantee: tests/statistic_removal_cases.py and tests/test_statistic_removal_ref.py."""
import ctypes

import numpy as np
import pytest

import statistic_removal_cases as cases
import staticmapping_amd as sm
from staticmapping_amd import _capi, filters as df
from oracle import filters as of

pytestmark = pytest.mark.gpu
F = np.float32
INVALID_ARGUMENT, NOT_READY = 1, 4                                   # smhip_status, include/smhip.h


@pytest.fixture(scope="module")
def matcher():
    m = sm.IcpFastHip(pair_slots=1, max_source_points=16384, max_target_points=16384)
    yield m
    m.close()


def rows5(rows):
    return rows if rows.shape[1] == 5 else of.with_factor(rows)


def check(matcher, rows, k, std_mul, ref):
    """one StatisticRemoval on `rows`: everything the device reports equals `ref`"""
    got, gsrc = df.run_chain(matcher, rows, [df.make_filter("StatisticRemoval", point_num_meank=k, std_mul=std_mul)])
    dist, stats = df.statistic_last(matcher, len(rows))
    assert np.array_equal(dist.view(np.uint32), ref["distance"].view(np.uint32))
    assert stats["V"] == ref["V"]
    for name in ("sum", "sq_sum", "threshold"):
        assert np.float64(stats[name]).tobytes() == np.float64(ref[name]).tobytes(), (name, stats[name], ref[name])
    keep = ref["keep"]
    assert np.array_equal(gsrc, np.flatnonzero(keep).astype(np.int32))
    assert np.array_equal(got.view(np.uint32), rows5(rows)[keep].view(np.uint32))
    return got, gsrc


def test_a_every_set_is_everyone(matcher):
    check(matcher, cases.cloud_a(31), 30, 1.0, cases.reference("A31", 30, 1.0))


@pytest.mark.parametrize("extra_bad", [0, 3], ids=["30_rows", "30_finite_of_33"])
def test_a_pass_through_leaves_a_warning(matcher, extra_bad):
    rows = cases.cloud_a(30)
    if extra_bad:
        bad = np.ones((3, 5), F)
        bad[0, 0], bad[1, 1], bad[2, 2] = np.nan, np.inf, -np.inf
        rows = np.ascontiguousarray(np.concatenate([rows[:10], bad, rows[10:]]))
    got, gsrc = df.run_chain(matcher, rows, [df.make_filter("StatisticRemoval", point_num_meank=30)])
    assert np.array_equal(got.view(np.uint32), rows.view(np.uint32))
    assert np.array_equal(gsrc, np.arange(len(rows), dtype=np.int32))
    n_out = ctypes.c_int()
    df._launch(matcher, rows, [df.make_filter("StatisticRemoval", point_num_meank=30)], n_out)
    assert n_out.value == len(rows)
    msg = matcher._lib.smhip_last_error(matcher._h).decode()
    assert msg.startswith("warning") and "StatisticRemoval" in msg and "30 finite" in msg
    assert matcher._lib.smhip_filter_statistic_last(matcher._h, None, len(rows), None) == NOT_READY   # no distances were computed


@pytest.mark.parametrize("k", [30, 1, 64])
@pytest.mark.parametrize("std_mul", [1.0, 0.0, 2.5])
def test_b_c_adversarial_cloud_and_parameter_sweep(matcher, k, std_mul):
    rows = cases.cloud_b()
    ref = cases.reference("B", k, std_mul)
    got, gsrc = check(matcher, rows, k, std_mul, ref)
    bad = np.flatnonzero(~np.isfinite(rows[:, :3]).all(axis=1))
    assert set(bad) <= set(gsrc) and ref["V"] == len(rows) - 3      # non-finite rows: kept, and absent from V
    assert 0 < len(got) < len(rows)


def test_d_realistic_density_profile(matcher):
    rows = cases.cloud_d()
    assert rows.shape == (12000, 4)
    got, _ = check(matcher, rows, 30, 1.0, cases.reference("D", 30, 1.0))
    assert 0 < len(got) < len(rows)


def test_e_in_a_chain(matcher):
    raw = cases.cloud_d()
    chain = [df.make_filter("Range", min_range=1.0, max_range=60.0), df.make_filter("StatisticRemoval"),
             df.make_filter("RandomSampler", sampling_rate=0.5, seed=cases.SAMPLER_E["seed"])]
    got, gsrc = df.run_chain(matcher, raw, chain)
    ranged, rsrc = cases.cloud_e_ranged()
    ref = cases.reference("E_ranged", 30, 1.0)
    want, wsrc = of.run_chain(ranged[ref["keep"]], [cases.SAMPLER_E])
    wsrc = rsrc[ref["keep"]][wsrc]                                   # composed through all three filters
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(gsrc, wsrc)
    dist, stats = df.statistic_last(matcher, len(ranged))           # the hook reports in that filter's input row order
    assert np.array_equal(dist.view(np.uint32), ref["distance"].view(np.uint32)) and stats["threshold"] == ref["threshold"]
    df.output_to_source(matcher, 0)
    ns = ctypes.c_int()
    matcher._check(matcher._lib.smhip_get_cloud_sizes(matcher._h, 0, ctypes.byref(ns), None, None))
    assert ns.value == len(got) > 0
    # the narrow entry point refuses the extended id
    d = _capi.FilterDesc()
    d.type = df.STATISTIC_REMOVAL
    n_out = ctypes.c_int()
    a = np.ascontiguousarray(raw)
    st = matcher._lib.smhip_filter_chain_f32(matcher._h, a.ctypes.data_as(_capi.c_float_p), 4, len(a), ctypes.byref(d), 1, ctypes.byref(n_out))
    assert st == INVALID_ARGUMENT


def test_f_determinism_and_table_growth():
    m = sm.IcpFastHip(pair_slots=1, max_source_points=16384, max_target_points=16384)    # a fresh handle: the tables grow here
    try:
        f = [df.make_filter("StatisticRemoval")]
        first = df.run_chain(m, cases.cloud_b(), f)
        d_first = df.statistic_last(m, 2503)[0]
        check(m, cases.cloud_d(), 30, 1.0, cases.reference("D", 30, 1.0))
        again = df.run_chain(m, cases.cloud_b(), f)
        d_again = df.statistic_last(m, 2503)[0]
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
        assert d_first.tobytes() == d_again.tobytes()
    finally:
        m.close()


def test_g_translated_cloud_is_still_exact(matcher):
    """no coordinate range: the search walks the cloud sorted along one axis, so nothing is refused; far from the origin the
    float d2 values are coarser and tie more often, and the answer must still be the restatement's"""
    check(matcher, cases.cloud_b_translated(), 30, 1.0, cases.reference("B_translated", 30, 1.0))


def test_hook_says_not_ready_without_the_filter(matcher):
    df.run_chain(matcher, cases.cloud_a(31), [df.make_filter("Range")])
    with pytest.raises(sm.matcher.SmhipError) as e:
        df.statistic_last(matcher, 31)
    assert e.value.status == NOT_READY
    df.run_chain(matcher, cases.cloud_a(31), [df.make_filter("StatisticRemoval", point_num_meank=5)])
    with pytest.raises(sm.matcher.SmhipError) as e:
        df.statistic_last(matcher, 30)                               # the wrong row count
    assert e.value.status == INVALID_ARGUMENT
    assert len(df.statistic_last(matcher, 31)[0]) == 31
