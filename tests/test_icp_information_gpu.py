"""smhip_icp_information_at / _range on the device against tests/icp_information_ref.py, on the pairs of
tests/icp_information_cases.py.  The restatement starts from the device's own f32 values -- the centred target, its normals and
the mean (smhip_icp_debug_get_grid), the matches and distances (smhip_icp_get_matches) -- so what separates the two sides is the
order of the f64 sums and the fused multiply-adds: n * 2^-53 ~ 2e-13 of the sum of magnitudes.  The bound asked of every entry,
1e-9 of sqrt(H_aa H_bb), leaves three orders for the gathers' order."""
import numpy as np
import pytest

import icp_information_cases as cases
import icp_information_ref as info

pytestmark = pytest.mark.gpu

H_TOL = 1e-9
NAMES = list(cases.REGULAR) + ["plane_far", "all_nan"]


@pytest.fixture(scope="module")
def smhip():
    import staticmapping_amd as sm
    from staticmapping_amd import _capi
    lib = _capi.load_library()
    assert lib.smhip_device_count() >= 1, "no gfx950 device visible"
    return sm


@pytest.fixture(scope="module")
def run(smhip):
    """One matcher, a slot per case; every case's single call with what the device matched for it, read right after the call."""
    all_cases = cases.cases()
    m = smhip.IcpFastHip(pair_slots=len(NAMES), max_source_points=2048, max_target_points=2048)
    got, seen = {}, {}
    for slot, name in enumerate(NAMES):
        c = all_cases[name]
        m.set_input_source(c["src"], slot=slot)
        m.set_input_target(c["tgt"], c["nrm"], slot=slot)
    for slot, name in enumerate(NAMES):
        c = all_cases[name]
        try:
            got[name] = m.information(c["T"], cases.RATIO, slot=slot)
        except smhip.SmhipError as e:
            got[name] = dict(m.last_information[0], error=e.status)
        g = m.debug_get_grid(slot)
        order = g["tq"][:, 3].copy().view(np.int32)
        tq, tn = np.zeros((g["nt"], 3)), np.zeros((g["nt"], 3))
        tq[order], tn[order] = g["tq"][:, :3], g["tn"][:, :3]
        ids, d2 = m.get_matches(len(c["src"]), slot)
        seen[name] = dict(mu=g["mu"].copy(), tq=tq, tn=tn, ids=ids.astype(np.int64), d2=d2.astype(np.float64))
    yield dict(m=m, got=got, seen=seen, slot={n: k for k, n in enumerate(NAMES)})
    m.close()


def _restated(name, seen):
    c = cases.cases()[name]
    Tc = c["T"].copy()
    Tc[:3, 3] -= seen["mu"]                                   # the device matches in the target's centred frame
    return info.information(c["src"][:, :3].astype(np.float64), seen["tq"], seen["tn"], Tc, cases.RATIO, ids=seen["ids"], d2=seen["d2"])


@pytest.mark.parametrize("name", cases.REGULAR)
def test_information_matches_the_restatement(run, name):
    c, got, seen = cases.cases()[name], run["got"][name], run["seen"][name]
    assert got["status"] == 0 and "error" not in got
    want = _restated(name, seen)
    # the fixture's property first, on the device's own values: no kept query has a runner-up within 1e-4 of its match
    margin, ids, _ = cases.near_tie_margin(cases.moved_f32(c["src"], c["T"], seen["mu"]), seen["tq"], keep=np.isin(np.arange(len(c["src"])), want["rows"]))
    assert margin > 1e-4, margin
    assert np.array_equal(ids[want["rows"]], seen["ids"][want["rows"]])
    assert (got["kept"], got["n_finite"]) == (want["kept"], want["n_finite"])
    assert got["n_finite"] == int(np.isfinite(c["src"][:, :3]).all(axis=1).sum())        # every match exact: every finite row has one
    assert got["limit_d2"] == want["limit_d2"]
    H, Hr = got["H"], want["H"]
    assert np.array_equal(H, H.T)
    scale = np.sqrt(np.outer(np.diag(Hr), np.diag(Hr)))
    worst = float((np.abs(H - Hr) / scale).max())
    rel_r2 = abs(got["sum_r2"] - want["sum_r2"]) / want["sum_r2"]
    print(f"{name}: kept {got['kept']} of {got['n_finite']}, worst |H - ref| / sqrt(H_aa H_bb) = {worst:.3e}, |sum_r2 - ref| / ref = {rel_r2:.3e}")
    assert worst <= H_TOL and rel_r2 <= H_TOL


def test_a_pair_beyond_every_search_and_one_without_a_finite_row(run):
    """plane_far: hundreds of metres from the target, past the ball and the rings -- the exact pass still finds every nearest point
    (the sweep over the whole target), so it is an ordinary pair; all_nan: no finite correspondence, its status in the row, H zero"""
    far, seen = run["got"]["plane_far"], run["seen"]["plane_far"]
    assert far["status"] == 0 and "error" not in far
    want = _restated("plane_far", seen)
    assert (far["kept"], far["n_finite"], far["limit_d2"]) == (want["kept"], 300, want["limit_d2"])
    # (at 400 m the runner-up is within f32 rounding of the match, so the ids are not pinned: the distances are)
    c = cases.cases()["plane_far"]
    d2 = info.brute_matches(cases.moved_f32(c["src"], c["T"], seen["mu"]), seen["tq"])[1]
    assert np.all(np.abs(seen["d2"] - d2) <= 1e-6 * d2) and d2.min() > 300.0 ** 2
    scale = np.sqrt(np.outer(np.diag(want["H"]), np.diag(want["H"])))
    assert (np.abs(far["H"] - want["H"]) / scale).max() <= H_TOL
    none = run["got"]["all_nan"]
    assert none["status"] == 6 and none.get("error") == 6                  # SMHIP_ERR_NO_MATCH, in the row and returned
    assert np.all(none["H"] == 0.0) and none["sum_r2"] == 0.0 and none["kept"] == 0 and none["n_finite"] == 0


def test_two_calls_and_the_range_call_give_the_same_bits(run):
    m, slot = run["m"], run["slot"]
    all_cases = cases.cases()
    for name in cases.REGULAR:
        again = m.information(all_cases[name]["T"], cases.RATIO, slot=slot[name])
        for key in ("H", "sum_r2", "limit_d2", "kept", "n_finite", "status"):
            assert np.array_equal(again[key], run["got"][name][key]), (name, key)
    rows = m.information_range(0, [all_cases[n]["T"] for n in cases.REGULAR], cases.RATIO)
    assert len(rows) == 5
    for name, row in zip(cases.REGULAR, rows):
        for key in ("H", "sum_r2", "limit_d2", "kept", "n_finite", "status"):
            assert np.array_equal(row[key], run["got"][name][key]), (name, key)
    # a failing pair inside a range: its own row says so, its neighbours' rows are untouched
    with pytest.raises(Exception):
        m.information_range(4, [all_cases[n]["T"] for n in NAMES[4:]], cases.RATIO)
    rows = m.last_information
    assert [r["status"] for r in rows] == [0, 0, 6] and np.all(rows[2]["H"] == 0.0)
    assert np.array_equal(rows[0]["H"], run["got"]["corridor_2000_nan_row"]["H"])


def test_the_launch_form_of_the_matching_pass_does_not_matter(run):
    m, slot = run["m"], run["slot"]
    all_cases = cases.cases()
    m.set_options(no_single_kernel=1)
    try:
        for name in ("three_planes_2000", "corridor_1999"):
            other = m.information(all_cases[name]["T"], cases.RATIO, slot=slot[name])
            assert np.array_equal(other["H"], run["got"][name]["H"]) and other["sum_r2"] == run["got"][name]["sum_r2"]
            assert (other["kept"], other["limit_d2"]) == (run["got"][name]["kept"], run["got"][name]["limit_d2"])
    finally:
        m.set_options(no_single_kernel=0)


def test_the_callers_options_survive_and_the_refusals(smhip):
    c = cases.cases()["three_planes_2000"]
    m = smhip.IcpFastHip(pair_slots=2, max_source_points=2048, max_target_points=2048, max_iteration=3, early_exit=0, dist_outlier_ratio=0.5)
    m.set_input_source(c["src"])
    m.set_input_target(c["tgt"], c["nrm"])
    res1, score1, stats1 = m.align_batch(1)
    got = m.information(c["T"], 0.7)
    res2, score2, stats2 = m.align_batch(1)
    assert stats1[0]["iterations"] == 3 and stats1 == stats2 and np.array_equal(res1, res2) and np.array_equal(score1, score2)
    assert got["kept"] > stats1[0]["kept"]                                  # 0.7 of the matches there, 0.5 here

    def refused(status, word, call):
        with pytest.raises(smhip.SmhipError, match=word) as err:
            call()
        assert err.value.status == status
    refused(1, "slot out of range", lambda: m.information(c["T"], 0.7, slot=2))
    refused(1, "slot out of range", lambda: m.information_range(1, [c["T"], c["T"]], 0.7))
    refused(1, r"\[0, 1\]", lambda: m.information(c["T"], 1.5))
    refused(1, r"\[0, 1\]", lambda: m.information(c["T"], float("nan")))
    refused(4, "before SetInputSource", lambda: m.information(c["T"], 0.7, slot=1))
    from staticmapping_amd import _capi
    T = np.ascontiguousarray(c["T"].T).reshape(-1)
    assert m._lib.smhip_icp_information_at(m._h, 0, T.ctypes.data_as(_capi.c_double_p), 0.7, None) == 1
    assert m._lib.smhip_icp_information_at(m._h, 0, None, 0.7, (_capi.IcpInformation * 1)()) == 1
    assert b"NULL" in m._lib.smhip_last_error(m._h)
    m.set_input_source(c["src"], slot=1)
    m.set_input_target(c["tgt"], None, slot=1)
    refused(5, "no normals", lambda: m.information(c["T"], 0.7, slot=1))
    m.close()
