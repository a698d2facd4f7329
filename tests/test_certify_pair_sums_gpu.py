"""The fused certificate pass (nn_certify_acc) holds its 27 sums in 14 slots per lane, shared by the lanes 2k and 2k+1 of a wave:
each lane adds its slots for both lanes' points, the partner's seven values (J, r) arrive by a DPP swap, and a lane whose own point
is not kept sends exact zeros (accumulate_terms_pair, block_reduce_pair_sums in csrc/icp_kernels.hip).  What can go wrong there shows
at the edges of pairs, waves and blocks and where only one lane of a pair is kept -- so: batches of 16 pairs (the smallest that take
the fused path), 12 fixed iterations, switch after 2, sources cut to sizes at the edge of a wave, of a round of 256 and of the
256 x 32-point block of a workgroup, against the same batch with the sums kept apart from the certificate pass (no_fused_sums = 1, `accumulate`): the same kept
count and quantile in the last iteration (integers / an order statistic: identical), poses within the project's tolerance for a
re-ordered f64 sum (1e-11 rad / 1e-10 m, tests/test_icp_gpu.py::test_fused_certificate_pass_sums_equal_the_separate_passes), two runs
bit-identical, 16 slots of identical input bit-identical, and every pair with at least one iteration whose sums came from the fused
pass (it is not the fallback that is compared).  The same sizes in the reference-search mode (nn_certify_acc<., true>).

Sizes.  A batch of 16 pairs takes the small-launch kernels -- no certificate pass at all -- while its search launch has fewer than
512 workgroups of 512 queries (icp_plan.h: Part::small), that is up to 15 872 points per pair: on the commit before the lane pairs
63, 64, 65, 255, 256, 257, 8191, 8192 and 8193 points all report fused_iterations = 0 (15 872 too; 15 873 reports 10).  Each is
replaced by the next larger size of its kind that carries fused iterations: 63 / 64 / 65 -> 15935 / 15936 / 15937 (249 waves: an
odd tail, a full wave, a half-filled pair), 255 / 256 / 257 -> 16127 / 16128 / 16129 (63 rounds of 256), 8191 / 8192 / 8193 ->
16383 / 16384 / 16385 (two blocks of 8192), and the fixture's full 20 000.

The device orders an uploaded source along a Morton curve (prep_normals.hip: morton_keys, 6.25 cm quantum from the cloud's finite
minimum), so a lane's partner is its neighbour on that curve, not in the caller's array: `_device_order` restates the keys on the
host, and the constructed inputs below are described in THAT order."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 16
ITER = 12
SIZES = [15935, 15936, 15937, 16127, 16128, 16129, 16383, 16384, 16385, None]          # None: the fixture's full size
_cache = {}


@pytest.fixture(scope="module")
def smhip():
    import staticmapping_amd as sm
    from staticmapping_amd import _capi
    lib = _capi.load_library()
    assert lib.smhip_device_count() >= 1, "no gfx950 device visible"
    return sm


def _guess(case):
    from staticmapping_amd import synth
    return case["T"] @ synth.make_pose(t=(0.02, -0.01, 0.01), rpy_deg=(0.05, -0.03, 0.1))


def _device_order(src):
    """The order the device gives an uploaded cloud: ascending Morton key of the coordinates quantised to 1/16 m from the finite
    minimum (non-finite coordinate: 0), ties in the caller's order."""
    p = np.asarray(src, dtype=np.float32)[:, :3]
    fin = np.isfinite(p)
    mn = np.where(fin, p, np.inf).min(axis=0).astype(np.float32)
    t = (p - mn) * np.float32(16.0)
    q = np.where(np.isfinite(t), np.clip(t, 0.0, 2097151.0), 0.0).astype(np.uint64)
    key = np.zeros(len(p), dtype=np.uint64)
    for bit in range(21):
        for c in range(3):
            key |= ((q[:, c] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + c)
    return np.argsort(key, kind="stable")


def _run(sm, src, case, guess, **opts):
    """Two batches of 16 slots of the same input and guess on one handle: (poses, scores, stats) of the second, after asserting that
    the two are the same bits and that the 16 slots are.  (The reference-search mode takes a batch's first fused iteration from the
    searched shares of the batch before, and the order of the sums follows it: both batches start from a forgotten history, as a
    handle's first batch does, so that runs that switch at the same place are compared.)"""
    m = sm.IcpFastHip(pair_slots=B, max_source_points=len(src), max_target_points=len(case["q"]), max_iteration=ITER, early_exit=0,
                      split_after=2, **opts)
    m.set_input_source(src); m.set_input_target(case["q"], case["n"])
    for s in range(1, B):
        m.copy_slot(0, s)
    runs = []
    for _ in range(2):
        m.forget_search_history()
        runs.append(m.align_batch(B, [guess] * B))
    m.close()
    (R0, sc0, st0), (R1, sc1, st1) = runs
    R0, R1 = np.asarray(R0), np.asarray(R1)
    assert R0.tobytes() == R1.tobytes() and np.asarray(sc0).tobytes() == np.asarray(sc1).tobytes(), "two runs differ"
    assert all(R1[s].tobytes() == R1[0].tobytes() for s in range(B)), "slots of identical input differ"
    assert [s["kept"] for s in st0] == [s["kept"] for s in st1]
    return R1, sc1, st1


def _compare(sm, src, case, key, **opts):
    """fused against separate on the same batch; the separate result of a (cloud, mode) is computed once."""
    guess = _guess(case)
    if key not in _cache:
        _cache[key] = _run(sm, src, case, guess, no_fused_sums=1, **opts)
    Rs, scs, sts = _cache[key]
    Rf, scf, stf = _run(sm, src, case, guess, **opts)
    assert all(s["fused_iterations"] == 0 for s in sts)
    fused = [s["fused_iterations"] for s in stf]
    print(f"{key}: fused_iterations {min(fused)}..{max(fused)} kept {stf[0]['kept']} (separate {sts[0]['kept']})")
    worst = (0.0, 0.0)
    for s in range(B):
        da, dt = sm.se3_error(Rf[s], Rs[s])
        worst = (max(worst[0], da), max(worst[1], dt))
    print(f"{key}: fused vs separate worst {worst[0]:.3e} rad / {worst[1]:.3e} m")
    assert min(fused) >= 1, fused
    for s in range(B):
        assert stf[s]["iterations"] == ITER and sts[s]["iterations"] == ITER
        assert stf[s]["kept"] == sts[s]["kept"] and stf[s]["limit_d2"] == sts[s]["limit_d2"], (s, stf[s], sts[s])
    assert np.isfinite(np.asarray(Rf)).all()
    assert worst[0] < 1e-11 and worst[1] < 1e-10, worst
    return stf, sts


@pytest.mark.parametrize("ns", SIZES)
def test_pair_sums_at_pair_wave_and_block_edges(smhip, velo20k, ns):
    """Sizes at the edge of a wave (an odd tail, a half-filled pair), of a workgroup's round, of its block of 256 x 32 points (see the
    module's note on the sizes) and the fixture's full size (20 000; the 120 000-point pair has its own test below)."""
    case = velo20k
    src = np.ascontiguousarray(case["src"][:ns] if ns else case["src"])
    _compare(smhip, src, case, ("grid", ns))


@pytest.mark.parametrize("ns", SIZES)
def test_pair_sums_in_the_reference_search_mode(smhip, velo20k, ns):
    """The same sizes through nn_certify_acc<., true> (nn_mode NABO): the template shares accumulate_terms_pair.

    Two runs of this mode used to differ in the last bit of a pose at most of the cut sizes (6 to 8 of the 10, another subset each
    run, before the lane pairs as well): the queries to walk again are appended to four class lists by atomics (nabo_list_append) and
    accumulate_listed summed them in list order, which follows the waves' timing.  It now sums a wave's share of the query INDICES in
    ascending index, wherever the queries stand in the lists; the assertion holds (three runs of this file: all 10 sizes)."""
    case = velo20k
    src = np.ascontiguousarray(case["src"][:ns] if ns else case["src"])
    _compare(smhip, src, case, ("nabo", ns), nn_mode=smhip.NN_NABO)


def test_pair_sums_at_full_size_120k(smhip, cfg2):
    """The headline's cloud size: 15 blocks per pair."""
    _compare(smhip, np.ascontiguousarray(cfg2["src"]), cfg2, ("grid", "cfg2"))


@pytest.mark.parametrize("parity", [1, 0])
def test_one_lane_of_a_pair_kept(smhip, velo20k, parity):
    """Every second point of a tenth of the cloud's device order (the odd ones; the mirror case: the even ones) displaced by +5 m in
    z: nothing lies within reach of a displaced point, so it is never kept, and its partner's terms must pass through the pair
    untouched.  (A tenth, not the whole cloud: with more than about a tenth of the points out of reach the trimming quantile meets
    their lower bounds, every iteration refines them and none takes its sums from the fused pass -- 12 % displaced reports
    fused_iterations = 0 on the commit before the lane pairs, 6 % reports 10.  And the displaced points take new places on the Morton
    curve: the restated order of the cloud as uploaded must still hold pairs with exactly one displaced lane, of both parities --
    asserted.  The 30 % of the matches above the quantile put one-lane pairs into every other case too.)"""
    src = np.array(velo20k["src"], dtype=np.float32, copy=True)
    order = _device_order(src)
    moved = order[4000 + parity:6000:2]
    src[moved, 2] += 5.0
    is_moved = np.zeros(len(src), dtype=bool); is_moved[moved] = True
    lanes = is_moved[_device_order(src)]
    pairs = lanes[: len(lanes) // 2 * 2].reshape(-1, 2)
    assert (pairs[:, 0] & ~pairs[:, 1]).sum() >= 1 and (~pairs[:, 0] & pairs[:, 1]).sum() >= 1
    stf, sts = _compare(smhip, src, velo20k, ("grid", "displaced", parity))
    assert 0 < stf[0]["kept"] <= len(src) - len(moved)


def test_nan_point_does_not_reach_its_partner(smhip, velo20k):
    """One NaN source point on an even lane and one on an odd lane (of the restated device order): each contributes exact zeros by
    select, its partner's terms survive -- the same kept count, quantile and poses as the separate passes, which never see the
    point (a non-finite query has no match), and finite poses."""
    src = np.array(velo20k["src"], dtype=np.float32, copy=True)
    order = _device_order(src)
    # the NaN coordinate moves a point on the curve: try candidates until the uploaded cloud has one NaN on each lane parity
    for a in range(200, 400):
        for b_ in range(9000, 9100):
            trial = src.copy()
            trial[order[a], 0] = np.nan; trial[order[b_], 1] = np.nan
            pos = np.flatnonzero(~np.isfinite(trial[_device_order(trial)][:, :3]).all(axis=1))
            if len(pos) == 2 and pos[0] % 2 != pos[1] % 2:
                break
        else:
            continue
        break
    else:
        raise AssertionError("no pair of NaN points on lanes of different parity found")
    stf, sts = _compare(smhip, trial, velo20k, ("grid", "nan"))
    clean = np.ascontiguousarray(trial[np.isfinite(trial[:, :3]).all(axis=1)])
    stc, _ = _compare(smhip, clean, velo20k, ("grid", "nan_removed"))
    assert stf[0]["kept"] == stc[0]["kept"] and stf[0]["limit_d2"] == stc[0]["limit_d2"]


def test_whole_waves_without_a_kept_point(smhip, velo20k):
    """A contiguous twentieth of the device order displaced by +5 m in z (all of it would leave no iteration to the fused pass, see
    above): the displaced points stay together on the curve, whole waves of them keep nothing below the band (their sums stay
    exact zeros, their kept counts 0), the others go on as before."""
    src = np.array(velo20k["src"], dtype=np.float32, copy=True)
    order = _device_order(src)
    moved = order[4000:5000]
    src[moved, 2] += 5.0
    is_moved = np.zeros(len(src), dtype=bool); is_moved[moved] = True
    lanes = is_moved[_device_order(src)]
    waves = lanes[: len(lanes) // 64 * 64].reshape(-1, 64)
    assert waves.all(axis=1).sum() >= 1
    stf, sts = _compare(smhip, src, velo20k, ("grid", "twentieth"))
    assert 0 < stf[0]["kept"] <= len(src) - len(moved)
