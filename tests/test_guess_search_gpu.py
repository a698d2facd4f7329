"""The device correlative guess search (smhip_guess_search_*, staticmapping_amd/guess_search.py, csrc/guess_search.hip) against its
definition (tests/guess_search_ref.py): the bitmap's box, every source voxel, the WHOLE score volume cell for cell, the pick, the
scores and the returned transform -- all by equality, since nothing after rule 5 is a float and rules 3 to 5 are pinned operation by
operation.  Shapes are the smallest at which a kernel can go wrong: source rows around a wave (63, 64, 65) and around the sample rule
(4 096, 4 097), one target row, windows of one candidate, of half_xy 1, wider than the bitmap, 1 and 5 yaws, bitmap rows of 31, 32, 33,
64 and 65 voxels, negative coordinates, a source outside the box, mixed strides, non-finite rows, a resolution that is no power of
two, and the two 20 000-point scans of DESIGN.md's experiment at the default window."""
import ctypes

import numpy as np
import pytest

import guess_search_cases as cases
import guess_search_ref as ref
import staticmapping_amd as sm
from staticmapping_amd import _capi, synth
from staticmapping_amd import guess_search as gs

pytestmark = pytest.mark.gpu

INVALID, CAPACITY, NOT_READY = 1, 7, 4          # include/smhip.h
SMALL = dict(half_xy=3, half_z=1, yaw_steps=1)
TRUTH = synth.make_pose(t=(1.2, -0.7, 0.3), rpy_deg=(0, 0, 3.0))
GUESS = synth.make_pose(t=(2.2, -1.2, 0.3), rpy_deg=(0, 0, 1.0))


def new_handle(cap=32768):
    return sm.IcpFastHip(pair_slots=1, max_source_points=cap, max_target_points=cap)


@pytest.fixture(scope="module")
def handle():
    h = new_handle()
    yield h
    h.close()


def box_cloud(n, seed, lo=(-6, -5, -1), hi=(7, 6, 2), cols=4):
    rng = np.random.default_rng(seed)
    c = np.zeros((n, cols), np.float32)
    c[:, :3] = rng.uniform(lo, hi, (n, 3))
    c[:, 3] = rng.uniform(0, 1, n)
    return c


def source_of(target, n, seed, cols=4, noise=0.02):
    """n rows of the target seen from TRUTH (with repeats when n exceeds the target), a little noise added"""
    rng = np.random.default_rng(seed)
    rows = target[rng.integers(0, len(target), n), :3].astype(np.float64)
    inv = np.linalg.inv(TRUTH)
    s = np.zeros((n, cols), np.float32)
    s[:, :3] = rows @ inv[:3, :3].T + inv[:3, 3] + rng.normal(0, noise, (n, 3))
    return s


def check(h, target, source, guess, **options):
    want = ref.search(target, source, guess, **options)
    got = gs.search(h, target, source, guess, **options)
    dev = gs.last(h, got)
    print("candidates", got["n_candidates"], "used", got["n_source_used"], "box", dev["origin"], dev["extent"], "best", got["best"], got["best_score"],
          "guess", got["guess_score"], "runner-up", got["runner_up_score"], "| want", want["best"], want["best_score"], want["guess_score"],
          want["runner_up_score"], "| cells that differ", int((dev["volume"] != want["volume"]).sum()))
    assert np.array_equal(dev["origin"], want["origin"]) and np.array_equal(dev["extent"], want["extent"])
    assert got["n_source_used"] == want["n_source_used"] and got["n_candidates"] == want["n_candidates"]
    reach = want["reachable"]
    assert np.array_equal(dev["voxels"][reach], want["voxels"][reach])
    assert (dev["voxels"][~reach] == np.iinfo(np.int32).min).all()
    assert np.array_equal(dev["volume"], want["volume"])
    assert got["best"] == want["best"]
    assert (got["best_score"], got["guess_score"], got["runner_up_score"]) == (want["best_score"], want["guess_score"], want["runner_up_score"])
    assert np.array_equal(got["transform"], want["transform"])
    return got, dev, want


@pytest.mark.parametrize("n_source", [1, 63, 64, 65, 4096, 4097])
def test_source_sizes_around_a_wave_and_the_sample_rule(handle, n_source):
    target = box_cloud(700, 1)
    got, _, _ = check(handle, target, source_of(target, n_source, 2), GUESS, **SMALL)
    assert got["n_source_used"] == min(n_source, 4096)
    if n_source >= 63:
        assert got["best_score"] > got["guess_score"]


def test_sample_rule_with_a_small_cap(handle):
    target = box_cloud(300, 3)
    for n in (7, 8, 13, 100):
        got, _, _ = check(handle, target, source_of(target, n, 4), GUESS, max_source_points=7, **SMALL)
        assert got["n_source_used"] == 7


def test_one_target_row(handle):
    target = np.array([[0.3, -0.2, 0.1, 1.0]], np.float32)
    got, dev, _ = check(handle, target, source_of(np.repeat(target, 5, axis=0), 70, 5, noise=0.3), GUESS, half_xy=4, half_z=1, yaw_steps=1)
    assert tuple(dev["extent"]) == (1, 1, 1)


@pytest.mark.parametrize("window", [dict(half_xy=0, half_z=0, yaw_steps=0), dict(half_xy=1, half_z=0, yaw_steps=0), dict(half_xy=1, half_z=1, yaw_steps=2),
                                    dict(half_xy=40, half_z=9, yaw_steps=0), dict(half_xy=0, half_z=3, yaw_steps=2)])
def test_windows(handle, window):
    target = box_cloud(400, 6)                       # a box of 26 x 22 x 6 voxels: the fourth window is wider than the bitmap
    got, _, _ = check(handle, target, source_of(target, 300, 7), GUESS, **window)
    if sum(window.values()) == 0:
        assert got["n_candidates"] == 1 and got["best"] == (0, 0, 0, 0) and got["best_score"] == got["guess_score"] and got["runner_up_score"] == 0


@pytest.mark.parametrize("row", [31, 32, 33, 64, 65])
def test_bitmap_rows_of_this_many_voxels(handle, row):
    target = box_cloud(500, 8, lo=(-3.0, -2, 0), hi=(-3.0 + 0.5 * row, 2, 1))
    target[0, 0], target[1, 0] = -2.99, -3.0 + 0.5 * row - 0.01           # both ends of the row are occupied
    _, dev, _ = check(handle, target, source_of(target, 200, 9), GUESS, **SMALL)
    assert dev["extent"][0] == row


def test_negative_coordinates_and_a_source_outside_the_box(handle):
    target = box_cloud(400, 10, lo=(-30, -25, -4), hi=(-20, -18, -2))
    check(handle, target, source_of(target, 150, 11), GUESS, **SMALL)
    far = source_of(target, 150, 12)
    far[:, :3] += np.float32(500.0)
    got, dev, _ = check(handle, target, far, GUESS, **SMALL)
    assert got["best_score"] == 0 and got["best"] == (0, 0, 0, 0) and (dev["voxels"] == np.iinfo(np.int32).min).all()


def test_mixed_strides_and_non_finite_rows(handle):
    t4 = box_cloud(300, 13)
    s4 = source_of(t4, 130, 14)
    t5, s5 = np.zeros((300, 5), np.float32), np.zeros((130, 5), np.float32)
    t5[:, :4], s5[:, :4] = t4, s4
    t5[:, 4], s5[:, 4] = 7.0, np.nan                              # the fifth column is not a coordinate
    a, _, _ = check(handle, t5, s4, GUESS, **SMALL)
    b, _, _ = check(handle, t4, s5, GUESS, **SMALL)
    assert a["best"] == b["best"] and a["best_score"] == b["best_score"]
    for c, col, v in ((t5, 0, np.nan), (t5, 2, np.inf), (s5, 1, -np.inf), (s5, 0, np.nan)):
        c[::3, col] = v
    t5[1, :3] = np.nan
    got, _, _ = check(handle, t5, s5, GUESS, **SMALL)
    assert got["n_source_used"] == len(ref.finite_rows(s5)) < 130


def test_resolution_that_is_no_power_of_two(handle):
    target = box_cloud(600, 15)
    target[:40, :3] = np.round(target[:40, :3] / np.float32(0.3)) * np.float32(0.3)     # rows on or next to voxel borders
    source = source_of(target, 256, 16)
    check(handle, target, source, GUESS, resolution=0.3, **SMALL)
    check(handle, target, source, np.eye(4), resolution=0.3, half_xy=2, half_z=1, yaw_steps=0)


def test_the_experiment_at_the_default_window(handle):
    target, source, truth, guess = cases.experiment()
    got, _, _ = check(handle, target, source, guess)
    assert got["n_candidates"] == 176505 and got["n_source_used"] == 4096
    assert np.abs(got["transform"][:3, 3] - truth[:3, 3]).max() <= 0.5 and got["best_score"] > got["guess_score"]


def test_two_calls_and_a_call_after_a_larger_one_give_the_same_bits(handle):
    target = box_cloud(500, 17)
    source = source_of(target, 200, 18)
    first = gs.search(handle, target, source, GUESS, **SMALL)
    v1 = gs.last(handle)
    big_t, big_s, _, big_g = cases.experiment()
    gs.search(handle, big_t, big_s, big_g)                            # a larger bitmap, volume and voxel table in between
    second = gs.search(handle, target, source, GUESS, **SMALL)
    v2 = gs.last(handle, second)
    fresh_handle = new_handle()
    third = gs.search(fresh_handle, target, source, GUESS, **SMALL)
    v3 = gs.last(fresh_handle, third)
    fresh_handle.close()
    for r, v in ((second, v2), (third, v3)):
        assert all(np.array_equal(v[k], v1[k]) for k in ("volume", "origin", "extent", "voxels"))
        assert all(np.array_equal(r[k], first[k]) for k in ("transform", "best", "best_score", "guess_score", "runner_up_score"))


def _raw(h, target, n_t, stride_t, source, n_s, stride_s, guess, options, result):
    p = lambda a: a.ctypes.data_as(_capi.c_float_p) if a is not None else None
    g = np.ascontiguousarray(np.asarray(guess, np.float64).reshape(4, 4).T) if guess is not None else None
    return h._lib.smhip_guess_search_f32(h._h, p(target), n_t, stride_t, p(source), n_s, stride_s, g.ctypes.data_as(_capi.c_double_p) if g is not None else None,
                                         ctypes.byref(options) if options is not None else None, ctypes.byref(result) if result is not None else None)


def test_refusals_write_nothing():
    h = new_handle(cap=1024)
    target, source = box_cloud(300, 19), source_of(box_cloud(300, 19), 100, 20)
    r = _capi.GuessSearchResult()
    ctypes.memset(ctypes.byref(r), 0x5A, ctypes.sizeof(r))
    untouched = bytes(r)
    vol = np.zeros(1, np.int32)
    assert h._lib.smhip_guess_search_last(h._h, vol.ctypes.data_as(_capi.c_int32_p), 1, None, None, None, 0) == NOT_READY
    o = lambda **kw: gs.make_options(**dict(SMALL, **kw))
    nan_cloud = np.full((50, 4), np.nan, np.float32)
    bad_guess = GUESS.copy()
    bad_guess[1, 3] = np.inf
    huge = np.zeros((5, 4), np.float32)
    huge[:, 0] = 3.0e9                                               # floor(x / 0.5) is beyond 2^30
    refused = [
        (INVALID, (None, 300, 4, source, 100, 4, GUESS, o(), r)), (INVALID, (target, 300, 4, None, 100, 4, GUESS, o(), r)),
        (INVALID, (target, 300, 4, source, 100, 4, None, o(), r)), (INVALID, (target, 300, 4, source, 100, 4, GUESS, None, r)),
        (INVALID, (target, 300, 3, source, 100, 4, GUESS, o(), r)), (INVALID, (target, 300, 4, source, 100, 6, GUESS, o(), r)),
        (INVALID, (target, 0, 4, source, 100, 4, GUESS, o(), r)), (INVALID, (target, 300, 4, source, 0, 4, GUESS, o(), r)),
        (INVALID, (target, 300, 4, source, 100, 4, GUESS, o(resolution=0.0), r)), (INVALID, (target, 300, 4, source, 100, 4, GUESS, o(resolution=float("nan")), r)),
        (INVALID, (target, 300, 4, source, 100, 4, GUESS, o(half_xy=-1), r)), (INVALID, (target, 300, 4, source, 100, 4, GUESS, o(half_z=-1), r)),
        (INVALID, (target, 300, 4, source, 100, 4, GUESS, o(yaw_steps=-1), r)), (INVALID, (target, 300, 4, source, 100, 4, GUESS, o(max_source_points=0), r)),
        (INVALID, (target, 300, 4, source, 100, 4, GUESS, o(yaw_step=float("inf")), r)), (INVALID, (target, 300, 4, source, 100, 4, bad_guess, o(), r)),
        (CAPACITY, (target, 300, 4, source, 100, 4, GUESS, o(half_xy=2896, half_z=0, yaw_steps=0), r)),
        (CAPACITY, (np.tile(target, (4, 1)), 1025, 4, source, 100, 4, GUESS, o(), r)), (CAPACITY, (target, 300, 4, np.tile(source, (11, 1)), 1025, 4, GUESS, o(), r)),
        (INVALID, (nan_cloud, 50, 4, source, 100, 4, GUESS, o(), r)), (INVALID, (target, 300, 4, nan_cloud, 50, 4, GUESS, o(), r)),
        (CAPACITY, (huge, 5, 4, source, 100, 4, GUESS, o(), r)), (CAPACITY, (target, 300, 4, huge, 5, 4, GUESS, o(), r)),
    ]
    for k, (status, args) in enumerate(refused):
        got = _raw(h, *args)
        print(k, "status", got, h._lib.smhip_last_error(h._h).decode())
        assert got == status, (k, got, status)
        assert bytes(r) == untouched and len(h._lib.smhip_last_error(h._h)) > 10
    assert _raw(h, target, 300, 4, source, 100, 4, GUESS, o(), None) == INVALID
    # and the handle still searches, with the bits of the definition
    check(h, target, source, GUESS, **SMALL)
    h.close()
