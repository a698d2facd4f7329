"""The GPU cases of tests/test_m2dp_gpu.py, one per process: `python tests/m2dp_gpu_cases.py CASE`.  Every case prints its
figures before it asserts and ends with the line `ok CASE`."""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

try:                                  # one HIP runtime per process: torch's first (tests/conftest.py)
    import torch  # noqa: F401
except ImportError:
    pass
import numpy as np

import staticmapping_amd as sm
import m2dp_ref as mr
import submap_ref as sr
from staticmapping_amd import _capi, synth
from staticmapping_amd import m2dp as dm
from staticmapping_amd import submap as dsub

NONDEFAULT = dict(t=8, p=2, q=4, r=0.5, max_distance=50.0)


def _status_codes():
    import re
    txt = open(os.path.join(ROOT, "include", "smhip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"(SMHIP_[A-Z_]+)\s*=\s*(-?\d+)", txt)}


def handle(cap=131072):
    return sm.IcpFastHip(pair_slots=1, max_source_points=cap, max_target_points=cap)


def scan_a(n):
    return synth.scan_pair("cfg2", n)[0]


def scan_c(n):
    return synth.velodyne_scan(synth.make_scene(7), synth.make_pose(t=(20, -15, 0), rpy_deg=(0, 0, 70)), seed=9, n_points=n)


def small_scan():
    return synth.velodyne_scan(synth.make_scene(0), synth.make_pose(), seed=2, n_points=4099)


def far_cloud():
    """scan a without its rows beyond 42 m, scaled by 6: about a tenth lies beyond max_distance, nothing beyond 256 m (where
    one float ulp would exceed the projection bound)"""
    a = scan_a(20_000)
    a = a[np.linalg.norm(a[:, :3], axis=1) <= 42.0].copy()
    a[:, :3] *= np.float32(6.0)
    return a


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def device(m, cloud, o):
    opts = dm.make_options(**o)
    d = dm.m2dp(m, cloud, opts)
    proj, kept, A, n_kept = dm.last(m, len(cloud), opts)
    return d, proj, kept, A, n_kept


def case_projection():
    m = handle()
    o = mr.options()
    for label, cloud in (("4099", small_scan()), ("20000", scan_a(20_000)), ("far", far_cloud())):
        _, proj, kept, _, n_kept = device(m, cloud, o)
        want, wkept, w = mr.pre_process(cloud, o)
        gaps = ((w[0] - w[1]) / w[0], (w[1] - w[2]) / w[1])
        err = float(np.abs(proj.astype(np.float64) - want.astype(np.float64)).max())
        ln = mr.get_length(want)
        edge = np.abs(ln - o["max_distance"]) <= 1e-5 * o["max_distance"]
        differ = kept != wkept
        print(f"{label}: n {len(cloud)} eigenvalue gaps {gaps[0]:.3f} {gaps[1]:.3f}; projected3 max |device - restatement| {err:.3e} m "
              f"(rows bit-equal: {bits_equal(proj, want)}); kept {int(kept.sum())} of {len(cloud)} (restatement {int(wkept.sum())}), "
              f"differing {int(differ.sum())}, within 1e-5 of max_distance {int(edge.sum())}; n_kept {n_kept}")
        assert min(gaps) > 0.10, label
        assert err <= 1.6e-5, label
        assert not (differ & ~edge).any(), label
        assert n_kept == int(kept.sum()), label
        if label == "far":
            share = 1.0 - wkept.mean()
            print(f"far: share beyond max_distance {share:.3f}")
            assert 0.05 < share < 0.2
    m.close()


def check_histogram(label, cloud, o, m):
    d, proj, kept, A, n_kept = device(m, cloud, o)
    s = mr.samples(proj[kept], o)
    flagged = s["flagged"]
    A_lo = mr.histogram_of(s, o, ~flagged)
    F = mr.flagged_spread(s, o)
    A_all = mr.histogram_of(s, o)
    A64 = A.astype(np.int64)
    share = flagged.mean()
    print(f"{label}: n {len(cloud)} kept {n_kept} samples {flagged.size} flagged {int(flagged.sum())} ({100 * share:.4f} %); cells where the "
          f"device differs from the restatement's A: {int((A64 != A_all).sum())} (sum |diff| {int(np.abs(A64 - A_all).sum())}); "
          f"below A_lo {int((A64 < A_lo).sum())}, above A_lo + F {int((A64 > A_lo + F).sum())}")
    assert share <= 1e-3, label
    assert (A64 >= A_lo).all() and (A64 <= A_lo + F).all(), label
    assert (A64.sum(axis=1) == n_kept).all() and n_kept == int(kept.sum()), label
    # the descriptor, given the device's own A
    want = mr.descriptor_of(A64)
    views = o["p"] * o["q"]
    err = float(np.abs(d.astype(np.float64) - want.astype(np.float64)).max())
    nu, nv = float(np.linalg.norm(d[:views].astype(np.float64))), float(np.linalg.norm(d[views:].astype(np.float64)))
    print(f"{label}: descriptor max |device - numpy SVD of the device's A| {err:.3e}; |u1| - 1 = {nu - 1:.2e}, |v1| - 1 = {nv - 1:.2e}; "
          f"sum(u1) {float(d[:views].sum()):.4f}")
    assert len(d) == mr.length(o) == dm.length(dm.make_options(**o)), label
    assert err <= 1e-6 and abs(nu - 1) <= 1e-6 and abs(nv - 1) <= 1e-6, label
    return d


def case_histogram():
    m = handle()
    check_histogram("20000 defaults", scan_a(20_000), mr.options(), m)
    check_histogram("4099 defaults", small_scan(), mr.options(), m)
    check_histogram("20000 t 8 p 2 q 4 r 0.5 max_distance 50", scan_a(20_000), mr.options(**NONDEFAULT), m)
    check_histogram("far defaults", far_cloud(), mr.options(), m)
    m.close()


def case_big():
    m = handle()
    check_histogram("120000 defaults", scan_a(120_000), mr.options(), m)
    m.close()


def drive(n_scans, n_points):
    scene = synth.make_scene(0)
    poses = [synth.make_pose(t=(0.8 * k, 0.03 * k, 0.0), rpy_deg=(0, 0, 0.6 * k)) for k in range(n_scans)]
    return poses, [synth.velodyne_scan(scene, P, seed=90 + k, n_points=n_points) for k, P in enumerate(poses)]


def case_same_bits():
    m = handle()
    o = mr.options()
    cloud = scan_a(20_000)
    d1, _, _, A1, _ = device(m, cloud, o)
    other, _, _, _, _ = device(m, small_scan(), o)               # something else in between
    d2, _, _, A2, _ = device(m, cloud, o)
    print("two calls: A equal", np.array_equal(A1, A2), "descriptor bit-equal", bits_equal(d1, d2), "; another cloud differs", not bits_equal(d1[:64], other[:64]))
    assert np.array_equal(A1, A2) and bits_equal(d1, d2) and not bits_equal(d1[:64], other[:64])
    # a device-built submap: the resident cloud against its downloaded rows
    poses, scans = drive(3, 20_000)
    n = dsub.build_submap_resident(m, scans, sr.local_poses(poses), sr.text_voxel_size(0.1))
    before, bsrc = dsub.get_submap(m, n)
    opts = dm.make_options()
    d_res = dm.m2dp_from_filter_output(m, opts)
    _, _, A_res, k_res = dm.last(m, n, opts)
    after, asrc = dsub.get_submap(m, n)
    d_up = dm.m2dp(m, before, opts)
    _, _, A_up, k_up = dm.last(m, n, opts)
    still, ssrc = dsub.get_submap(m, n)
    print(f"submap of {n} rows: resident = uploaded: descriptor {bits_equal(d_res, d_up)}, A {np.array_equal(A_res, A_up)}, kept {k_res} {k_up}; "
          f"workspace unchanged {bits_equal(before, after) and bits_equal(before, still)}")
    assert bits_equal(d_res, d_up) and np.array_equal(A_res, A_up) and k_res == k_up
    assert bits_equal(before, after) and np.array_equal(bsrc, asrc) and bits_equal(before, still) and np.array_equal(bsrc, ssrc)
    w = mr.pca_axes(before)[2]
    print(f"submap eigenvalue gaps {(w[0] - w[1]) / w[0]:.3f} {(w[1] - w[2]) / w[1]:.3f}")
    m.close()


def case_gate():
    m = handle()
    o = mr.options()
    a, b, _ = synth.scan_pair("cfg2", 20_000)
    clouds = dict(a=a, b=b, c=scan_c(20_000))
    dev = {k: dm.m2dp(m, v) for k, v in clouds.items()}
    ref = {k: mr.m2dp(v, o) for k, v in clouds.items()}
    moved = {k: mr.descriptor_of(mr.moved_histogram(r["samples"], o)) for k, r in ref.items()}
    for (i, j) in (("a", "b"), ("a", "c")):
        want = mr.match(ref[i]["descriptor"], ref[j]["descriptor"])
        change = max(abs(mr.match(moved[i], ref[j]["descriptor"]) - want), abs(mr.match(ref[i]["descriptor"], moved[j]) - want),
                     abs(mr.match(moved[i], moved[j]) - want))
        bound = 4.0 * change
        got = dm.match(dev[i], dev[j])
        host = mr.match(dev[i], dev[j])
        print(f"{i}-{j}: device score {got:.7f} restatement {want:.7f} |difference| {abs(got - want):.2e}; flagged samples moved change the "
              f"restatement's score by {change:.2e}, bound {bound:.2e}; smhip_m2dp_match vs the restated formula {abs(got - host):.1e}")
        assert abs(want - 0.98) > 0.005, "choose other seeds"
        assert abs(got - host) <= 1e-12
        assert abs(got - want) <= bound, (i, j)
        assert (got > 0.98) == (j == "b")                         # the gate is strict (loop_detector.cc:114-116)
    assert dm.match(dev["a"], dev["a"][:-1]) == -1.0 and dm.match(dev["a"][:9], dev["a"][:9]) == -1.0
    m.close()


def case_refusals():
    codes = _status_codes()
    inv, cap, notready = codes["SMHIP_ERR_INVALID_ARGUMENT"], codes["SMHIP_ERR_CAPACITY"], codes["SMHIP_ERR_NOT_READY"]
    lib = _capi.load_library()
    o = dm.make_options()
    ln = dm.length(o)
    assert ln == 64 + 32 * 16
    bad_opts = {"r 1e-7": dict(r=1e-7), "r nan": dict(r=float("nan")), "max_distance inf": dict(max_distance=float("inf")),
                "max_distance 0": dict(max_distance=0.0), "t 0": dict(t=0), "p 0": dict(p=0), "q -1": dict(q=-1),
                "p q = 65 views": dict(p=5, q=13), "l t = 8208 columns": dict(t=513, r=1.0, max_distance=256.0)}
    for label, kw in bad_opts.items():
        print("length", label, dm.length(dm.make_options(**kw)))
        assert dm.length(dm.make_options(**kw)) == -1, label
    assert dm.length(dm.make_options(p=4, q=16, t=512, r=1.0, max_distance=256.0)) == 64 + 8192
    assert lib.smhip_m2dp_length(None) == -1

    m = sm.IcpFastHip(pair_slots=1, max_source_points=2048, max_target_points=4096)
    h = m._h
    rng = np.random.default_rng(3)
    out = np.full(ln, 7.0, np.float32)
    op, fp = ctypes.byref(o), out.ctypes.data_as(_capi.c_float_p)
    st = lib.smhip_m2dp_from_filter_output(h, op, fp, ln)
    print("from_filter_output on a fresh handle:", st, lib.smhip_last_error(h).decode())
    assert st == notready and lib.smhip_last_error(h).decode()
    st = lib.smhip_m2dp_last(h, None, None, None, 0, None)
    assert st == notready

    frames = [(rng.uniform(-30, 30, (n, 4)) * np.array([1.0, 0.6, 0.1, 1.0])).astype(np.float32) for n in (500, 700)]
    local = [np.eye(4), synth.make_pose(t=(1.0, 0.2, 0.0), rpy_deg=(0, 0, 3.0))]
    resident, rsrc = dsub.build_submap(m, frames, local, 0.5)
    good = dm.m2dp_from_filter_output(m, o)
    out[:] = good
    pts = (rng.uniform(-30, 30, (4097, 4)) * np.array([1.0, 0.5, 0.2, 1.0])).astype(np.float32)
    pp = pts.ctypes.data_as(_capi.c_float_p)
    nan_row = pts[:1000].copy(); nan_row[17, 1] = np.nan
    inf_row = pts[:1000].copy(); inf_row[999, 2] = np.inf
    tiny = dm.make_options(max_distance=1e-3, r=1e-4)            # every row but the centroid's neighbourhood is dropped: sigma1 = 0
    tiny_len = dm.length(tiny)
    tiny_out = np.full(tiny_len, 7.0, np.float32)
    bad = dm.make_options(r=1e-7)
    calls = {
        "null points": (inv, lambda: lib.smhip_m2dp_f32(h, None, 4, 1000, op, fp, ln)),
        "null descriptor": (inv, lambda: lib.smhip_m2dp_f32(h, pp, 4, 1000, op, None, ln)),
        "null options": (inv, lambda: lib.smhip_m2dp_f32(h, pp, 4, 1000, None, fp, ln)),
        "stride 3": (inv, lambda: lib.smhip_m2dp_f32(h, pp, 3, 1000, op, fp, ln)),
        "stride 6": (inv, lambda: lib.smhip_m2dp_f32(h, pp, 6, 600, op, fp, ln)),
        "n 1": (inv, lambda: lib.smhip_m2dp_f32(h, pp, 4, 1, op, fp, ln)),
        "n 0": (inv, lambda: lib.smhip_m2dp_f32(h, pp, 4, 0, op, fp, ln)),
        "len - 1": (inv, lambda: lib.smhip_m2dp_f32(h, pp, 4, 1000, op, fp, ln - 1)),
        "refused options": (inv, lambda: lib.smhip_m2dp_f32(h, pp, 4, 1000, ctypes.byref(bad), fp, ln)),
        "4097 rows on a 4096 handle": (cap, lambda: lib.smhip_m2dp_f32(h, pp, 4, 4097, op, fp, ln)),
        "resident: null descriptor": (inv, lambda: lib.smhip_m2dp_from_filter_output(h, op, None, ln)),
        "resident: len + 1": (inv, lambda: lib.smhip_m2dp_from_filter_output(h, op, fp, ln + 1)),
        "resident: refused options": (inv, lambda: lib.smhip_m2dp_from_filter_output(h, ctypes.byref(bad), fp, ln)),
        "a NaN row (found by the kernels)": (inv, lambda: lib.smhip_m2dp_f32(h, nan_row.ctypes.data_as(_capi.c_float_p), 4, 1000, op, fp, ln)),
        "an infinite row (found by the kernels)": (inv, lambda: lib.smhip_m2dp_f32(h, inf_row.ctypes.data_as(_capi.c_float_p), 4, 1000, op, fp, ln)),
    }
    for label, (want_status, call) in calls.items():
        st = call()
        msg = lib.smhip_last_error(h).decode()
        after, asrc = dsub.get_submap(m, len(resident))
        print(f"{label}: status {st} ({msg!r}); descriptor untouched {bits_equal(out, good)}, resident cloud unchanged {bits_equal(after, resident)}")
        assert st == want_status, label
        assert msg, label
        assert bits_equal(out, good), label
        assert bits_equal(after, resident) and np.array_equal(asrc, rsrc), label
    # no row within max_distance: two far clusters, the centroid between them
    two = np.zeros((1000, 4), np.float32)
    two[:500, 0], two[500:, 0] = -5.0, 5.0
    two[:, 1] = rng.uniform(-1, 1, 1000) * 0.3
    two[:, 2] = rng.uniform(-1, 1, 1000) * 0.01
    st = lib.smhip_m2dp_f32(h, two.ctypes.data_as(_capi.c_float_p), 4, 1000, ctypes.byref(tiny), tiny_out.ctypes.data_as(_capi.c_float_p), tiny_len)
    msg = lib.smhip_last_error(h).decode()
    print(f"no row within max_distance: status {st} ({msg!r}); descriptor untouched {bool((tiny_out == 7.0).all())}")
    assert st == inv and msg and (tiny_out == 7.0).all()
    nk = ctypes.c_int(-1)
    assert lib.smhip_m2dp_last(h, None, None, None, 0, ctypes.byref(nk)) == 0 and nk.value == 0
    # exactly the capacity is taken, and the handle still answers as before
    st = lib.smhip_m2dp_f32(h, pp, 4, 4096, op, fp, ln)
    assert st == 0 and not bits_equal(out, good)
    again = dm.m2dp_from_filter_output(m, o)
    assert bits_equal(again, good)
    assert lib.smhip_m2dp_last(h, None, None, None, 5, None) == 0           # a_len is only read with A
    A = np.zeros(5, np.int32)
    assert lib.smhip_m2dp_last(h, None, None, A.ctypes.data_as(_capi.c_int32_p), 5, None) == inv
    # a resident cloud of one row: refused before anything is touched
    one, _ = dsub.build_submap(m, [frames[0][:1]], local[:1], 0.0)
    out[:] = good
    st = lib.smhip_m2dp_from_filter_output(h, op, fp, ln)
    msg = lib.smhip_last_error(h).decode()
    print(f"resident cloud of {len(one)} row: status {st} ({msg!r})")
    assert len(one) == 1 and st == inv and msg and bits_equal(out, good)
    m.close()


CASES = {"projection": case_projection, "histogram": case_histogram, "big": case_big, "same_bits": case_same_bits, "gate": case_gate,
         "refusals": case_refusals}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print("ok", sys.argv[1])
