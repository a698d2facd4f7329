"""IcpFast with inner motion compensation on the device (smhip_icp_set_inner_compensation) against its restatement
(tests/icp_compensation_ref.py): comp_apply's block edges, pose parity, the caller's row index, batches, and the rigid paths of a
handle that has used the mode.  Tolerances: ids as tests/test_icp_gpu.py states them for FindClosests, SE(3) within
BASELINE.json's 1e-4 rad / 1e-3 m, score within 1e-4."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_compensation_ref as cr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROT_TOL = 1e-4      # rad, BASELINE.json north_star
TRANS_TOL = 1e-3    # m


@pytest.fixture(scope="module")
def smhip():
    import staticmapping_amd as sm
    from staticmapping_amd import _capi
    lib = _capi.load_library()
    assert lib.smhip_device_count() >= 1, "no gfx950 device visible"
    return sm


@pytest.fixture(scope="module")
def pair3k():
    """3 000-point scans against their own CalculateNormals target: the batches' pair."""
    from staticmapping_amd import synth
    from oracle import cref
    a, b, T = synth.scan_pair("cfg2", n_points=3000)
    q, n, _ = cref.calculate_normals(a[:, :3].astype(np.float64))
    ok = np.isfinite(n).all(axis=1)
    return dict(src=b, q=q[ok], n=n[ok], guess=synth.make_pose(t=(0.6, 0.0, 0.0)))


def _matcher(smhip, case, n_src=None, slots=1, **opts):
    n_src = len(case["src"]) if n_src is None else n_src
    return smhip.IcpFastHip(pair_slots=slots, max_source_points=n_src, max_target_points=len(case["q"]), **opts)


def _src64(case, n=None):
    return case["src"][:n, :3].astype(np.float64)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_comp_apply_block_edges(smhip, velo20k, n):
    """One iteration over sources that end before, at and behind a workgroup of comp_apply: the matches of the step cloud it
    wrote are the restatement's (every match exact, so that the rejected ones compare too)."""
    c = velo20k
    m = _matcher(smhip, c, n_src=n, inner_compensation=True, max_iteration=1, early_exit=0, exact_matches=1)
    assert m.inner_compensation
    m.set_input_source(c["src"][:n])
    m.set_input_target(c["q"], c["n"])
    ok, R = m.align(c["guess"])
    ids, d2 = m.get_matches(n)
    m.close()
    trace = []
    cr.icp_fast_align_compensated(_src64(c, n), c["q"], c["n"], guess=c["guess"], max_iteration=1, early_exit=False, trace=trace)
    ids_o, d2_o = trace[0]["ids"], trace[0]["d2"]
    same = ids == ids_o
    print(f"[comp_apply n={n}] {int((~same).sum())} of {n} ids differ, max |d2 - oracle| / oracle = {np.max(np.abs(d2 - d2_o) / np.maximum(d2_o, 1e-12)):.2e}")
    assert ok
    assert same.mean() >= 0.9999
    assert np.allclose(d2[~same], d2_o[~same], rtol=1e-4, atol=1e-9)
    assert np.allclose(d2, d2_o, rtol=2e-4, atol=1e-8)


_REF = {}


def _reference(name, case, guess, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = cr.icp_fast_align_compensated(_src64(case), case["q"], case["n"], guess=guess, **kw)
    return _REF[key]


@pytest.mark.parametrize("run", ["one", "twenty", "early_exit"])
@pytest.mark.parametrize("fixture_name", ["cfg1", "velo20k"])
def test_pose_parity(request, smhip, fixture_name, run):
    c = request.getfixturevalue(fixture_name)
    guess = c.get("guess", np.eye(4))
    opts = {"one": dict(max_iteration=1, early_exit=0), "twenty": dict(max_iteration=20, early_exit=0), "early_exit": dict(max_iteration=100, early_exit=1)}[run]
    m = _matcher(smhip, c, inner_compensation=True, **opts)
    m.set_input_source(c["src"])
    m.set_input_target(c["q"], c["n"])
    ok, R = m.align(guess)
    score, stats = m.get_fitness_score(), m.last_stats[0]
    m.close()
    R_o, score_o, it_o = _reference(fixture_name, c, guess, max_iteration=opts["max_iteration"], early_exit=bool(opts["early_exit"]))
    da, dt = smhip.se3_error(R, R_o)
    print(f"[inner compensation parity {fixture_name}/{run}] {da:.2e} rad / {dt:.2e} m, score {abs(score - score_o):.2e}, iterations {stats['iterations']} / {it_o}")
    assert ok and da < ROT_TOL and dt < TRANS_TOL, (da, dt)
    assert abs(score - score_o) < 1e-4
    assert stats["iterations"] == it_o
    # and it is not the rigid alignment of the same rows
    if run != "one" and fixture_name == "velo20k":
        from oracle import cref
        rigid = cref.icp_fast_align(_src64(c), c["q"], c["n"], guess=guess, max_iteration=opts["max_iteration"], early_exit=bool(opts["early_exit"]))
        assert smhip.se3_error(R, rigid["result"])[1] > 10 * TRANS_TOL


def test_the_factor_follows_the_uploaded_row_not_the_device_order(smhip, velo20k):
    """Rows permuted before upload: the device orders them along its own curve either way, and the result is the restatement's
    for the rows as uploaded -- another sweep order, another alignment than the unpermuted upload's."""
    c = velo20k
    perm = np.random.default_rng(3).permutation(len(c["src"]))
    src = np.ascontiguousarray(c["src"][perm])
    m = _matcher(smhip, c, inner_compensation=True, max_iteration=20, early_exit=0)
    m.set_input_source(src)
    m.set_input_target(c["q"], c["n"])
    ok, R = m.align(c["guess"])
    m.close()
    R_o, _, _ = cr.icp_fast_align_compensated(src[:, :3].astype(np.float64), c["q"], c["n"], guess=c["guess"], max_iteration=20, early_exit=False)
    da, dt = smhip.se3_error(R, R_o)
    assert ok and da < ROT_TOL and dt < TRANS_TOL, (da, dt)
    R_u, _, _ = _reference("velo20k", c, c["guess"], max_iteration=20, early_exit=False)
    assert smhip.se3_error(R, R_u)[1] > 10 * TRANS_TOL


def test_ragged_batch_slots_equal_single_runs(smhip, velo20k, cfg1):
    cases = [velo20k, cfg1, velo20k]
    guesses = [velo20k["guess"], np.eye(4), np.eye(4)]
    cap_s = max(len(c["src"]) for c in cases); cap_t = max(len(c["q"]) for c in cases)
    mb = smhip.IcpFastHip(pair_slots=3, max_source_points=cap_s, max_target_points=cap_t, inner_compensation=True)
    for s, c in enumerate(cases):
        mb.set_input_source(c["src"], slot=s)
        mb.set_input_target(c["q"], c["n"], slot=s)
    Rb, sb, stb = mb.align_batch(3, guesses)
    mb.close()
    for s, c in enumerate(cases):
        m1 = smhip.IcpFastHip(max_source_points=cap_s, max_target_points=cap_t, inner_compensation=True)
        m1.set_input_source(c["src"]); m1.set_input_target(c["q"], c["n"])
        ok, R1 = m1.align(guesses[s])
        assert stb[s]["iterations"] == m1.last_stats[0]["iterations"]
        da, dt = smhip.se3_error(Rb[s], R1)
        assert da < 1e-7 and dt < 1e-6
        assert abs(sb[s] - m1.get_fitness_score()) < 1e-9
        m1.close()
    # and slot 0 is the restatement's alignment, not only the single run's
    R_o, _, it_o = _reference("velo20k", velo20k, velo20k["guess"], max_iteration=100, early_exit=True)
    da, dt = smhip.se3_error(Rb[0], R_o)
    assert da < ROT_TOL and dt < TRANS_TOL and stb[0]["iterations"] == it_o


@pytest.mark.parametrize("pairs", [16, 32])
def test_batch_of_small_clouds_equals_single_runs(smhip, pair3k, pairs):
    """16 pairs of 3 000-point clouds are one part of the plan (a batch is cut at 32 pairs: plan::kMinPartPairs), 32 pairs two
    parts on two streams, each with its own comp_apply per iteration."""
    from staticmapping_amd import synth
    c = pair3k
    guesses = [c["guess"] @ synth.make_pose(t=(0.02 * k, -0.01 * k, 0.0), rpy_deg=(0, 0, 0.1 * k)) for k in range(4)]
    m = _matcher(smhip, c, slots=pairs, inner_compensation=True, max_iteration=12, early_exit=0)
    m.set_input_source(c["src"]); m.set_input_target(c["q"], c["n"])
    for s in range(1, pairs):
        m.copy_slot(0, s)
    R, sc, st = m.align_batch(pairs, [guesses[s % 4] for s in range(pairs)])
    m.close()
    m1 = _matcher(smhip, c, inner_compensation=True, max_iteration=12, early_exit=0)
    m1.set_input_source(c["src"]); m1.set_input_target(c["q"], c["n"])
    single = [m1.align(g)[1] for g in guesses]
    m1.close()
    for s in range(pairs):
        da, dt = smhip.se3_error(R[s], single[s % 4])
        assert st[s]["iterations"] == 12 and da < 1e-7 and dt < 1e-6, (s, da, dt)
    R_o, _, _ = cr.icp_fast_align_compensated(_src64(c), c["q"], c["n"], guess=guesses[1], max_iteration=12, early_exit=False)
    da, dt = smhip.se3_error(R[1], R_o)
    assert da < ROT_TOL and dt < TRANS_TOL, (da, dt)


def _rigid_outputs(m, c, lib):
    import ctypes
    from staticmapping_amd import _capi
    ok, R = m.align(c["guess"])
    score, stats = m.get_fitness_score(), dict(m.last_stats[0])
    ids_a, d2_a = m.get_matches(len(c["src"]))
    ids, d2 = m.find_closests(c["guess"], len(c["src"]))
    Tc = np.ascontiguousarray(np.asarray(R, np.float64).T).reshape(-1)
    ts, kept = ctypes.c_double(0), ctypes.c_int32(0)
    m._check(lib.smhip_icp_trimmed_score(m._h, 0, Tc.ctypes.data_as(_capi.c_double_p), 0.7, ctypes.byref(ts), ctypes.byref(kept)))
    return dict(R=np.asarray(R).copy(), score=score, it=stats["iterations"], kept=stats["kept"], ids_a=ids_a, d2_a=d2_a.view(np.uint32),
                ids=ids, d2=d2.view(np.uint32), ts=ts.value, ts_kept=kept.value)


def test_rigid_paths_are_untouched_by_a_compensated_align(smhip, velo20k):
    """A handle that enabled the mode, aligned, and disabled it again gives bit for bit the Align, find_closests and
    trimmed_score of a handle that never heard of it; with the mode still ON, find_closests and trimmed_score are the same rigid
    passes."""
    from staticmapping_amd import _capi
    lib = _capi.load_library()
    c = velo20k
    fresh = _matcher(smhip, c)
    fresh.set_input_source(c["src"]); fresh.set_input_target(c["q"], c["n"])
    want = _rigid_outputs(fresh, c, lib)
    fresh.close()
    m = _matcher(smhip, c)
    m.set_input_source(c["src"]); m.set_input_target(c["q"], c["n"])
    m.set_inner_compensation(True)
    ok, Rc = m.align(c["guess"])
    assert ok and smhip.se3_error(Rc, want["R"])[1] > 10 * TRANS_TOL
    # mode still on: the passes that are rigid by definition
    ids, d2 = m.find_closests(c["guess"], len(c["src"]))
    assert np.array_equal(ids, want["ids"]) and np.array_equal(d2.view(np.uint32), want["d2"])
    m.set_inner_compensation(False)
    assert not m.inner_compensation
    got = _rigid_outputs(m, c, lib)
    m.close()
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def test_other_search_modes_are_refused(smhip, cfg1):
    c = cfg1
    for mode in (2, 0):                                   # SMHIP_NN_NABO, SMHIP_NN_BRUTE
        m = _matcher(smhip, c, nn_mode=mode, inner_compensation=True)
        m.set_input_source(c["src"]); m.set_input_target(c["q"], c["n"])
        with pytest.raises(smhip.SmhipError) as e:
            m.align()
        assert e.value.status == 1
        m.set_inner_compensation(False)
        ok, R = m.align()                                 # nothing was touched: the rigid Align runs
        assert ok
        m.close()


def test_cpp_interface_flag_and_mode(tmp_path, smhip, velo20k):
    """registrator.h: inner_compensation_mode 0 + EnableInnerCompensation() is refused as ever, mode 1 runs the compensated
    iteration, and the same matcher with the flag off aligns rigidly bit for bit."""
    from staticmapping_amd import build
    lib = build.build()
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "test_inner_compensation")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_inner_compensation.cc")
    deps = [src, lib, os.path.join(ROOT, "include", "smhip", "registrator.h"), os.path.join(ROOT, "include", "smhip.h")]
    if (not os.path.exists(exe)) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                               "-L", os.path.dirname(lib), "-lsmhip", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"])
    c = velo20k
    tgt_bin, src_bin = tmp_path / "t.bin", tmp_path / "s.bin"
    c["tgt"].astype(np.float32).tofile(tgt_bin)
    c["src"].astype(np.float32).tofile(src_bin)
    out = subprocess.check_output([exe, str(tgt_bin), str(src_bin), "0.6"], text=True, timeout=300)
    res = json.loads(out.strip().splitlines()[-1])
    assert res["rigid_ok"] and res["refused_in_mode_0"] and res["mode_0_off_runs"]
    assert res["compensated_ok"] and res["mode_1_off_is_rigid"]
    q, n = smhip.calculate_normals(c["tgt"][:, :3].astype(np.float64))
    R_o, score_o, _ = cr.icp_fast_align_compensated(_src64(c), q, n, guess=c["guess"], max_iteration=20)
    Rc = np.array(res["compensated"]).reshape(4, 4)
    da, dt = smhip.se3_error(Rc, R_o)
    assert da < ROT_TOL and dt < TRANS_TOL, (da, dt)
    assert abs(res["compensated_score"] - score_o) < 1e-3          # (the bound tests/test_cpp_interface.py uses for this path's score)
    assert smhip.se3_error(Rc, np.array(res["rigid"]).reshape(4, 4))[1] > 10 * TRANS_TOL
