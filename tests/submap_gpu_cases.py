"""The GPU cases of tests/test_submap_gpu.py, one per process: `python tests/submap_gpu_cases.py CASE`.  Every case prints its
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
import submap_ref as sr
from test_submap_cpp import _build_exe as build_cpp      # tests/cpp/test_submap.cc against the built library
from staticmapping_amd import _capi, synth
from staticmapping_amd import filters as df
from staticmapping_amd import submap as dsub

def _status_codes():
    import re
    txt = open(os.path.join(ROOT, "include", "smhip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"(SMHIP_[A-Z_]+)\s*=\s*(-?\d+)", txt)}


def drive(n_scans, n_points):
    """The straight drive of tests/test_back_end_gpu.py::_submaps: world poses and the scans taken there."""
    scene = synth.make_scene(0)
    poses = [synth.make_pose(t=(0.8 * k, 0.03 * k, 0.0), rpy_deg=(0, 0, 0.6 * k)) for k in range(n_scans)]
    scans = [synth.velodyne_scan(scene, P, seed=90 + k, n_points=n_points) for k, P in enumerate(poses)]
    return poses, scans


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_cloud(m, label, frames, poses, voxel, composition=True):
    got, gsrc = dsub.build_submap(m, frames, poses, voxel)
    want, wsrc = sr.build_submap(frames, poses, voxel)
    same = bits_equal(got, want) and np.array_equal(gsrc, wsrc)
    print(f"{label}: device {got.shape} restatement {want.shape} bit-equal {same}")
    assert same, label
    if composition:
        # what could be done before: TransformPoint on the host, then smhip_filter_chain_f32([VoxelGrid]) on the rows
        rows5 = sr.concatenate(frames, poses)
        chain = [df.make_filter("VoxelGrid", voxel_size=voxel)] if voxel > 0 else []
        comp, csrc = df.run_chain(m, rows5, chain)
        same = bits_equal(got, comp) and np.array_equal(gsrc, csrc)
        print(f"{label}: equals host transform + filter chain: {same}")
        assert same, label + " (composition)"
    return got, gsrc


def case_cloud():
    poses, scans = drive(3, 20_000)
    local = sr.local_poses(poses)
    size = sr.text_voxel_size(0.1)
    m = sm.IcpFastHip(pair_slots=1, max_source_points=131072, max_target_points=131072)
    check_cloud(m, "3 x 20000 stride 4 voxel 0.1", scans, local, size)
    check_cloud(m, "3 x 20000 stride 4 voxel 0", scans, local, 0.0)
    rng = np.random.default_rng(5)
    scans5 = [np.concatenate([s, rng.uniform(0, 1, (len(s), 1)).astype(np.float32)], axis=1) for s in scans]
    check_cloud(m, "3 x 20000 stride 5 voxel 0.1", scans5, local, size)
    check_cloud(m, "3 x 20000 stride 5 voxel 0", scans5, local, 0.0)
    # unequal frames, one of them empty (first, middle and last position of the empty frame)
    for order in ([0, 1, 2], [1, 0, 2], [1, 2, 0]):
        parts = [scans[0][:0], scans[1][:7001], scans[2][:333]]
        frames = [parts[k] for k in order]
        check_cloud(m, f"unequal frames {[len(f) for f in frames]} stride 4 voxel 0.1", frames, local, size)
        check_cloud(m, f"unequal frames {[len(f) for f in frames]} stride 4 voxel 0", frames, local, 0.0)
    frames5 = [scans5[0][:12345], scans5[1][:0], scans5[2]]
    check_cloud(m, "unequal frames stride 5 voxel 0.1", frames5, local, size)
    m.close()


def case_big():
    poses, scans = drive(5, 120_000)
    local = sr.local_poses(poses)
    m = sm.IcpFastHip(pair_slots=1, max_source_points=131072, max_target_points=1 << 20)
    check_cloud(m, "5 x 120000 stride 4 voxel 0.1", scans, local, sr.text_voxel_size(0.1))
    m.close()


def case_handover():
    poses, scans = drive(3, 20_000)
    local = sr.local_poses(poses)
    size = sr.text_voxel_size(0.1)
    m = sm.IcpFastHip(pair_slots=2, max_source_points=131072, max_target_points=131072)
    for voxel in (size, 0.0):
        cloud, _ = dsub.build_submap(m, scans, local, voxel)
        n_t = dsub.output_to_target(m, 0)
        p0, n0 = m.get_target(n_t, 0)
        n_ref = m.prepare_target(cloud, slot=1)                     # smhip_prepare_target_f32 on the downloaded rows
        p1, n1 = m.get_target(n_ref, 1)
        same = n_t == n_ref and bits_equal(p0, p1) and bits_equal(n0, n1)
        print(f"voxel {voxel}: output_to_target n = {n_t}, prepare_target n = {n_ref}, points and normals bit-equal {same}")
        assert same
        # the cloud is still resident after the target was made: to a source slot, and back
        n = dsub.build_submap_resident(m, scans, local, voxel)
        dsub.output_to_source(m, 1)
        p_dev, idx = m.get_source(1)
        same = len(idx) == n == len(cloud) and np.array_equal(np.sort(idx), np.arange(n)) and bits_equal(p_dev, cloud[idx, :3])
        print(f"voxel {voxel}: output_to_source + get_source returns the {n} rows: {same}")
        assert same
    # the builder's device form: same target as the functions above
    b = sm.SubmapBuilder(frame_count=3, enable_voxel_filter=True, voxel_size=0.1)
    for s, P in zip(scans, poses):
        b.insert_frame(s, P)
    n_b = b.to_target(m, 0)
    pb, nb = m.get_target(n_b, 0)
    dsub.build_submap_resident(m, scans, local, size)
    n_f = dsub.output_to_target(m, 1)
    pf, nf = m.get_target(n_f, 1)
    assert n_b == n_f and bits_equal(pb, pf) and bits_equal(nb, nf)
    m.close()
    # no cloud resident: NOT_READY
    codes = _status_codes()
    m = sm.IcpFastHip(pair_slots=1, max_source_points=4096, max_target_points=4096)
    out = ctypes.c_int()
    st = m._lib.smhip_filter_output_to_target(m._h, 0, ctypes.byref(out))
    print("output_to_target on a fresh handle:", st)
    assert st == codes["SMHIP_ERR_NOT_READY"]
    m.close()


def case_refusals():
    codes = _status_codes()
    inv, cap = codes["SMHIP_ERR_INVALID_ARGUMENT"], codes["SMHIP_ERR_CAPACITY"]
    rng = np.random.default_rng(11)
    frames = [rng.uniform(-30, 30, (n, 4)).astype(np.float32) for n in (500, 700)]
    local = [np.eye(4), synth.make_pose(t=(1.0, 0.2, 0.0), rpy_deg=(0, 0, 3.0))]
    m = sm.IcpFastHip(pair_slots=1, max_source_points=2048, max_target_points=4096)
    kept, ksrc = dsub.build_submap(m, frames, local, 0.5)
    want, _ = sr.build_submap(frames, local, 0.5)
    assert bits_equal(kept, want)

    lib, h = m._lib, m._h
    rows = (_capi.c_float_p * 2)(*[f.ctypes.data_as(_capi.c_float_p) for f in frames])
    n = np.array([500, 700], np.int32)
    zero = np.array([0, 0], np.int32)
    poses = np.ascontiguousarray([P.T.reshape(16) for P in local]).reshape(-1)
    np_ = n.ctypes.data_as(_capi.c_int32_p)
    pp = poses.ctypes.data_as(_capi.c_double_p)
    big = [rng.uniform(-30, 30, (3000, 4)).astype(np.float32), rng.uniform(-30, 30, (1097, 4)).astype(np.float32)]
    big_rows = (_capi.c_float_p * 2)(*[f.ctypes.data_as(_capi.c_float_p) for f in big])
    big_n = np.array([3000, 1097], np.int32)
    out = ctypes.c_int(-7)
    calls = {
        "n_frames 0": (inv, lambda: lib.smhip_submap_build_f32(h, 0, rows, 4, np_, pp, 0.5, ctypes.byref(out))),
        "n_frames -1": (inv, lambda: lib.smhip_submap_build_f32(h, -1, rows, 4, np_, pp, 0.5, ctypes.byref(out))),
        "null rows table": (inv, lambda: lib.smhip_submap_build_f32(h, 2, None, 4, np_, pp, 0.5, ctypes.byref(out))),
        "null size table": (inv, lambda: lib.smhip_submap_build_f32(h, 2, rows, 4, None, pp, 0.5, ctypes.byref(out))),
        "null pose table": (inv, lambda: lib.smhip_submap_build_f32(h, 2, rows, 4, np_, None, 0.5, ctypes.byref(out))),
        "stride 3": (inv, lambda: lib.smhip_submap_build_f32(h, 2, rows, 3, np_, pp, 0.5, ctypes.byref(out))),
        "stride 6": (inv, lambda: lib.smhip_submap_build_f32(h, 2, rows, 6, np_, pp, 0.5, ctypes.byref(out))),
        "voxel -0.1": (inv, lambda: lib.smhip_submap_build_f32(h, 2, rows, 4, np_, pp, -0.1, ctypes.byref(out))),
        "voxel nan": (inv, lambda: lib.smhip_submap_build_f32(h, 2, rows, 4, np_, pp, float("nan"), ctypes.byref(out))),
        "voxel inf": (inv, lambda: lib.smhip_submap_build_f32(h, 2, rows, 4, np_, pp, float("inf"), ctypes.byref(out))),
        "every frame empty": (inv, lambda: lib.smhip_submap_build_f32(h, 2, rows, 4, zero.ctypes.data_as(_capi.c_int32_p), pp, 0.5, ctypes.byref(out))),
        "4097 rows on a 4096 handle": (cap, lambda: lib.smhip_submap_build_f32(h, 2, big_rows, 4, big_n.ctypes.data_as(_capi.c_int32_p), pp, 0.5,
                                                                             ctypes.byref(out))),
    }
    for label, (want_status, call) in calls.items():
        st = call()
        msg = lib.smhip_last_error(h).decode()
        after, asrc = dsub.get_submap(m, len(kept))
        print(f"{label}: status {st} ({msg!r}), resident cloud unchanged {bits_equal(after, kept)}")
        assert st == want_status, label
        assert msg, label
        assert bits_equal(after, kept) and np.array_equal(asrc, ksrc), label
    # exactly the capacity is taken
    big_n[1] = 1096
    assert lib.smhip_submap_build_f32(h, 2, big_rows, 4, big_n.ctypes.data_as(_capi.c_int32_p), pp, 0.0, ctypes.byref(out)) == 0
    assert out.value == 4096
    m.close()


def oracle_align(src_cloud, tgt_cloud, guess):
    from oracle import cref
    q, nrm, _ = cref.calculate_normals(tgt_cloud[:, :3].astype(np.float64))
    fin = np.isfinite(nrm).all(axis=1)
    return cref.icp_fast_align(src_cloud[:, :3].astype(np.float64), q[fin], nrm[fin], guess=guess, nthreads=cref.usable_cores())


def case_matching():
    import json
    import subprocess
    import tempfile
    from staticmapping_amd import kitti
    poses, scans = drive(6, 20_000)
    size = sr.text_voxel_size(0.1)
    truth = np.linalg.inv(poses[0]) @ poses[3]                     # source submap frame -> target submap frame
    # the global poses as the callers see them: the second submap's frames moved by 0.25 m / 0.05 m (poses[0] is the identity, so
    # the shift is the same in the target submap's frame; a common shift leaves the frames' local poses as they are)
    shift = np.eye(4)
    shift[0, 3], shift[1, 3] = -0.25, 0.05
    seen = poses[:3] + [shift @ P for P in poses[3:]]
    guess = np.linalg.inv(seen[0]) @ seen[3]
    assert np.allclose(guess[:3, :3], truth[:3, :3], atol=1e-15) and np.allclose(guess[:3, 3] - truth[:3, 3], [-0.25, 0.05, 0.0], atol=1e-12)
    m = sm.IcpFastHip(pair_slots=1, max_source_points=131072, max_target_points=131072)
    tb, sb = sm.SubmapBuilder(3, True, 0.1), sm.SubmapBuilder(3, True, 0.1)
    for k in range(3):
        tb.insert_frame(scans[k], seen[k]); sb.insert_frame(scans[3 + k], seen[3 + k])
    tb.to_target(m, 0)
    sb.to_source(m, 0)
    _, R = m.align(guess)
    score = m.get_fitness_score()
    tgt, _ = sr.build_submap(scans[:3], sr.local_poses(seen[:3]), size)
    src, _ = sr.build_submap(scans[3:], sr.local_poses(seen[3:]), size)
    ref = oracle_align(src, tgt, guess)
    da, dt = sm.se3_error(R, ref["result"])
    oa, ot = sm.se3_error(ref["result"], truth)
    print(f"device: score {score:.6f} iterations {m.last_stats[0]['iterations']}; oracle: score {ref['score']:.6f} iterations "
          f"{ref['iterations']} ({oa:.2e} rad / {ot:.2e} m from the truth); device vs oracle {da:.2e} rad / {dt:.2e} m, "
          f"score {abs(score - ref['score']):.2e}")
    assert da < 1e-4 and dt < 1e-3 and abs(score - ref["score"]) < 1e-4, (da, dt, score, ref["score"])

    # ---- the same pair through C++ Submap and ConnectSubmaps.  ConnectSubmaps hands SubmapPairMatchBatch the submaps' Cloud():
    # the device-built cloud downloaded, then the host CalculateNormals on it -- for the source too, as Submap::Cloud() gives
    # (submap.cc:160-161) -- and IcpFast as a batch of one.  The Python path below does the same with the package's calls.
    with tempfile.TemporaryDirectory() as d:
        for k, s in enumerate(scans):
            kitti.write_bin(os.path.join(d, "%06d.bin" % k), s)
        np.savetxt(os.path.join(d, "poses.txt"), np.stack(seen).reshape(6, 16), fmt="%.17g")
        out = subprocess.run([build_cpp(), "match", d, "6", "3", "20000", "0.1"], capture_output=True, text=True, timeout=300)
    print(out.stderr[-2000:])
    assert out.returncode == 0, out.returncode
    res = json.loads(out.stdout.strip().splitlines()[-1])
    M = lambda key: np.array(res[key]).reshape(4, 4)
    tc, _ = tb.cloud(m)
    sc, _ = sb.cloud(m)
    assert res["pairs"] == 1 and res["cloud0"] == len(tc) and res["cloud1"] == len(sc)
    qs, _ = sm.calculate_normals(sc[:, :3])
    qt, nt = sm.calculate_normals(tc[:, :3])
    m.set_input_source(qs)
    m.set_input_target(qt, nt)
    Rs, scores, _ = m.align_batch(1, [guess])
    da, dt = sm.se3_error(M("transform0"), Rs[0])
    dg = np.abs(M("guess0") - guess).max()
    print(f"C++ ConnectSubmaps vs the Python path: {da:.2e} rad / {dt:.2e} m, score {abs(res['score0'] - scores[0]):.2e}, guess {dg:.2e}; "
          f"accepted {res['accepted0']} score {res['score0']:.6f}")
    assert da < 1e-9 and dt < 1e-9 and abs(res["score0"] - scores[0]) < 1e-9 and dg < 1e-12
    assert res["accepted0"] and res["score0"] >= 0.7
    da, dt = sm.se3_error(M("transform0"), truth)
    assert da < 3e-3 and dt < 5e-2, (da, dt)
    # the C++ device forms (ToTarget / ToSource, no download) against the Python device path above
    da, dt = sm.se3_error(M("resident_transform"), R)
    print(f"C++ ToTarget / ToSource vs Python to_target / to_source: {da:.2e} rad / {dt:.2e} m, score {abs(res['resident_score'] - score):.2e}")
    assert res["resident_ok"] and res["resident_ns"] == len(sc) and da < 1e-7 and dt < 1e-6 and abs(res["resident_score"] - score) < 1e-7
    m.close()


def read_edges(path):
    rows = np.loadtxt(path, dtype=np.float64, ndmin=2)
    assert rows.size == 0 or rows.shape[1] == 16, rows.shape
    out = []
    for r in rows:
        T = np.eye(4)
        T[:3, :] = r[4:].reshape(3, 4)
        out.append(dict(a=int(r[0]), b=int(r[1]), accepted=int(r[2]), score=float(r[3]), transform=T))
    return out


def case_driver():
    """smhip_shard --submap-edges on 12 and 13 generated scans (three edges each, the 13th scan a group that is not full) and on
    11 (three full groups: the first two of those edges)."""
    import json
    import subprocess
    import tempfile
    import driver_ref as dr
    from staticmapping_amd import build, kitti
    from oracle import cref
    exe = build.build_shard_driver()
    world = dr.drive_truth()
    scene = synth.make_drive_scene(world, seed=5)
    scans = [synth.velodyne_scan(synth.scene_near(scene, P[:3, 3]), P, seed=1000 + k, n_points=40_000) for k, P in enumerate(world[:13])]
    size = sr.text_voxel_size(0.1)
    edges = {}
    with tempfile.TemporaryDirectory() as d:
        # 12 scans with the driver's default batch: the run that is compared with the oracle.  Then 12, 13 and 11 scans with
        # --batch 1, where every pair is aligned on its own whatever the directory holds: the pose files agree line for line, so
        # the edge files can be compared as text
        for count, extra in ((12, []), (12, ["--batch", "1"]), (13, ["--batch", "1"]), (11, ["--batch", "1"])):
            sd = os.path.join(d, "scans%d" % count)
            if not os.path.isdir(sd):
                os.makedirs(sd)
                for k in range(count):
                    kitti.write_bin(kitti.scan_path(sd, k), scans[k])
            tag = "%d%s" % (count, "b1" if extra else "")
            pose_file, edge_file = os.path.join(d, "pose%s.txt" % tag), os.path.join(d, "edges%s.txt" % tag)
            cmd = [exe, "--scans", sd, "--gpus", "1", "--guess-tx", str(dr.GUESS_TX), "--iterations", "20", "--out", pose_file,
                   "--submap-frames", "3", "--submap-voxel", "0.1", "--submap-edges", edge_file] + extra
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            print(r.stderr[-2000:])
            assert r.returncode == 0, (" ".join(cmd), r.returncode)
            line = json.loads(r.stdout.strip().splitlines()[-1])
            print(tag, {k: v for k, v in line.items() if k.startswith("submap")})
            edges[tag] = (read_edges(edge_file), open(edge_file).read(), dr.read_chain(pose_file), line, open(pose_file).read())
    got, _, poses, line, _ = edges["12"]
    assert len(got) == 3 and line["submaps"] == 4 and line["submap_edges"] == 3
    assert [(e["a"], e["b"]) for e in got] == [(0, 1), (1, 2), (2, 3)]
    # every edge against the oracle on submaps restated from the pose file AS WRITTEN
    clouds = []
    for k in range(4):
        # (the arrays are the files' content: float32 rows written as they are)
        frames = [np.ascontiguousarray(scans[f][:, :4], dtype=np.float32) for f in range(3 * k, 3 * k + 3)]
        clouds.append(sr.build_submap(frames, sr.local_poses(list(poses[3 * k:3 * k + 3])), size)[0])
    for e in got:
        k = e["a"]
        guess = np.linalg.inv(poses[3 * k]) @ poses[3 * (k + 1)]
        q, nrm, _ = cref.calculate_normals(clouds[k][:, :3].astype(np.float64))
        fin = np.isfinite(nrm).all(axis=1)
        ref = cref.icp_fast_align(clouds[k + 1][:, :3].astype(np.float64), q[fin], nrm[fin], guess=guess, max_iteration=20, early_exit=False,
                                  nthreads=cref.usable_cores())
        want = ref["result"] if ref["score"] >= 0.7 else guess
        # what the file's 8 significant digits can move (tests/driver_ref.py::half_unit_8g)
        p_rot = float(np.sqrt((dr.half_unit_8g(e["transform"][:3, :3]) ** 2).sum()))
        p_t = float(np.sqrt((dr.half_unit_8g(e["transform"][:3, 3]) ** 2).sum()))
        p_s = float(dr.half_unit_8g(e["score"]))
        da, dt = dr.se3_error(e["transform"], want)
        print(f"edge {e['a']} -> {e['b']}: accepted {e['accepted']} score {e['score']:.8g} (oracle {ref['score']:.8g}, {ref['iterations']} iterations); "
              f"vs oracle {da:.2e} rad / {dt:.2e} m; printed precision {p_rot:.1e} rad / {p_t:.1e} m / {p_s:.1e}")
        assert da < 1e-4 + p_rot and dt < 1e-3 + p_t and abs(e["score"] - ref["score"]) < 1e-4 + p_s, (e, da, dt, ref["score"])
        assert e["accepted"] == int(e["score"] >= 0.7)
        if not e["accepted"]:
            da, dt = dr.se3_error(e["transform"], guess)
            assert da < p_rot * 1.01 + 1e-12 and dt < p_t * 1.01 + 1e-12
    # a trailing group that is not full is dropped: 13 scans give the same three edges, 11 scans (three full groups) the first two
    text = edges["12b1"][1]
    assert len(edges["12b1"][0]) == 3 and edges["12b1"][3]["submaps"] == 4
    assert edges["13b1"][4].splitlines()[:12] == edges["12b1"][4].splitlines() and edges["11b1"][4].splitlines() == edges["12b1"][4].splitlines()[:11]
    assert edges["13b1"][3]["submaps"] == 4 and edges["13b1"][1] == text
    assert edges["11b1"][3]["submaps"] == 3 and edges["11b1"][1] == "".join(text.splitlines(keepends=True)[:2])


CASES = {"cloud": case_cloud, "big": case_big, "handover": case_handover, "refusals": case_refusals, "matching": case_matching, "driver": case_driver}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print("ok", sys.argv[1])
