"""Row N1: CalculateNormals on the device (csrc/prep_normals.hip) vs the ORACLE (oracle/csrc/smref_icp.c,
builder/data/cloud_types.cc:73-144, 347-368); the host implementation is checked against the same oracle in
tests/test_calculate_normals.py."""
import time

import numpy as np
import pytest

import normals_ref as nr

pytestmark = pytest.mark.gpu


def _match_sets(p_dev, n_dev, p_host, n_host):
    from scipy.spatial import cKDTree
    d, i = cKDTree(p_host).query(p_dev)
    return d, n_host[i]


@pytest.mark.parametrize("n_points", [20_000, 120_000])
def test_device_calculate_normals_matches_oracle(n_points):
    import staticmapping_amd as sm
    from staticmapping_amd import synth
    from oracle import cref
    a, b, T = synth.scan_pair("cfg2", n_points=n_points)
    # ties in a coordinate make nth_element's partition implementation-defined: break them like the oracle tests do
    a = a.copy()
    a[:, :3] += np.random.default_rng(0).normal(0, 2e-5, (n_points, 3)).astype(np.float32)
    q, n, _ = cref.calculate_normals(a[:, :3].astype(np.float64))
    ok = np.isfinite(n).all(axis=1)
    q, n = q[ok], n[ok]
    m = sm.IcpFastHip(max_source_points=n_points, max_target_points=n_points // 4 + 64)
    t0 = time.time()
    M = m.prepare_target(a)
    dt = time.time() - t0
    p_dev, n_dev = m.get_target(M)
    assert abs(M - len(q)) <= 2                               # same leaves (dropped singular leaves may differ by rounding)
    d, n_ref = _match_sets(p_dev.astype(np.float64), n_dev, q, n)
    assert (d < 1e-4).mean() > 0.995                          # same kd-box partition -> same leaf means (float32 storage)
    good = d < 1e-4
    # the unconstrained-LS normal is ill-conditioned on near-collinear leaves; the bulk must agree
    agree = np.abs(n_dev[good] - n_ref[good]).max(axis=1) < 1e-2
    assert agree.mean() > 0.97
    # and leaf by leaf against the exact reference: membership, bit-equal means, normals within the measured spread
    print(nr.compare(nr.LeafReference(a[:, :3]), p_dev, n_dev))
    print(f"device CalculateNormals {n_points} pts -> {M}: {dt*1e3:.1f} ms (first call, incl. workspace allocation)")
    m.close()


def test_prepared_target_aligns_like_host_prepared(velo20k):
    """End to end: target prepared on the device from the source slot of the previous pair."""
    import staticmapping_amd as sm
    c = velo20k
    m = sm.IcpFastHip(pair_slots=2, max_source_points=len(c["src"]), max_target_points=len(c["src"]) // 4 + 64)
    m.set_input_source(c["tgt"], slot=1)                      # the older scan sits in a source slot ...
    M = m.prepare_target_from_source(1, 0)                    # ... and becomes slot 0's target without a second upload
    m.set_input_source(c["src"], slot=0)
    ok, R_dev = m.align(c["guess"])
    q, n = sm.calculate_normals(c["tgt"][:, :3].astype(np.float64))
    m.set_input_target(q, n, slot=0)
    ok, R_host = m.align(c["guess"])
    da, dt = sm.se3_error(R_dev, R_host)
    assert da < 2e-4 and dt < 2e-3, (da, dt)                  # ties may move a few leaves; the alignment does not care
    da, dt = sm.se3_error(R_dev, c["T"])
    assert da < 2e-3 and dt < 2e-2
    m.close()


def test_batched_preparation_equals_single_calls(velo20k, cfg2):
    """One kd forest for several scans gives exactly what the scans give one at a time."""
    import staticmapping_amd as sm
    scans = [velo20k["tgt"], cfg2["tgt"][:60000], velo20k["src"]]
    cap = max(len(s) for s in scans)
    m = sm.IcpFastHip(pair_slots=6, max_source_points=cap, max_target_points=cap // 4 + 64)
    single = []
    for k, sc in enumerate(scans):
        m.set_input_source(sc, slot=k)
        M = m.prepare_target_from_source(k, k)
        single.append(m.get_target(M, slot=k))
    Ms = m.prepare_targets_from_sources([0, 1, 2], [3, 4, 5])
    for k in range(3):
        p1, n1 = single[k]
        assert Ms[k] == len(p1)
        p2, n2 = m.get_target(int(Ms[k]), slot=3 + k)
        assert np.array_equal(p1, p2) and np.array_equal(n1, n2)
    m.close()


def test_large_batch_forest_equals_single_calls_and_the_oracle(cfg2, capsys):
    """From 32 scans on a batch is prepared by the one-workgroup-per-scan forest (radix select + partition per level,
    kd_median_tree.h) instead of the sort-per-level one: on tie-free scans both give the same leaves as each other and as the
    oracle (cloud_types.cc:105-144), scan by scan, for scans of different sizes."""
    import time
    import staticmapping_amd as sm
    from oracle import cref
    rng = np.random.default_rng(7)
    base = cfg2["tgt"]
    scans = []
    for k in range(32):
        n = 20_000 + 1_250 * k                                   # 20 000 .. 58 750 points
        sc = base[rng.choice(len(base), size=n, replace=False)].copy()
        sc[:, :3] += rng.normal(0, 2e-5, (n, 3)).astype(np.float32)     # no ties on a cut coordinate
        sc[:, 0] += 0.37 * k
        scans.append(np.ascontiguousarray(sc))
    cap = max(len(s) for s in scans)
    m = sm.IcpFastHip(pair_slots=64, max_source_points=cap, max_target_points=cap // 4 + 64)
    for k, sc in enumerate(scans):
        m.set_input_source(sc, slot=k)
    m.prepare_targets_from_sources(list(range(32)), list(range(32, 64)))       # first call: workspace allocation
    m.synchronize()
    t0 = time.perf_counter()
    Ms = m.prepare_targets_from_sources(list(range(32)), list(range(32, 64)))
    dt = time.perf_counter() - t0

    def canon(p, nrm):
        o = np.lexsort((p[:, 2], p[:, 1], p[:, 0]))
        return p[o], nrm[o]
    for k in (0, 13, 31):
        pb, nb = canon(*m.get_target(int(Ms[k]), slot=32 + k))
        M1 = m.prepare_target_from_source(k, k)                                # the sort-per-level form (one scan)
        p1, n1 = canon(*m.get_target(M1, slot=k))
        assert M1 == Ms[k]
        assert np.abs(pb - p1).max() < 1e-5
        well = np.abs(nb - n1).max(axis=1) < 1e-3                              # ill-conditioned leaves aside (unconstrained LS normal)
        assert well.mean() > 0.995
    q, n, _ = cref.calculate_normals(scans[31][:, :3].astype(np.float64))
    ok = np.isfinite(n).all(axis=1)
    pb, nb = m.get_target(int(Ms[31]), slot=63)
    assert abs(len(pb) - ok.sum()) <= 2
    d, _ = _match_sets(pb.astype(np.float64), nb, q[ok], n[ok])
    assert (d < 1e-4).mean() > 0.995
    p_res, _ = m.get_source(31)                                                # the scan in the order the forest indexed it
    nr.compare(nr.LeafReference(p_res), pb, nb)
    with capsys.disabled():
        print(f"\n[forest] 32 scans ({sum(len(s) for s in scans)} points) prepared in {dt * 1e3:.2f} ms = {dt * 1e3 / 32:.3f} ms per scan")
    m.close()


def test_tied_coordinates_give_the_same_leaves_in_every_batch_size(cfg2):
    """Real scans carry tied coordinates (KITTI's are quantised), and std::nth_element leaves open which of the points ON a
    median go left.  Both builders break such ties by point index -- the forest (batches of >= 32 scans) in its select, the
    sort-per-level form by putting a tie run that straddles a split in index order -- so a scan's target points and normals do
    not depend on the size of the batch it was prepared in: here scans quantised to 2 cm (thousands of ties per cut) prepared
    in a batch of 32 against the same scans one at a time, bit for bit."""
    import staticmapping_amd as sm
    rng = np.random.default_rng(11)
    base = cfg2["tgt"]
    scans = []
    for k in range(32):
        n = 15_000 + 700 * k
        sc = base[rng.choice(len(base), size=n, replace=False)].copy()
        sc[:, :3] = np.round(sc[:, :3] / 0.02) * 0.02
        scans.append(np.ascontiguousarray(sc.astype(np.float32)))
    cap = max(len(s) for s in scans)
    m = sm.IcpFastHip(pair_slots=64, max_source_points=cap, max_target_points=cap // 4 + 64)
    for k, sc in enumerate(scans):
        m.set_input_source(sc, slot=k)
    Ms = m.prepare_targets_from_sources(list(range(32)), list(range(32, 64)))

    def canon(p, nrm):
        o = np.lexsort((nrm[:, 2], nrm[:, 1], nrm[:, 0], p[:, 2], p[:, 1], p[:, 0]))
        return p[o], nrm[o]
    ties = 0
    for k in (0, 7, 19, 31):
        pb, nb = canon(*m.get_target(int(Ms[k]), slot=32 + k))
        M1 = m.prepare_target_from_source(k, k)                                # the sort-per-level form (one scan)
        p1, n1 = canon(*m.get_target(M1, slot=k))
        assert M1 == Ms[k]
        assert np.array_equal(pb, p1) and np.array_equal(nb, n1), (k, int((pb != p1).any(axis=1).sum()), int((nb != n1).any(axis=1).sum()))
        ties += len(scans[k]) - len(np.unique(scans[k][:, 0]))
    assert ties > 10_000                                                       # the scans did carry ties
    m.close()
