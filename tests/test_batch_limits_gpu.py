"""Ndt and NdtWithGicp lock-step batches across the host's fixed-size splits, against single calls and the oracle.

The batch entry points split their work into pieces of fixed size, and each split is a place where a per-job offset, a prefix or a
key width can go wrong:
  - NdtWithGicp: from 4 jobs target covariances are estimated on demand; gicp_need / gicp_corr / gicp_fdf carry 16 jobs per launch,
    gicp_knn_cov 32 clouds; the batched ApproximateVoxelGrid takes 64 clouds per pass (a batch of K jobs filters up to 2 K clouds).
  - Ndt: the voxel sort key grows with K and with the batch's largest target; the fitness grids shrink per pair as K grows.
Every batch here crosses some of them, with jobs that all differ in size and guess.  Each job must return the bits of a single Align of
the same pair on a handle of its own (rebuilt, and again with the targets kept), and what can be recomputed independently is: the
down-sampled sizes (oracle/ndt_gicp.py's filter), the GICP fitness (float64 k-d tree over the oracle's clouds), the occupied NDT voxels
(oracle/ndt.py's grid) and the NDT fitness score (float64 brute force over the raw target).
"""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import staticmapping_amd as sm
from staticmapping_amd import synth
from oracle import ndt as ondt
from oracle import ndt_gicp as ong

pytestmark = pytest.mark.gpu

N_PAIRS = 65
GICP_FIELDS = ("ok", "n_source", "n_target", "ndt_iterations", "gicp_iterations", "gicp_function_evaluations",
               "gicp_correspondences", "ndt_score", "gicp_score")
GICP_REJECTED = 43                               # its guess is far off: NDT's fitness ends above 1, the job returns the guess
                                                 # (from its own guess this pair's NDT stage would end at 1.24 and be rejected too)
FAR = synth.make_pose(t=(60.0, -45.0, 3.0))


@pytest.fixture(scope="module")
def scenes():
    return [synth.scan_pair("cfg2", n_points=12000 + 800 * s, scene_seed=s) for s in range(10)]


def _derived(scenes, p):
    """Pair p: scene p % 10, strided and truncated by p so that no two pairs share a source size or a target size."""
    a, b, T = scenes[p % 10]
    v = p // 10
    src = b[(v % 2)::1 + v % 3, :3]
    tgt = a[((v + 1) % 2)::1 + (v + 1) % 3, :3]
    src, tgt = src[:len(src) - 7 * p], tgt[:len(tgt) - 11 * p]
    return np.ascontiguousarray(src), np.ascontiguousarray(tgt), T


def _distinct_sizes(pairs):
    assert len({len(p[0]) for p in pairs}) == len(pairs) and len({len(p[1]) for p in pairs}) == len(pairs)


# ---- NdtWithGicp -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gicp_pairs(scenes):
    pairs = []
    for p in range(N_PAIRS):
        src, tgt, T = _derived(scenes, p)
        G = T @ synth.make_pose(t=(0.04 * ((p % 3) - 1) - 0.2, 0.03 + 0.01 * (p % 5), 0.0), rpy_deg=(0, 0, 0.2 * ((p % 4) - 1.5)))
        pairs.append((src, tgt, FAR if p == GICP_REJECTED else G))
    _distinct_sizes(pairs)
    return pairs


def _gicp_caps(pairs):
    return dict(max_source_points=max(len(p[0]) for p in pairs), max_target_points=max(len(p[1]) for p in pairs))


def _gicp_single(pairs, n, **options):
    m = sm.NdtGicpHip(**_gicp_caps(pairs), **options)
    out = []
    for src, tgt, G in pairs[:n]:
        m.set_input_source(src); m.set_input_target(tgt)
        ok, R = m.align(G)
        out.append((R, m.get_fitness_score(), dict(m.last_gicp_stats)))
    m.close()
    return out


@pytest.fixture(scope="module")
def gicp_single_on(gicp_pairs):
    return _gicp_single(gicp_pairs, N_PAIRS)


@pytest.fixture(scope="module")
def gicp_single_off(gicp_pairs):
    return _gicp_single(gicp_pairs, 33, using_voxel_filter=0)


class _GicpOracle:
    """The clouds GICP sees (the oracle's ApproximateVoxelGrid(0.2), or the raw clouds) and the fitness over them."""

    def __init__(self, pairs, filt):
        self.pairs, self.filt, self.clouds = pairs, filt, {}

    def clouds_of(self, p):
        if p not in self.clouds:
            src, tgt, _ = self.pairs[p]
            if self.filt:
                src, tgt = ong.approximate_voxel_grid(src, 0.2), ong.approximate_voxel_grid(tgt, 0.2)
            self.clouds[p] = (src, tgt, cKDTree(tgt.astype(np.float64)))
        return self.clouds[p]

    def check(self, p, R, score, st, what):
        src, tgt, tree = self.clouds_of(p)
        assert st["n_source"] == len(src) and st["n_target"] == len(tgt), (what, p, st["n_source"], len(src), st["n_target"], len(tgt))
        if not st["ok"]:
            return
        # oracle/ndt_gicp.py gicp_align's score: the source moved by the float pose, float squared 1-NN distances, averaged in double
        Rf = R.astype(np.float32)
        moved = (np.concatenate([src, np.ones((len(src), 1), np.float32)], axis=1) @ Rf.T).astype(np.float32)[:, :3]
        d, _ = tree.query(moved.astype(np.float64))
        want = float((d.astype(np.float32) ** 2).astype(np.float64).mean())
        assert abs(st["gicp_score"] - want) <= 2e-5 * want + 1e-9, (what, p, st["gicp_score"], want)
        assert abs(score - np.exp(-st["gicp_score"])) <= 1e-15 * score, (what, p, score, st["gicp_score"])


@pytest.fixture(scope="module")
def gicp_oracle(gicp_pairs):
    return {1: _GicpOracle(gicp_pairs, True), 0: _GicpOracle(gicp_pairs, False)}


def test_ndt_gicp_single_calls_match_the_oracle(gicp_pairs, gicp_single_on, gicp_single_off, gicp_oracle):
    """The references of the batches below: every single call against the oracle's down-sampled sizes and fitness."""
    for filt, single in ((1, gicp_single_on), (0, gicp_single_off)):
        for p, (R, score, st) in enumerate(single):
            gicp_oracle[filt].check(p, R, score, st, f"single, filter {filt}")
            assert st["ok"] == (p != GICP_REJECTED), (filt, p, st)
    R, score, st = gicp_single_on[GICP_REJECTED]
    assert np.array_equal(R, FAR) and score == np.exp(-10.0)


def _check_gicp_batch(pairs, single, oracle, K, first, **options):
    mb = sm.NdtGicpHip(**_gicp_caps(pairs), jobs=first + K, **options)
    for k in range(K):
        mb.set_input_source(pairs[k][0], slot=first + k); mb.set_input_target(pairs[k][1], slot=first + k)
    for attempt in ("rebuilt", "kept"):
        R, sc, st = mb.align_batch(K, [p[2] for p in pairs[:K]], first_job=first)
        for k in range(K):
            R1, s1, st1 = single[k]
            assert np.array_equal(R[k], R1), f"{attempt}: job {k} pose differs from the single call's by {np.abs(R[k] - R1).max():.3e}"
            assert sc[k] == s1, (attempt, k, sc[k], s1)
            for key in GICP_FIELDS:
                assert st[k][key] == st1[key], (attempt, k, key, st[k][key], st1[key])
            oracle.check(k, R[k], sc[k], st[k], attempt)
    mb.close()
    return R, sc, st


@pytest.mark.parametrize("K, first, filt", [(16, 0, 1), (17, 2, 1), (33, 0, 1), (33, 0, 0)],
                         ids=["16-jobs", "17-jobs-from-2", "33-jobs", "33-jobs-unfiltered"])
def test_ndt_gicp_batch_across_launch_limits(gicp_pairs, gicp_single_on, gicp_single_off, gicp_oracle, K, first, filt):
    """16 = one full gicp_corr / gicp_fdf launch, 17 = one more job in a second launch, 33 = a full gicp_knn_cov launch of sources
    and one more, and 66 clouds for the batched voxel filter when the targets are rebuilt (two passes).  Unfiltered, the jobs are
    staged one at a time and only the launch splits are crossed."""
    single = gicp_single_on if filt else gicp_single_off
    _check_gicp_batch(gicp_pairs, single, gicp_oracle[filt], K, first, using_voxel_filter=filt)


def test_ndt_gicp_batch_of_65_with_a_rejected_job(gicp_pairs, gicp_single_on, gicp_oracle):
    """65 jobs: 130 clouds for the voxel filter when the targets are rebuilt, 65 sources when they are kept -- past 64 both times.
    One job's NDT stage is rejected; the jobs finish at different rounds."""
    R, sc, st = _check_gicp_batch(gicp_pairs, gicp_single_on, gicp_oracle[1], N_PAIRS, 0)
    assert st[GICP_REJECTED]["ok"] == 0 and np.array_equal(R[GICP_REJECTED], FAR) and sc[GICP_REJECTED] == np.exp(-10.0)
    assert sum(s["ok"] for s in st) == N_PAIRS - 1
    assert len({s["gicp_function_evaluations"] for s in st}) > 1, "the jobs all took the same path: the batch was never out of step"


# ---- Ndt -------------------------------------------------------------------------------------------------------------------------

NDT_SUBMAP, NDT_SMALL = 5, 20                   # the batch's largest target (~90 k points, sets the key width alone) and a small one
NDT_FAR = {7: synth.make_pose(t=(40.0, 25.0, 1.0)), 27: synth.make_pose(rpy_deg=(0, 0, 30.0)), 30: synth.make_pose(t=(6.0, -3.0, 0.2))}
NDT_FAR_ABS = {13: synth.make_pose(t=(500.0, 0.0, 0.0))}


def _submap():
    """A source scan and a target merged from the three scans before it (the shape of tests/test_ndt_gpu.py's ndt_case)."""
    scene = synth.make_scene(0)
    poses = [synth.make_pose(t=(0.8 * k, 0.02 * k, 0.0), rpy_deg=(0, 0, 0.5 * k)) for k in range(4)]
    scans = [synth.velodyne_scan(scene, P, seed=10 + k, n_points=30000) for k, P in enumerate(poses)]
    tgt = np.concatenate([s[:, :3].astype(np.float64) @ P[:3, :3].T + P[:3, 3] for s, P in zip(scans[:3], poses[:3])]).astype(np.float32)
    return np.ascontiguousarray(scans[3][:, :3]), tgt, poses[3]


@pytest.fixture(scope="module")
def ndt_pairs(scenes):
    pairs = []
    for p in range(N_PAIRS):
        src, tgt, T = _submap() if p == NDT_SUBMAP else _derived(scenes, p)
        if p == NDT_SMALL:
            tgt = np.ascontiguousarray(scenes[p % 10][0][::6, :3])
        if p in NDT_FAR_ABS:
            G = NDT_FAR_ABS[p]
        elif p in NDT_FAR:
            G = T @ NDT_FAR[p]
        else:
            G = T @ synth.make_pose(t=(-0.1 - 0.03 * (p % 7), 0.03 * (p % 3), 0.0), rpy_deg=(0, 0, 0.2 * (p % 4)))
        pairs.append((src, tgt, G))
    _distinct_sizes(pairs)
    nt = sorted(len(p[1]) for p in pairs)
    assert len(pairs[NDT_SMALL][1]) == nt[0] < 4000 and len(pairs[NDT_SUBMAP][1]) == nt[-1] > 2 * nt[-2]
    return pairs


def _ndt_caps(pairs):
    return dict(max_source_points=max(len(p[0]) for p in pairs), max_target_points=max(len(p[1]) for p in pairs))


@pytest.fixture(scope="module")
def ndt_single(ndt_pairs):
    m = sm.NdtHip(**_ndt_caps(ndt_pairs))
    out = []
    for src, tgt, G in ndt_pairs:
        m.set_input_source(src); m.set_input_target(tgt)
        ok, R = m.align(G)
        out.append((R, m.get_fitness_score(), dict(m.last_ndt_stats)))
    m.close()
    return out


class _NdtOracle:
    def __init__(self, pairs):
        self.pairs, self.cache = pairs, {}

    def of(self, p):
        if p not in self.cache:
            tgt = self.pairs[p][1]
            self.cache[p] = (ondt.VoxelGrid(tgt).occupied, cKDTree(tgt.astype(np.float64)))
        return self.cache[p]

    def check(self, p, R, score, st, what):
        occupied, tree = self.of(p)
        assert st["voxels"] == occupied, (what, p, st["voxels"], occupied)
        # pcl getFitnessScore: the source moved by the float32 of the returned pose, mean squared 1-NN distance over the raw target
        Rf = R.astype(np.float32)
        moved = (self.pairs[p][0].astype(np.float32) @ Rf[:3, :3].T + Rf[:3, 3]).astype(np.float64)
        d, _ = tree.query(moved)
        want = float(np.mean(d * d))
        assert abs(score - want) <= 2e-5 * want + 1e-9, (what, p, score, want)


@pytest.fixture(scope="module")
def ndt_oracle(ndt_pairs):
    return _NdtOracle(ndt_pairs)


def test_ndt_single_calls_match_the_oracle(ndt_pairs, ndt_single, ndt_oracle):
    """The references of the batches below: the voxel count is every occupied voxel of the target (searchable or not), the fitness
    the exact nearest-neighbour mean; the far guesses leave the source off the target (their queries go through the far pass)."""
    for p, (R, score, st) in enumerate(ndt_single):
        ndt_oracle.check(p, R, score, st, "single")
    near = [s for p, (_, s, _) in enumerate(ndt_single) if p not in NDT_FAR and p not in NDT_FAR_ABS]
    assert max(near) < 5.0 and min(ndt_single[p][1] for p in (7, 13)) > 100.0
    assert len({st["iterations"] for _, _, st in ndt_single}) > 1


@pytest.mark.parametrize("K, first", [(33, 0), (64, 1), (65, 0)], ids=["33-pairs", "64-pairs-from-1", "65-pairs"])
def test_ndt_batch_across_key_and_grid_limits(ndt_pairs, ndt_single, ndt_oracle, K, first):
    """One target of ~90 k points sets the sort key width of the whole batch, one of ~2.5 k is the smallest; near, half-off, far
    and turned guesses share the fitness passes.  Pairs first .. first + K - 1 in slots of the same numbers."""
    mb = sm.NdtHip(**_ndt_caps(ndt_pairs), pair_slots=first + K)
    for p in range(first, first + K):
        mb.set_input_source(ndt_pairs[p][0], slot=p); mb.set_input_target(ndt_pairs[p][1], slot=p)
    for attempt in ("rebuilt", "kept"):
        R, sc, st = mb.align_batch(K, [ndt_pairs[p][2] for p in range(first, first + K)], first_slot=first)
        for k in range(K):
            p = first + k
            R1, s1, st1 = ndt_single[p]
            assert R[k].tobytes() == R1.tobytes(), (attempt, p, np.abs(R[k] - R1).max())
            assert sc[k] == s1 and st[k] == st1, (attempt, p, sc[k], s1, st[k], st1)
            ndt_oracle.check(p, R[k], sc[k], st[k], attempt)
    mb.close()
