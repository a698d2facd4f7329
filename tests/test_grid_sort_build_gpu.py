"""The ICP search grid of a small target is built by one in-LDS stable sort per pair (csrc/grid_sort_build.hip) instead of the
mark / rank / count / cscan / scatter / place kernels over a zeroed bitmap.  Both forms must leave the same bytes -- mean,
geometry, words, cstart, the cell-sorted target -- so that every search, pose, score and count stays what it was.

Two handles live in this process on the same inputs: one created (and configured) with SMHIP_GRID_BUILD=0 in the environment,
which keeps the old kernels for every launch, and one without.  The structure is read back through smhip_icp_debug_get_grid.
The last test restates in numpy what the structure must be and checks the new form against that alone."""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SLOTS, NS_CAP, NT_CAP = 9, 2048, 33000
CELL = np.float32(0.25)


@contextlib.contextmanager
def _old_kernels():
    """The library reads SMHIP_GRID_BUILD whenever a handle's options are resolved (creation, set_options)."""
    os.environ["SMHIP_GRID_BUILD"] = "0"
    try:
        yield
    finally:
        del os.environ["SMHIP_GRID_BUILD"]


@pytest.fixture(scope="module")
def handles():
    import staticmapping_amd as sm
    assert "SMHIP_GRID_BUILD" not in os.environ
    with _old_kernels():
        old = sm.IcpFastHip(pair_slots=SLOTS, max_source_points=NS_CAP, max_target_points=NT_CAP, max_iteration=12)
    new = sm.IcpFastHip(pair_slots=SLOTS, max_source_points=NS_CAP, max_target_points=NT_CAP, max_iteration=12)
    yield old, new
    old.close(); new.close()


def _set_options(handles, **kw):
    old, new = handles
    with _old_kernels():
        old.set_options(**kw)
    new.set_options(**kw)


# ---- clouds ----------------------------------------------------------------------------------------------------------------
def _unit(rs, n):
    v = rs.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _box_cloud(n, seed, extent=(20.0, 20.0, 4.0)):
    rs = np.random.RandomState(seed)
    return rs.uniform(-0.5, 0.5, (n, 3)) * np.asarray(extent) + np.array([3.0, -7.0, 1.0]), _unit(rs, n)


def _planes(n, seed, pose=None, sigma=0.01):
    """n points on three orthogonal 6 m patches with their exact normals (optionally moved by a 4x4 pose)."""
    rs = np.random.RandomState(seed)
    which = rs.randint(0, 3, n)
    p = rs.uniform(0.0, 6.0, (n, 3))
    p[np.arange(n), which] = sigma * rs.standard_normal(n)
    nrm = np.zeros((n, 3)); nrm[np.arange(n), which] = 1.0
    if pose is not None:
        p = p @ pose[:3, :3].T + pose[:3, 3]
        nrm = nrm @ pose[:3, :3].T
    return p, nrm


def _cases():
    rs = np.random.RandomState(7)
    out = {}
    for n in (1, 63, 64, 65, 1023, 1025, 4999, 32768, 32769):
        out[f"n{n}"] = _box_cloud(n, 100 + n)
    out["one_cell"] = (np.array([5.0, 5.0, 5.0]) + 1e-3 * rs.uniform(-1, 1, (100, 3)), _unit(rs, 100))
    lattice = np.stack(np.meshgrid(*[np.arange(10) * 0.5] * 3, indexing="ij"), -1).reshape(-1, 3)
    out["one_point_per_cell"] = (lattice[rs.permutation(len(lattice))] + 0.01 * rs.uniform(-1, 1, lattice.shape), _unit(rs, len(lattice)))
    base, _ = _box_cloud(300, 55, extent=(3.0, 3.0, 1.0))
    out["duplicates_shuffled"] = (base[rs.randint(0, 300, 1500)], _unit(rs, 1500))
    # a lattice symmetric about 0 (the mean is exactly 0): with the origin half a cell below the box every odd step lies on a face
    faces = np.stack(np.meshgrid(*[np.arange(-8, 9) * 0.125] * 3, indexing="ij"), -1).reshape(-1, 3)
    out["cell_faces"] = (faces[rs.permutation(len(faces))], _unit(rs, len(faces)))
    a, _ = _box_cloud(700, 56, extent=(10.0, 10.0, 10.0)); b, _ = _box_cloud(900, 57, extent=(10.0, 10.0, 10.0))
    out["wide_box"] = (np.concatenate([a, b + np.array([400.0, 300.0, 0.0])])[rs.permutation(1600)], _unit(rs, 1600))
    return out


CASES = _cases()
BATCH_NT = [300, 5000, 1023, 1025, 700, 2048, 64, 4999, 1500]        # some above and some below 1 024 points


def _grid_equal(a, b):
    for k in ("mu", "h", "origin", "nx", "ny", "nz", "wx", "nw", "nocc", "nt", "words", "cstart"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    for k in ("tq", "tn"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k      # bits: the caller index rides in tq.w


SMALL_SOURCE = _box_cloud(64, 3, extent=(4.0, 4.0, 2.0))[0]


def _search(m):
    """FindClosests of a 64-point source in slot 0: builds the slot's grid, and gives one more result to compare."""
    m.set_input_source(SMALL_SOURCE)
    return m.find_closests(np.eye(4), len(SMALL_SOURCE))


# ---- 1. the structure ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_structure_is_the_same_bytes(handles, name):
    p, nrm = CASES[name]
    got = []
    for m in handles:
        m.set_input_target(p, nrm)
        ids, d2 = _search(m)
        got.append((m.debug_get_grid(0), ids, d2))
    (ga, ia, da), (gb, ib, db) = got
    assert ga["nt"] == len(p)
    _grid_equal(ga, gb)
    assert np.array_equal(ia, ib) and np.array_equal(da, db)
    if name == "one_cell":
        assert gb["nocc"] == 1
    if name == "one_point_per_cell":
        assert gb["nocc"] == gb["nt"]
    if name == "wide_box":
        assert gb["h"] > CELL and gb["nw"] <= 1 << 18
    if name == "duplicates_shuffled":
        assert gb["nocc"] < gb["nt"] and (np.diff(gb["cstart"].astype(np.int64)) > 1).any()


def test_nan_target_fails_cleanly_and_the_slot_recovers(handles):
    """A target with a NaN coordinate is answered with status 1 (SMHIP_ERR_INVALID_ARGUMENT) by both handles -- the upload is where
    the library refuses it, before any build --, whatever an Align on the slot then says is the same on both, and the next Align on
    that slot with a good target works and leaves the same structure."""
    import staticmapping_amd as sm
    p, nrm = _planes(900, 21)
    bad = p.copy(); bad[417, 1] = np.nan
    good_t, good_n = _planes(1200, 22)
    src, _ = _planes(64, 23)
    res = []
    for m in handles:
        m.set_input_source(src)
        m.set_input_target(p, nrm); m.align(np.eye(4))           # a structure is resident when the bad target arrives
        with pytest.raises(sm.SmhipError) as e:
            m.set_input_target(bad, nrm)
        try:
            _, T = m.align(np.eye(4))
            after = (0, T.tobytes(), m.last_stats[0])
        except sm.SmhipError as e2:
            after = (e2.status, None, None)
        m.set_input_target(good_t, good_n)
        _, T = m.align(np.eye(4))
        res.append((e.value.status, after, T, m.last_stats[0], m.debug_get_grid(0)))
    assert res[0][0] == 1 and res[1][0] == 1
    assert res[0][1] == res[1][1]
    assert res[0][3]["status"] == 0 and res[1][3]["status"] == 0 and res[1][3]["kept"] > 0
    assert np.array_equal(res[0][2], res[1][2]) and res[0][3] == res[1][3]
    assert res[1][4]["nt"] == 1200
    _grid_equal(res[0][4], res[1][4])


@pytest.fixture(scope="module")
def batch_clouds():
    pose = np.eye(4); pose[:3, 3] = (0.05, -0.03, 0.02)
    c, s = np.cos(0.01), np.sin(0.01)
    pose[:2, :2] = [[c, -s], [s, c]]
    return [(_planes(BATCH_NT[k], 300 + k), _planes(2000, 400 + k, pose=pose)[0]) for k in range(SLOTS)]


def _load_batch(m, batch_clouds):
    for k, ((t, n), s) in enumerate(batch_clouds):
        m.set_input_target(t, n, slot=k)
        m.set_input_source(s, slot=k)


def _align_batch(m, npairs):
    res, scores, stats = m.align_batch(npairs)
    return res, scores, [(s["iterations"], s["kept"], s["status"]) for s in stats]


def test_batch_of_nine_pairs(handles, batch_clouds):
    got = []
    for m in handles:
        _load_batch(m, batch_clouds)
        out = _align_batch(m, SLOTS)
        got.append((out, [m.debug_get_grid(k) for k in range(SLOTS)]))
    (oa, ga), (ob, gb) = got
    for k in range(SLOTS):
        assert gb[k]["nt"] == BATCH_NT[k]
        _grid_equal(ga[k], gb[k])
    assert np.array_equal(oa[0], ob[0]) and np.array_equal(oa[1], ob[1]) and oa[2] == ob[2]
    assert all(st == 0 for _, _, st in ob[2])


def test_smaller_target_after_a_larger_one(handles, batch_clouds):
    (t_big, n_big), src = batch_clouds[1]          # 5 000 points
    (t_small, n_small), _ = batch_clouds[0]        # 300
    got = []
    for m in handles:
        m.set_input_source(src)
        m.set_input_target(t_big, n_big); m.align(np.eye(4))
        m.set_input_target(t_small, n_small)
        _, T = m.align(np.eye(4))
        g = m.debug_get_grid(0)
        got.append((T, m.get_fitness_score(), m.last_stats[0], g, m.find_closests(np.eye(4), len(src))))
    a, b = got
    assert b[3]["nt"] == 300
    _grid_equal(a[3], b[3])
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2]
    assert np.array_equal(a[4][0], b[4][0]) and np.array_equal(a[4][1], b[4][1])


# ---- 2. the results --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cache", [True, False])
@pytest.mark.parametrize("no_single_kernel", [0, 1])
def test_results_are_identical(handles, batch_clouds, no_single_kernel, cache):
    _set_options(handles, no_single_kernel=no_single_kernel)
    (t, n), src = batch_clouds[1]                   # a 2 000-point source against a 5 000-point target
    got = []
    try:
        for m in handles:
            m.set_target_cache(cache)
            m.set_input_source(src[:2000]); m.set_input_target(t, n)
            fc = m.find_closests(np.eye(4), len(src[:2000]))
            _, T1 = m.align(np.eye(4)); s1 = (m.get_fitness_score(), m.last_stats[0])
            _, T2 = m.align(np.eye(4)); s2 = (m.get_fitness_score(), m.last_stats[0])      # target unchanged: kept when the cache is on
            _load_batch(m, batch_clouds)
            got.append((fc, T1, s1, T2, s2, _align_batch(m, SLOTS)))
    finally:
        _set_options(handles, no_single_kernel=0)
        for m in handles:
            m.set_target_cache(True)
    a, b = got
    assert np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[0][1], b[0][1])
    assert np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3]) and a[4] == b[4]
    assert np.array_equal(b[1], b[3]) and b[2] == b[4]
    assert np.array_equal(a[5][0], b[5][0]) and np.array_equal(a[5][1], b[5][1]) and a[5][2] == b[5][2]
    assert b[2][1]["status"] == 0 and b[2][1]["iterations"] >= 1 and b[2][1]["kept"] > 0


# ---- 3. what the structure must be, restated -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 4999])
def test_new_form_against_a_numpy_restatement(handles, n):
    _, m = handles
    assert "SMHIP_GRID_BUILD" not in os.environ
    p, nrm = CASES[f"n{n}"]
    m.set_input_target(p, nrm)
    _search(m)
    g = m.debug_get_grid(0)
    raw, raw_n = m.get_target(n)                    # the float32 rows the device holds, in caller order
    assert g["nt"] == n
    c = (raw.astype(np.float64) - g["mu"]).astype(np.float32)
    inv_h = np.float32(1.0) / np.float32(g["h"])
    dims = np.array([g["nx"], g["ny"], g["nz"]])
    cell = np.floor((c - g["origin"].astype(np.float32)) * inv_h).astype(np.int64)
    cell = np.minimum(np.maximum(cell, 0), dims - 1)
    assert g["wx"] == (g["nx"] + 31) // 32 and g["nw"] == g["wx"] * g["ny"] * g["nz"]
    key = (((cell[:, 2] * g["ny"] + cell[:, 1]) * g["wx"] + (cell[:, 0] >> 5)) << 5) | (cell[:, 0] & 31)
    order = np.argsort(key, kind="stable")          # cells in linear order, a cell's points by caller index
    cells, counts = np.unique(key, return_counts=True)
    assert g["nocc"] == len(cells)
    assert np.array_equal(np.diff(g["cstart"].astype(np.int64)), counts) and g["cstart"][0] == 0 and g["cstart"][-1] == n
    bits = np.zeros(g["nw"], np.uint32)
    np.bitwise_or.at(bits, cells >> 5, (np.uint32(1) << (cells & 31).astype(np.uint32)))
    pop = np.array([bin(int(v)).count("1") for v in bits], np.int64)
    assert np.array_equal(g["words"][:, 0], bits)
    assert np.array_equal(g["words"][:, 1].astype(np.int64), np.cumsum(pop) - pop)
    idx = g["tq"][:, 3].copy().view(np.int32)
    assert np.array_equal(idx, order)
    for k in range(len(cells)):                     # (said once more, cell by cell)
        run = idx[g["cstart"][k]:g["cstart"][k + 1]]
        assert (np.diff(run) > 0).all() and (key[run] == cells[k]).all()
    assert np.array_equal(g["tq"][:, :3].view(np.uint32), c[order].view(np.uint32))
    assert np.array_equal(g["tn"][:, :3].view(np.uint32), np.ascontiguousarray(raw_n[order]).view(np.uint32))
    assert (g["tn"][:, 3].view(np.uint32) == 0).all()
