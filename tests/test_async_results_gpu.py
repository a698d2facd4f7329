"""The asynchronous calls the sequence driver and the bench's end-to-end leg are made of -- smhip_icp_enqueue_batch,
smhip_icp_export_results_device, smhip_synchronize, and smhip_icp_fetch_batch as the witness -- from Python, in the driver's own
slot layout (csrc/shard_driver.cc: slots [0, B) hold the pairs of a batch, the first target scan is parked in slot B, targets are
prepared from source slots by the kd forest, `from = [B, 0, 1, ...]`).  The exported 18-double rows are the only result the driver
ever reads: they are compared bit for bit with what fetch_batch and a fresh handle's align_batch return, with the memory around
them, and with the CPU oracle computed from the files alone (tests/driver_ref.py; the conditions that oracle has to meet are
asserted in tests/test_driver_ref.py)."""
import numpy as np
import pytest

import driver_ref as dr

pytestmark = pytest.mark.gpu

PREFIX_PAIRS = 12
BATCHES = [1, 2, 5, 8, 12, 32]
SENTINEL = -12345.678


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    return dr.sequence_sets(tmp_path_factory)


def _handle(B, oracle, n_scans, **opts):
    import staticmapping_amd as sm
    cap = max(len(oracle.scan(k)) for k in range(n_scans)) + 1
    o = dict(max_iteration=20, early_exit=0)
    o.update(opts)
    return sm.IcpFastHip(pair_slots=2 * B, max_source_points=cap, max_target_points=cap, **o)


def _upload_and_prepare(m, oracle, first, nb, B):
    """One batch the way the driver lays it out: the target scan of the batch's first pair parked in slot B, the sources in slots
    0 .. nb - 1, every target prepared from the slot that holds its scan.  Returns the target sizes."""
    clouds = [oracle.scan(first)] + [oracle.scan(first + 1 + k) for k in range(nb)]
    m.set_input_sources_batch(clouds, [B] + list(range(nb)))
    return m.prepare_targets_from_sources([B] + list(range(nb - 1)), list(range(nb)))


def _batches(total, B):
    return [(base, min(B, total - base)) for base in range(0, total, B)]


def _out_tensor(n_doubles):
    import torch
    return torch.full((n_doubles,), SENTINEL, dtype=torch.float64, device="cuda:0")


def _ptr(t, first_double):
    return t.data_ptr() + 8 * first_double


def _unpack(rows):
    """[n, 18] -> (poses [n, 4, 4] in (row, col) indexing, scores, iteration column)."""
    a = np.asarray(rows, dtype=np.float64).reshape(-1, 18)
    return a[:, :16].reshape(-1, 4, 4).transpose(0, 2, 1).copy(), a[:, 16].copy(), a[:, 17].copy()


def _row_of(R, score, iterations):
    return np.concatenate([np.asarray(R, dtype=np.float64).T.reshape(-1), [float(score)], [float(iterations)]])


def _total(B):
    return 32 if B == 32 else PREFIX_PAIRS


@pytest.mark.parametrize("B", BATCHES)
def test_exported_row_is_the_fetched_result(sets, B):
    """Enqueue, export, synchronise, then fetch the same enqueue: the row is the fetched result's bits -- 16 column-major doubles,
    the score, the iteration count as a double."""
    o = sets["full"]
    total = _total(B)
    m = _handle(B, o, total + 1)
    out = _out_tensor(18 * total)
    for base, nb in _batches(total, B):
        _upload_and_prepare(m, o, base, nb, B)
        m.enqueue_batch(nb, [dr.guess()] * nb)
        m.export_results_device(nb, _ptr(out, 18 * base))
        m.synchronize()
        rows = out.cpu().numpy().reshape(-1, 18)[base:base + nb]
        R, sc, st = m.fetch_batch(nb)
        for k in range(nb):
            assert st[k]["status"] == 0 and st[k]["iterations"] == 20, (base, k, st[k])
            assert rows[k].tobytes() == _row_of(R[k], sc[k], st[k]["iterations"]).tobytes(), (B, base, k, rows[k], R[k], sc[k])
    assert m.single_launch_counts()[1] == 0          # no cooperative launch stopped itself and was redone behind the export's back
    m.close()


def _driver_rows(o, total, B, **opts):
    """What the driver does and nothing else: enqueue + export per batch, never a fetch, one synchronise at the end."""
    m = _handle(B, o, total + 1, **opts)
    out = _out_tensor(18 * total)
    for base, nb in _batches(total, B):
        _upload_and_prepare(m, o, base, nb, B)
        m.enqueue_batch(nb, [dr.guess()] * nb)
        m.export_results_device(nb, _ptr(out, 18 * base))
    m.synchronize()
    rows = out.cpu().numpy().reshape(-1, 18).copy()
    m.close()
    return rows


def _align_batch_rows(o, total, B, **opts):
    m = _handle(B, o, total + 1, **opts)
    rows = []
    for base, nb in _batches(total, B):
        _upload_and_prepare(m, o, base, nb, B)
        R, sc, st = m.align_batch(nb, [dr.guess()] * nb)
        rows += [_row_of(R[k], sc[k], st[k]["iterations"]) for k in range(nb)]
    m.close()
    return np.stack(rows)


@pytest.mark.parametrize("B", BATCHES)
def test_rows_exported_without_a_fetch_equal_a_fresh_align_batch(sets, B):
    """The driver never fetches.  Its rows must be those of a fresh handle that goes through the same batches with align_batch."""
    o = sets["full"]
    total = _total(B)
    got = _driver_rows(o, total, B)
    want = _align_batch_rows(o, total, B)
    for k in range(total):
        assert got[k].tobytes() == want[k].tobytes(), (B, k, got[k], want[k])


def test_export_writes_exactly_its_block(sets):
    """Two consecutive enqueue + export calls into adjacent blocks in the middle of a larger tensor, no host synchronisation
    between them (the driver's `local_dev + 18 * base`): exactly 2 x 5 x 18 doubles change, each block holds its own batch."""
    o = sets["full"]
    B, front, back = 5, 7, 11
    m = _handle(B, o, 11)
    out = _out_tensor(front + 18 * 10 + back)
    for base in (0, 5):
        _upload_and_prepare(m, o, base, B, B)
        m.enqueue_batch(B, [dr.guess()] * B)
        m.export_results_device(B, _ptr(out, front + 18 * base))
    m.synchronize()
    a = out.cpu().numpy()
    m.close()
    sentinel = np.float64(SENTINEL).tobytes()
    assert a[:front].tobytes() == sentinel * front and a[front + 180:].tobytes() == sentinel * back
    want = _align_batch_rows(o, 10, B)
    got = a[front:front + 180].reshape(10, 18)
    for k in range(10):
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])
    assert not np.any(got == SENTINEL)


@pytest.mark.parametrize("early_exit", [0, 1])
@pytest.mark.parametrize("which", ["full", "ragged"])
def test_both_layers_against_the_oracle(sets, which, early_exit, capsys):
    """(a) the composition -- batched upload, Morton order, forest-prepared targets, enqueue, export -- against the oracle on its
    own normals from the file order; (b) the ICP alone: the oracle fed the device's own prepared target, read back, where the
    iteration counts must be equal too.  Full size: 32 pairs in one batch; ragged: 12 pairs in batches of 5, 5, 2."""
    o = sets[which]
    total, B = (32, 32) if which == "full" else (12, 5)
    opts = dict(max_iteration=100, early_exit=1) if early_exit else dict(max_iteration=20, early_exit=0)
    m = _handle(B, o, total + 1, **opts)
    out = _out_tensor(18 * total)
    targets = []
    for base, nb in _batches(total, B):
        nts = _upload_and_prepare(m, o, base, nb, B)
        targets += [m.get_target(int(nts[k]), slot=k) for k in range(nb)]
        m.enqueue_batch(nb, [dr.guess()] * nb)
        m.export_results_device(nb, _ptr(out, 18 * base))
    m.synchronize()
    assert m.single_launch_counts()[1] == 0
    T, sc, it = _unpack(out.cpu().numpy())
    m.close()
    wa, wb = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    its_dev, its_a = [], []
    for k in range(total):
        assert it[k] >= 1 and it[k] == int(it[k]), (k, it[k])
        a = o.pair(k, early_exit=bool(early_exit))
        da, dt = dr.se3_error(T[k], a["result"])
        ds = abs(sc[k] - a["score"])
        wa = [max(wa[0], da), max(wa[1], dt), max(wa[2], ds)]
        q, n = targets[k]
        b = o.icp(k, q, n, early_exit=bool(early_exit))
        db, dtb = dr.se3_error(T[k], b["result"])
        dsb = abs(sc[k] - b["score"])
        wb = [max(wb[0], db), max(wb[1], dtb), max(wb[2], dsb)]
        its_dev.append(int(it[k])); its_a.append(a["iterations"])
        print(f"pair {k}: (a) {da:.2e} rad {dt:.2e} m score {ds:.1e} it {int(it[k])}/{a['iterations']}; (b) {db:.2e} rad {dtb:.2e} m score {dsb:.1e} it {b['iterations']}")
        assert da < dr.ROT_TOL and dt < dr.TRANS_TOL and ds < dr.SCORE_TOL, (which, k, "composition", da, dt, ds)
        assert db < dr.ROT_TOL and dtb < dr.TRANS_TOL and dsb < dr.SCORE_TOL, (which, k, "icp alone", db, dtb, dsb)
        assert int(it[k]) == b["iterations"], (which, k, it[k], b["iterations"])
        if not early_exit:
            assert it[k] == 20 == a["iterations"]
        else:
            assert abs(int(it[k]) - a["iterations"]) <= 1, (which, k, it[k], a["iterations"])   # see test_driver_ref.py
    with capsys.disabled():
        print(f"\n[exported rows vs oracle, {which}, early exit {early_exit}] {total} pairs: (a) composition worst {wa[0]:.2e} rad / {wa[1]:.2e} m, "
              f"score {wa[2]:.1e}; (b) ICP alone worst {wb[0]:.2e} rad / {wb[1]:.2e} m, score {wb[2]:.1e}; iterations device "
              f"{min(its_dev)}..{max(its_dev)}, oracle {min(its_a)}..{max(its_a)}, {sum(x != y for x, y in zip(its_dev, its_a))} pairs one off")


def test_a_failed_pair_is_recognisable_from_its_row_alone(sets):
    """A batch of 5 in the plain layout (every target from set_input_target with the oracle's points and normals; nothing non-finite
    goes through the kd forest), slot 2's source all NaN -- input the library answers with a status.  fetch_batch reports that
    pair and no other; its exported row is the guess with score 0 and an iteration count below 1, which is how the driver tells
    it from a finished pair (`row[17] >= 1`; include/smhip.h); the other four rows do not depend on what shared the launch."""
    import staticmapping_amd as sm
    o = sets["full"]
    G = dr.guess()
    rows = {}
    for name in ("bad", "good"):
        cap = dr.N_POINTS + 1
        m = sm.IcpFastHip(pair_slots=5, max_source_points=cap, max_target_points=cap, max_iteration=20, early_exit=0)
        for k in range(5):
            q, n = o.target(k)
            m.set_input_target(q, n, slot=k)
            src = o.scan(k + 1)
            if name == "bad" and k == 2:
                src = np.full_like(src, np.nan)
            m.set_input_source(src, slot=k)
        out = _out_tensor(18 * 5)
        m.enqueue_batch(5, [G] * 5)
        m.export_results_device(5, out.data_ptr())
        m.synchronize()
        rows[name] = out.cpu().numpy().reshape(5, 18).copy()
        if name == "bad":
            with pytest.raises(sm.SmhipError):
                m.fetch_batch(5)
        else:
            m.fetch_batch(5)
        status = [s["status"] for s in m.last_stats]
        assert [s != 0 for s in status] == [name == "bad" and k == 2 for k in range(5)], status
        m.close()
    T, sc, it = _unpack(rows["bad"])
    Tg, scg, itg = _unpack(rows["good"])
    assert np.array_equal(T[2], G) and sc[2] == 0.0
    assert not (it[2] >= 1.0), it[2]
    assert list(itg) == [20.0] * 5 and [it[k] for k in (0, 1, 3, 4)] == [20.0] * 4
    for k in (0, 1, 3, 4):
        da, dt = dr.se3_error(T[k], Tg[k])
        assert da < 1e-10 and dt < 1e-10, (k, da, dt)
        # score = exp(-mean distance): a pose 1e-10 rad / 1e-10 m away moves no distance by more than 1e-10 x the 120 m range + 1e-10
        assert abs(sc[k] - scg[k]) < 1e-10 * 120.0 + 1e-10
    # and the good batch is the right answer: the oracle's, on the same targets
    for k in range(5):
        a = o.pair(k)
        da, dt = dr.se3_error(Tg[k], a["result"])
        assert da < dr.ROT_TOL and dt < dr.TRANS_TOL and abs(scg[k] - a["score"]) < dr.SCORE_TOL, (k, da, dt)
