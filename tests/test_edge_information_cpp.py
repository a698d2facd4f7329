"""include/smhip/edge_information.h without a GPU, through tests/cpp/test_edge_information.cc: MakeEdgeInformation's limits (an alignment
that pins everything gives the floor back, one that sees nothing gives the floor inflated max_inflation times, a rank-5 one
inflates exactly one direction), L^T L symmetric positive definite in every case, the numpy restatement
(tests/icp_information_ref.py), and the header's cyclic Jacobi against numpy's eigh.  The program computes every case twice and
fails when the bits differ."""
import os
import struct
import subprocess

import numpy as np
import pytest

import icp_information_ref as info

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_edge_information.cc")
FLOOR = info.DEFAULT_FLOOR
W2 = np.diag(1.0 / FLOOR ** 2)


def _exe():
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "test_edge_information")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "include", "smhip", "edge_information.h")]
    if (not os.path.exists(exe)) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe])
    return exe


def run(cases, tmp_path):
    """cases: dicts with H, sum_r2, kept and optionally min_residual_sigma, information_scale, max_inflation, floor"""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as fh:
        fh.write(struct.pack("<i", len(cases)))
        for c in cases:
            row = np.zeros(48)
            row[:36] = np.asarray(c["H"], np.float64).reshape(36)
            row[36:42] = [c["sum_r2"], c["kept"], c.get("min_residual_sigma", 0.02), c.get("information_scale", 1.0), c.get("max_inflation", 100.0),
                          1.0 if "floor" in c else 0.0]
            fh.write(row.astype("<f8").tobytes())
            if "floor" in c:
                fh.write(np.asarray(c["floor"], "<f8").tobytes())
    out = subprocess.run([_exe(), str(src), str(dst)], text=True, capture_output=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    a = np.frombuffer(open(dst, "rb").read(), "<f8").reshape(len(cases), 91)
    return [dict(L=r[:36].reshape(6, 6), strength=r[36:42], weakest=r[42:48], residual_sigma=r[48], w=r[49:55], Q=r[55:91].reshape(6, 6)) for r in a]


def _spd(L):
    M = L.T @ L
    assert np.array_equal(M, M.T) or np.allclose(M, M.T, rtol=0, atol=1e-12 * np.abs(M).max())
    assert np.linalg.eigvalsh(0.5 * (M + M.T)).min() > 0.0
    return M


def test_an_alignment_that_pins_everything_gives_the_floor_back(tmp_path):
    got = run([dict(H=c * np.eye(6), sum_r2=0.0, kept=1000) for c in (1e6, 1e9, 1e12)], tmp_path)
    for c, g in zip((1e6, 1e9, 1e12), got):
        M = _spd(g["L"])
        h_min = c / 0.02 ** 2 * 0.1 ** 2                      # the smallest whitened eigenvalue
        assert np.abs(M - W2).max() <= 1.01 / h_min * W2.max(), c
        assert g["residual_sigma"] == 0.02


def test_an_alignment_that_sees_nothing_gives_the_floor_inflated(tmp_path):
    got = run([dict(H=np.zeros((6, 6)), sum_r2=0.0, kept=1000), dict(H=1e6 * np.eye(6), sum_r2=1.0, kept=6),
               dict(H=np.zeros((6, 6)), sum_r2=0.0, kept=1000, max_inflation=10.0)], tmp_path)
    for g, inflation in zip(got, (100.0, 100.0, 10.0)):
        M = _spd(g["L"])
        assert np.allclose(M, W2 / inflation ** 2, rtol=1e-14, atol=0)
        assert np.all(g["strength"] == 0.0)


def test_a_rank_five_alignment_inflates_exactly_one_direction(tmp_path):
    rng = np.random.default_rng(7)
    Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    floor = np.array([0.1, 0.12, 0.08, 0.15, 0.2, 0.1])
    lam = np.array([0.0, 3e7, 5e7, 8e7, 2e8, 4e8])
    H = (Q * lam) @ Q.T
    sum_r2, kept = 0.03 ** 2 * 994, 1000                     # sigma2 = 0.03^2
    g = run([dict(H=H, sum_r2=sum_r2, kept=kept, floor=floor)], tmp_path)[0]
    assert np.isclose(g["residual_sigma"], 0.03, rtol=1e-12)
    M = _spd(g["L"])
    Wm = np.diag(1.0 / floor)
    Mw = np.linalg.inv(Wm) @ M @ np.linalg.inv(Wm)            # the edge's information in units of the floor's
    ev = np.linalg.eigvalsh(0.5 * (Mw + Mw.T))
    h = g["strength"]
    assert h[0] < 1e-6 and h[1] > 1e3
    assert np.isclose(ev[0], 1e-4, rtol=1e-6)                    # one direction: the floor's sigma times 100
    assert np.all(1.0 - ev[1:] <= 1.0 / h[1] * 1.000001) and np.all(ev[1:] <= 1.0 + 1e-12)   # five: the floor to 1/h
    x = g["weakest"]                                             # the direction H does not see
    assert np.isclose(np.linalg.norm(x), 1.0) and x[int(np.argmax(np.abs(x)))] > 0
    assert np.linalg.norm(H @ x) <= 1e-8 * lam.max()
    assert abs(x @ Q[:, 0]) > 1.0 - 1e-9


def test_the_header_follows_the_numpy_restatement(tmp_path):
    rng = np.random.default_rng(11)
    cases = []
    for k in range(20):
        J = rng.normal(size=(50, 6)) * rng.uniform(0.1, 30.0, size=6)
        cases.append(dict(H=J.T @ J * 10.0 ** rng.uniform(-2, 4), sum_r2=rng.uniform(0.0, 0.5), kept=int(rng.integers(5, 400)),
                          information_scale=10.0 ** rng.uniform(-2, 0), max_inflation=float(rng.choice([10.0, 100.0, 1000.0]))))
    got = run(cases, tmp_path)
    for c, g in zip(cases, got):
        want = info.edge_information(c["H"], c["sum_r2"], c["kept"], information_scale=c["information_scale"], max_inflation=c["max_inflation"])
        M = _spd(g["L"])
        Mw = want["L"].T @ want["L"]
        assert np.abs(M - Mw).max() <= 1e-10 * np.abs(Mw).max()
        assert np.allclose(g["strength"], want["strength"], rtol=1e-9, atol=1e-9 * want["strength"].max())
        assert np.isclose(g["residual_sigma"], want["residual_sigma"], rtol=1e-14)
        if c["kept"] > 6:
            assert abs(g["weakest"] @ want["weakest"]) > 1.0 - 1e-9 and g["weakest"][int(np.argmax(np.abs(g["weakest"])))] > 0


def test_the_jacobi_solver_against_eigh(tmp_path):
    rng = np.random.default_rng(2024)
    mats = []
    for k in range(100):
        A = rng.normal(size=(6, 6)) * 10.0 ** rng.uniform(-3, 3)
        A = A + A.T
        if k % 10 == 0:
            A = A @ A.T                                          # semi-definite ones too, one of them rank-deficient
        if k == 50:
            A[:, 0] = 0.0
            A[0, :] = 0.0
        mats.append(A)
    got = run([dict(H=A, sum_r2=0.0, kept=100) for A in mats], tmp_path)
    worst = 0.0
    for A, g in zip(mats, got):
        w, Q = g["w"], g["Q"]
        norm = np.abs(np.linalg.eigvalsh(A)).max()
        assert np.all(np.diff(w) >= 0.0)
        worst = max(worst, np.abs(w - np.linalg.eigvalsh(A)).max() / norm, np.abs(Q @ np.diag(w) @ Q.T - A).max() / norm,
                    np.abs(Q.T @ Q - np.eye(6)).max())
    print("worst eigenvalue / reconstruction / orthogonality error over the spectral norm:", worst)
    assert worst <= 1e-12
