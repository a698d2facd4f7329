"""The restatement of IcpFast with inner motion compensation (tests/icp_compensation_ref.py) against the rigid oracle it is built
on, and the experiment that says what the mode is for.  CPU only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_compensation_ref as cr  # noqa: E402
from oracle import icp_fast as ref  # noqa: E402


@pytest.fixture(scope="module")
def small():
    """A 3 000-point scan pair: enough for every leaf of the definition, seconds for the oracle."""
    from staticmapping_amd import synth
    a, b, T = synth.scan_pair("cfg2", n_points=3000)
    q, n, _ = ref.calculate_normals(a[:, :3].astype(np.float64))
    ok = np.isfinite(n).all(axis=1)
    return dict(src=b[:, :3].astype(np.float64), q=q[ok], n=n[ok], guess=synth.make_pose(t=(0.6, 0.0, 0.0)))


@pytest.fixture(scope="module")
def prototype():
    return cr.prototype_case(20_000)


def test_iteration_zero_is_the_rigid_iteration_zero(small):
    """T_iter = I: the step cloud is P0 rounded to float, so the matches and the kept set are icp_fast_align's (this pair has no
    query whose two nearest targets lie within that rounding of each other, nor two distances that close at the quantile)."""
    tr_c, tr_r = [], []
    cr.icp_fast_align_compensated(small["src"], small["q"], small["n"], guess=small["guess"], max_iteration=1, trace=tr_c)
    ref.icp_fast_align(small["src"], small["q"], small["n"], guess=small["guess"], max_iteration=1, trace=tr_r)
    c, r = tr_c[0], tr_r[0]
    assert np.array_equal(c["T_before"], np.eye(4))
    assert np.array_equal(c["ids"], r["ids"])
    assert np.array_equal(c["keep"], r["keep"])
    # a position rounded to float moves by at most sqrt(3) 2^-24 |coordinate|_max = delta; d2 then by at most 2 d delta + delta^2
    delta = np.sqrt(3.0) * 2.0 ** -24 * np.abs(c["P"]).max()
    assert (np.abs(c["d2"] - r["d2"]) <= 2.0 * np.sqrt(r["d2"]) * delta + delta * delta + 1e-15).all()
    # and the sums differ from the rigid ones exactly by the factors
    f = cr.factors(len(small["src"]))
    P, keep, ids = c["P"], c["keep"], c["ids"]
    mu = small["q"].mean(axis=0)
    J = np.concatenate([np.cross(P[keep], small["n"][ids[keep]]), small["n"][ids[keep]]], axis=1)
    rr = np.einsum("ij,ij->i", P[keep] - (small["q"] - mu)[ids[keep]], small["n"][ids[keep]])
    assert np.allclose(c["A"], (J * f[keep, None] ** 2).T @ J, rtol=1e-12, atol=1e-12)
    assert np.allclose(c["b"], -(J * f[keep, None]).T @ rr, rtol=1e-12, atol=1e-12)


def test_the_factor_follows_the_caller_index(small):
    """Rows permuted before the call, each carrying its own index: the same alignment.  Rows permuted WITHOUT their indices are
    another scan (another sweep order) and give another result."""
    rng = np.random.default_rng(11)
    perm = rng.permutation(len(small["src"]))
    kw = dict(guess=small["guess"], max_iteration=4, early_exit=False)
    R0, s0, _ = cr.icp_fast_align_compensated(small["src"], small["q"], small["n"], **kw)
    R1, s1, _ = cr.icp_fast_align_compensated(small["src"][perm], small["q"], small["n"], rows=perm, **kw)
    da, dt = ref.se3_error(R0, R1)
    assert da < 1e-9 and dt < 1e-9 and abs(s0 - s1) < 1e-12              # only the order of the sums differs
    R2, _, _ = cr.icp_fast_align_compensated(small["src"][perm], small["q"], small["n"], **kw)
    da, dt = ref.se3_error(R0, R2)
    assert dt > 1e-3, (da, dt)


def test_a_skewed_scan_is_brought_to_the_end_of_sweep_pose(prototype, capsys):
    """A scan taken while the sensor moves by `delta`, aligned from the pose at the start of its sweep, 20 fixed iterations: the
    compensated Align ends near the pose at the END of the sweep, the rigid Align on the same rows and guess does not."""
    p = prototype
    kw = dict(guess=p["start"], max_iteration=20, early_exit=False)
    Rc, sc, _ = cr.icp_fast_align_compensated(p["src_skewed"], p["q"], p["n"], **kw)
    Rr, sr, _ = ref.icp_fast_align(p["src_skewed"], p["q"], p["n"], **kw)
    ca, ct = ref.se3_error(Rc, p["end"])
    ra, rt = ref.se3_error(Rr, p["end"])
    with capsys.disabled():
        print(f"\n[inner compensation, 20 iterations] compensated {ca:.2e} rad / {ct:.3f} m (score {sc:.4f}), "
              f"rigid {ra:.2e} rad / {rt:.3f} m (score {sr:.4f})")
    assert ct < 0.2 and ct < rt / 3.0, (ct, rt)
    assert ca < ra / 3.0, (ca, ra)
