"""Oracle vs known answers from numpy/scipy (tests/golden/closed_forms.json) and vs the
reference's own nanoflann radius search (tests/golden/ref_nanoflann_radius.npz), SURVEY.md 8c."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def kat():
    with open(os.path.join(GOLDEN, "closed_forms.json")) as f:
        return json.load(f)


def test_cubic_step_matches_numpy_roots(oracle, kat):
    # cvo.cpp:76-92,317-333: smallest strictly positive real root, else min_step 0.2, clamp 0.8
    for case in kat["cubic"]:
        c = case["coef"]
        got = oracle.cubic_step(c[0], c[1], c[2], c[3], 0.2)
        root = case["smallest_positive_real_root"]
        want = 0.2 if root is None else min(root, 0.8)
        assert got == pytest.approx(want, rel=2e-5, abs=1e-7), (c, got, want)


def test_cubic_degenerate_leading_coefficient(oracle):
    # E == 0 -> division by zero in the companion matrix -> no root qualifies -> min_step
    assert oracle.cubic_step(0.0, 1.0, -1.0, 0.5, 0.2) == pytest.approx(0.2)
    assert oracle.cubic_step(0.0, 0.0, 0.0, 0.0, 0.2) == pytest.approx(0.2)


def test_exp_sek3_matches_scipy_expm(oracle, kat):
    for case in kat["exp"]:
        dR, dT = oracle.exp_sek3(case["omega"], case["v"], case["dt"])
        # the reference evaluates (1-cos)/theta^2 and (dt*theta-sin)/theta^3 in f32 (LieGroup.cpp:176-179):
        # the cancellation costs ~1e-5 relative on dT for small angles; the oracle keeps that formula
        np.testing.assert_allclose(dR.ravel(), case["R"], atol=1e-5)
        np.testing.assert_allclose(dT, case["t"], atol=5e-5)


def test_exp_sek3_small_angle_quirk(oracle):
    # LieGroup.cpp:168-170 (Q3): theta < 1e-6 -> R = I and Jl = I, so dT = v (NOT dt*v)
    v = np.array([0.3, -0.2, 0.1], np.float32)
    dR, dT = oracle.exp_sek3(np.array([1e-7, 0, 0], np.float32), v, 0.25)
    np.testing.assert_array_equal(dR, np.eye(3, dtype=np.float32))
    np.testing.assert_array_equal(dT, v)


def test_dist_se3_matches_scipy_logm(oracle, kat):
    for case in kat["dist"]:
        got = oracle.dist_se3(case["dR"], case["dT"])
        assert got == pytest.approx(case["frob_log"], rel=2e-3, abs=2e-7), case   # f32 dR carries ~1e-7 absolute noise


def test_hessian_regularize_eigen_shift(oracle, kat):
    # cvo.cpp:726-758: after scaling by -1e-5 and shifting, the eigenvalue of smallest magnitude has |lambda| >= 1
    for case in kat["eig"]:
        H = np.array(case["H"], np.float32).reshape(6, 6)
        out = oracle.hessian_regularize(H, 5)
        ev = np.linalg.eigvalsh(out)
        assert np.abs(ev).min() >= 1.0 - 1e-3
        shift = out[0, 0] - np.float32(H[0, 0]) * np.float32(-1e-5)
        ev0 = np.array(case["eig_scaled"])
        np.testing.assert_allclose(ev, ev0 + shift, rtol=1e-4, atol=1e-3 * max(1.0, np.abs(ev0).max()))
    np.testing.assert_array_equal(oracle.hessian_regularize(np.zeros((6, 6), np.float32), 0), np.eye(6))   # cvo.cpp:755


def test_radius_search_kdtree_equals_brute(oracle):
    rng = np.random.default_rng(5)
    cloud = rng.uniform(-1, 1, size=(2000, 3)).astype(np.float32)
    for q in rng.uniform(-1, 1, size=(50, 3)).astype(np.float32):
        for r2 in (0.0004, 0.0045, 0.05):
            ib, db = oracle.radius_search(cloud, q, r2, use_kdtree=False)
            ik, dk = oracle.radius_search(cloud, q, r2, use_kdtree=True)
            assert sorted(ib.tolist()) == sorted(ik.tolist())
            assert np.all(db < r2) and np.all(np.diff(db) >= 0)          # strict <, sorted by distance


def test_radius_search_matches_reference_nanoflann(oracle):
    """Pin against the reference's own vendored nanoflann (thirdparty/cvo/thirdparty/nanoflann.hpp): its answers on a seeded
    cloud are stored in tests/golden/ref_nanoflann_radius.npz (tests/golden/make_golden.py --reference, through oracle/_ref).
    Same index set, same float d2 values, same distance-sorted order (nanoflann.hpp:249-253,403-406,1285-1286)."""
    g = np.load(os.path.join(GOLDEN, "ref_nanoflann_radius.npz"))
    cloud, queries, radii, counts, idx_all, d2_all = (g[k] for k in ("cloud", "queries", "r2", "counts", "idx", "d2"))
    assert counts.shape == (len(radii), len(queries)) and counts.sum() == len(idx_all) == len(d2_all)
    off = 0
    for r2, cnt in zip(radii, counts):
        for q in range(len(queries)):
            n = int(cnt[q]); idx = idx_all[off:off + n]; d2 = d2_all[off:off + n]; off += n
            io, do = oracle.radius_search(cloud, queries[q], float(r2), use_kdtree=True)
            assert n == len(io)
            ref_pairs = sorted(zip(idx.tolist(), d2.tolist()))
            orc_pairs = sorted(zip(io.tolist(), do.tolist()))
            assert ref_pairs == orc_pairs                                 # bit-identical d2 per index
            np.testing.assert_array_equal(d2, do)                          # same distance-sorted sequence
