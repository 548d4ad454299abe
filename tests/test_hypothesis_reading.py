"""tests/hypothesis_reading.py (the dense numpy reading of the hypothesis scores) against the C++ oracle's function_inner_product, the
condition that keeps the selection tests of tests/test_gpu_hypotheses.py honest (the true transform wins by a gap no rounding can close),
cvo_slam_amd.hypotheses.around, and the plumbing of the four entry points that needs no GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import hypothesis_reading as hr
from conftest import ROOT

FIXED, MOVING = 0, 1
NEW_SYMBOLS = ["cvo_score_hypotheses", "cvo_batch_score_hypotheses", "cvo_batch_seed_hypotheses_async", "cvo_batch_hypothesis_results"]


@pytest.fixture(scope="module")
def readings():
    """the reading of the full hypothesis set, once per (case, ell)"""
    from cvo_slam_amd import synth
    out = {}
    for case in hr.CASES:
        p = synth.make_small_pair(*case)
        trans = hr.hypothesis_set(p.true_transform)
        for ell in hr.ELLS:
            out[(case, ell)] = (p, trans) + hr.scores((p.moving.xyz, p.moving.feat), (p.fixed.xyz, p.fixed.feat), trans, ell)
    return out


@pytest.mark.parametrize("ell", hr.ELLS)
@pytest.mark.parametrize("case", hr.CASES)
def test_reading_equals_the_oracle(oracle, readings, case, ell):
    p, trans, values, nums, best = readings[(case, ell)]
    assert trans.shape == (15, 3, 4) and trans.dtype == np.float32
    o = oracle.OracleCvo()
    o.set_pcd(p.fixed.xyz, p.fixed.feat); o.set_pcd(p.moving.xyz, p.moving.feat); o.set_state(np.eye(3), np.zeros(3), ell)
    for k in range(trans.shape[0]):
        rc, (value, num, num_e) = o.function_inner_product(MOVING, trans[k], FIXED)
        assert rc == 0 and num_e == 0
        assert int(nums[k]) == num, (case, ell, k)
        assert float(values[k]) == pytest.approx(value, rel=1e-6), (case, ell, k)
    assert int(nums[hr.TRUTH]) > 1


@pytest.mark.parametrize("ell", hr.ELLS)
@pytest.mark.parametrize("case", hr.CASES)
def test_the_truth_wins_by_a_gap_no_rounding_can_close(readings, case, ell):
    _, _, values, _, best = readings[(case, ell)]
    gap = hr.relative_gap(values)
    print(case, ell, "best", best, "relative gap to the second best", gap)
    assert best == hr.TRUTH
    assert gap >= hr.MIN_GAP[ell], (case, ell, gap)


def test_around_is_the_centre_and_twelve_rigid_neighbours():
    from cvo_slam_amd import hypotheses, synth
    c = synth.make_small_pair(5, 200).true_transform
    h = hypotheses.around(c, 0.05, 0.05)
    assert h.shape == (13, 3, 4) and h.dtype == np.float32
    np.testing.assert_array_equal(h[0], np.asarray(c, np.float32))
    for k in range(13):
        R = h[k, :, :3].astype(np.float64)
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-6 and abs(np.linalg.det(R) - 1) <= 1e-6, k
    c64 = np.asarray(c, np.float64)
    for k in range(1, 7):                                               # +- a rotation about x, y, z, composed on the left: D = h * c^-1 is that rotation
        D = h[k, :, :3].astype(np.float64) @ c64[:, :3].T
        ang = np.arccos(np.clip((np.trace(D) - 1) / 2, -1, 1))
        assert ang == pytest.approx(0.05, abs=1e-6)
        axis = np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
        axis /= np.linalg.norm(axis)                                    # (float32 entries: 6e-8 each against a length of 2 sin 0.05 = 0.1)
        want = np.zeros(3); want[(k - 1) // 2] = 1.0 if k % 2 else -1.0
        np.testing.assert_allclose(axis, want, atol=1e-5)
        np.testing.assert_allclose(h[k, :, 3], D @ c64[:, 3], atol=1e-6)
    for k in range(7, 13):                                              # +- a translation along x, y, z
        np.testing.assert_allclose(h[k, :, :3], c64[:, :3], atol=1e-6)
        want = np.zeros(3); want[(k - 7) // 2] = 0.05 if k % 2 else -0.05
        np.testing.assert_allclose(h[k, :, 3] - c64[:, 3], want, atol=1e-6)
    assert hypotheses.around(np.eye(3, 4), 0.0, 0.0).shape == (13, 3, 4)


def test_the_four_entry_points_are_declared_exported_and_bound(hiplib):
    src = open(os.path.join(ROOT, "include", "cvo_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cvo_[a-zA-Z0-9_]+)\s*\(", src))
    out = subprocess.check_output(["nm", "-D", "--defined-only", hiplib.lib_path()], text=True)
    exported = set(re.findall(r" T (cvo_[a-zA-Z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/cvo_hip.h"
        assert name in exported, f"{name} is not exported by the built library"
        assert name in hiplib.api.ABI_SYMBOLS, f"{name} is not listed in api.ABI_SYMBOLS"
    assert re.search(r"#define\s+CVO_MAX_HYPOTHESES\s+64\b", src) and hiplib.api.MAX_HYPOTHESES == 64
    for cls, name in ((hiplib.Cvo, "score_hypotheses"), (hiplib.CvoBatch, "score_hypotheses"), (hiplib.CvoBatch, "seed_hypotheses"),
                      (hiplib.CvoBatch, "hypothesis_results")):
        assert callable(getattr(cls, name, None)), (cls.__name__, name)
