"""Pose hypotheses, read densely in numpy: TEST INFRASTRUCTURE for tests/test_gpu_hypotheses.py, validated against the C++ oracle's
function_inner_product by tests/test_hypothesis_reading.py.

The definition (include/cvo_hip.h, "pose hypotheses"): the score of a hypothesis is function_inner_product (cvo.cpp:388-459) of the moving
cloud under that transform against the fixed cloud.  The reading is support_reading.point_support, summed: value = float32 of the float64
sum of the moving side's per-point sums, num = the number of inside pairs (1 where that is 0, cvo.cpp:455-456), best = the first index of
the largest float32 value.
"""
from __future__ import annotations

import numpy as np

import support_reading
from cvo_slam_amd import hypotheses

ROT, SHIFT = 0.05, 0.05          # the perturbations of the set: 0.05 rad, 5 cm
CASES = [(5, 200), (31, 700), (77, 800)]
ELLS = [0.06, 0.15]
MIN_GAP = {0.06: 1e-2, 0.15: 5e-3}   # relative gap between the best and the second-best value that keeps the selection tests honest
TRUTH = 1                        # index of the true transform in hypothesis_set


def hypothesis_set(true_transform) -> np.ndarray:
    """(15, 3, 4) float32: identity, the true transform, the truth left-composed with +-0.05 rad about x, y, z, with +-5 cm along x, y, z,
    and with one mixed perturbation"""
    around = hypotheses.around(true_transform, ROT, SHIFT)            # the truth first, then the 12 single perturbations
    from helpers import make_tf
    mixed = hypotheses.compose(make_tf([1, -2, 0.5], 0.04, [0.03, -0.02, 0.025]), true_transform)
    return np.concatenate([np.eye(3, 4, dtype=np.float32)[None], around, mixed.astype(np.float32)[None]], axis=0)


def score(moving, fixed, tran, ell):
    """(value float32, num int) of one hypothesis; moving, fixed: (xyz, feat)"""
    sum_a, count_a, _, _ = support_reading.point_support(moving[0], moving[1], fixed[0], fixed[1], ell, tran)
    total = int(count_a.sum())
    return np.float32(np.float64(sum_a.sum(dtype=np.float64))), (total if total else 1)


def scores(moving, fixed, trans, ell):
    """(values float32[K], nums int32[K], best) of the K transforms `trans`"""
    got = [score(moving, fixed, t, ell) for t in np.asarray(trans, np.float32).reshape(-1, 3, 4)]
    values = np.array([g[0] for g in got], np.float32); nums = np.array([g[1] for g in got], np.int32)
    return values, nums, int(np.argmax(values))


def relative_gap(values) -> float:
    """(best - second best) / best of float32 values"""
    v = np.sort(np.asarray(values, np.float64))[::-1]
    return float((v[0] - v[1]) / v[0]) if v[0] > 0 else 0.0
