"""Pose-hypothesis sets for Cvo.score_hypotheses / CvoBatch.score_hypotheses / CvoBatch.seed_hypotheses.  Plain numpy: no device code."""
from __future__ import annotations

import numpy as np


def _rot(axis: int, angle: float) -> np.ndarray:
    c, s = np.cos(angle), np.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i] = c; R[j, j] = c; R[i, j] = -s; R[j, i] = s
    return R


def compose(left, right) -> np.ndarray:
    """left * right for 3 x 4 transforms [R | t] (right is applied to a point first), in double"""
    a = np.asarray(left, np.float64).reshape(3, 4); b = np.asarray(right, np.float64).reshape(3, 4)
    return np.hstack([a[:, :3] @ b[:, :3], (a[:, :3] @ b[:, 3] + a[:, 3])[:, None]])


def around(center, rot_rad: float, trans_m: float) -> np.ndarray:
    """13 transforms (13, 3, 4) float32 around `center` (3 x 4, moving -> fixed): the centre itself, then the centre left-composed with a rotation of
    +rot_rad and -rot_rad about x, y and z, then with a translation of +trans_m and -trans_m along x, y and z."""
    c = np.asarray(center, np.float64).reshape(3, 4)
    out = [c]
    for axis in range(3):
        for sign in (1.0, -1.0):
            out.append(compose(np.hstack([_rot(axis, sign * rot_rad), np.zeros((3, 1))]), c))
    for axis in range(3):
        for sign in (1.0, -1.0):
            d = np.zeros(3); d[axis] = sign * trans_m
            out.append(compose(np.hstack([np.eye(3), d[:, None]]), c))
    return np.asarray(out, np.float32)
