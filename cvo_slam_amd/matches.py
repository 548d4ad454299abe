"""What to do with point matches (Cvo.point_matches / CvoBatch.point_matches / CvoTracks.point_matches): the two summaries registration
libraries report for a result, the mutual correspondences a fusion step wants, and the residual vectors of a frame's points.  Plain numpy:
no device code.

A fit record is one direction's dict {rows, matched, sum_w, sum_w_res2} (fit_moving / fit_fixed of a result); anything with those four
fields under those names (a numpy record, a ctypes structure) does as well."""
from __future__ import annotations

import numpy as np


def _field(fit, name):
    return fit[name] if isinstance(fit, dict) or hasattr(fit, "dtype") else getattr(fit, name)


def fitness(fit) -> float:
    """matched / rows: the share of the direction's points that have a partner inside both gates (0.0 for no rows)"""
    rows = int(_field(fit, "rows"))
    return int(_field(fit, "matched")) / rows if rows > 0 else 0.0


def rmse(fit) -> float:
    """sqrt(sum_w_res2 / sum_w): the kernel-weighted RMS distance, in metres, between a point and the weighted mean of its partners; nan when
    nothing matched (sum_w 0)"""
    w = float(_field(fit, "sum_w"))
    return float(np.sqrt(float(_field(fit, "sum_w_res2")) / w)) if w > 0.0 else float("nan")


def mutual(best_moving, best_fixed) -> np.ndarray:
    """(k, 2) int index pairs (i, j), ascending i, with best_moving[i] == j and best_fixed[j] == i: each is the other's best partner"""
    bm = np.asarray(best_moving).astype(np.int64).reshape(-1); bf = np.asarray(best_fixed).astype(np.int64).reshape(-1)
    i = np.nonzero(bm >= 0)[0]
    j = bm[i]
    if ((j >= bf.shape[0]).any()):
        raise ValueError("best_moving names a column past best_fixed")
    keep = bf[j] == i
    return np.stack([i[keep], j[keep]], axis=1)


def residuals(mean, points) -> np.ndarray:
    """mean - points, (n, 3) float32: from each point (in the fixed frame: a moving cloud's points are to be moved by the transform first) to
    the weighted mean of its partners.  A row without a partner has mean 0, so its residual is -point: mask those rows with best >= 0."""
    m = np.asarray(mean, np.float32).reshape(-1, 3); p = np.asarray(points, np.float32).reshape(-1, 3)
    if m.shape != p.shape:
        raise ValueError(f"mean {m.shape} and points {p.shape} differ in shape")
    return m - p
