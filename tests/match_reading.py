"""Point matches, read densely in numpy: TEST INFRASTRUCTURE for tests/test_gpu_point_matches.py, held against
support_reading.point_support and a plain double loop by tests/test_match_reading.py.

The definition (include/cvo_hip.h, "point matches"): rows, columns, the move of a, the two gates and a_ij = ck * k as one float are
per-point support's (tests/support_reading.py).  Per row of a direction: the column of the largest a_ij (floats compared, the lowest
column on a tie), that value, the a-weighted mean of the partners' points (sums and quotient in float64, rounded to float32 once), the
support's sum and count; per direction a fit record.  All coordinates are in the fixed frame: the moving side's partners are b's points
as stored, the fixed side's partners are the moved points of a.  Built on support_reading.move, second_reading.pair_arrays and the gates
support_reading uses; no neighbour search, every pair is formed and masked.
"""
from __future__ import annotations

import numpy as np

import second_reading as sr
import support_reading

f32 = np.float32
f64 = np.float64
FIELDS = ("best", "best_value", "mean", "sum", "count")
EDGE_SIZES = [1, 31, 33, 64, 65]


def edge_pair(pair, n):
    """((xyz, feat) of the moving cloud, of the fixed cloud): the first n points of both clouds of a synth pair (point i of one is point i of
    the other, so every size has partners) -- row blocks and 32-point box groups end unevenly at 1, 31, 33 and 65"""
    cut = lambda c: (np.ascontiguousarray(c.xyz[:n]), np.ascontiguousarray(c.feat[:, :n]))
    return cut(pair.moving), cut(pair.fixed)


def kernel_matrix(xa, fa, xb, fb, ell, tran_a=None, P=sr.Params):
    """(a float32 N x M with 0 outside, inside bool N x M, the rows' points in the fixed frame): support_reading.point_support's own lines"""
    xa = np.asarray(xa, f32); xb = np.asarray(xb, f32); fa = np.asarray(fa, f32); fb = np.asarray(fb, f32)
    if tran_a is not None:
        xa = support_reading.move(tran_a, xa)
    s2 = f32(P.sigma * P.sigma)
    d2_thres = f32(-2.0 * f64(ell) * f64(ell) * f64(np.log(f32(f32(P.sp_thres / P.sigma) / P.sigma))))         # cvo.cpp:395
    _, _, d2_c_thres = sr.gates(ell, P)                                                                         # cvo.cpp:396
    d2, d2c = sr.pair_arrays(xa, fa, xb, fb)
    inside = (d2 < d2_thres) & (d2c < d2_c_thres)                                                               # cvo.cpp:423, 428
    k = (f64(s2) * np.exp(-d2.astype(f64) / (2.0 * f64(ell) * f64(ell)))).astype(f32)                           # cvo.cpp:429
    ck = (f64(f32(P.c_sigma * P.c_sigma)) * np.exp(-d2c.astype(f64) / (2.0 * f64(P.c_ell) * f64(P.c_ell)))).astype(f32)   # :430
    return np.where(inside, ck * k, f32(0)).astype(f32), inside, xa, d2_thres                                   # cvo.cpp:431


def direction(a, inside, rows_xyz, cols_xyz):
    """one direction of the reading: a (rows x columns, float32), the rows' and the columns' points in the fixed frame"""
    n = a.shape[0]
    count = inside.sum(axis=1).astype(np.int64)
    matched = count > 0
    ad = a.astype(f64)
    total = ad.sum(axis=1)
    masked = np.where(inside, a, f32(-1))
    best = np.where(matched, masked.argmax(axis=1), -1).astype(np.int64)        # argmax: the first, so the lowest, column of the maximum
    top = np.sort(masked, axis=1)[:, ::-1][:, :2] if a.shape[1] > 1 else np.concatenate([masked, np.full((n, 1), f32(-1))], axis=1)
    best_value = np.where(matched, top[:, 0], f32(0)).astype(f32)
    second = np.maximum(top[:, 1], f32(0)).astype(f64)                          # a row with one partner: the runner-up is "0"
    gap = np.where(matched, (top[:, 0].astype(f64) - second) / np.where(matched, top[:, 0].astype(f64), 1.0), np.inf)
    mean = np.zeros((n, 3), f32)
    num = ad @ np.asarray(cols_xyz, f32).astype(f64)
    mean[matched] = (num[matched] / total[matched, None]).astype(f32)           # the quotient in float64, one rounding
    r = mean - np.asarray(rows_xyz, f32)                                        # float32
    res2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
    w = total.astype(f32).astype(f64)                                           # (double)sum[i] of the float array
    fit = dict(rows=int(n), matched=int(matched.sum()), sum_w=float(w.sum()), sum_w_res2=float((w * res2.astype(f64)).sum()))
    return dict(best=best, best_value=best_value, mean=mean, sum=total, count=count, fit=fit, gap=gap,
                residual=np.sqrt(res2.astype(f64)) * matched)


def matches(xa, fa, xb, fb, ell, tran_a=None, P=sr.Params):
    """A dict keyed like Cvo.point_matches' result -- best_*, best_value_*, mean_*, sum_* (float64, as support_reading gives it), count_*,
    fit_* for * in moving (the rows of a) and fixed (the rows of b) -- plus per row gap_* (the relative gap between its two largest a_ij:
    (v0 - v1) / v0, v1 = 0 for a single partner, inf for none) and residual_* (|mean - point|, 0 for an unmatched row), d2_thres, and `a`,
    the float32 kernel matrix itself (rows of a by rows of b, 0 outside)."""
    a, inside, xa_moved, d2_thres = kernel_matrix(xa, fa, xb, fb, ell, tran_a, P)
    xb = np.asarray(xb, f32)
    out = {"d2_thres": float(d2_thres), "a": a}
    for side, d in (("moving", direction(a, inside, xa_moved, xb)), ("fixed", direction(a.T, inside.T, xb, xa_moved))):
        for key, v in d.items():
            out[f"{key}_{side}"] = v
    return out
