"""Per-point support, read densely in numpy: TEST INFRASTRUCTURE for tests/test_gpu_point_support.py, validated against the C++
oracle's totals by tests/test_support_reading.py.

The definition (include/cvo_hip.h, "per-point support"): pair (i, j) of clouds a (rows, moved by a 3 x 4 `tran_a` first when one is
given, cvo.cpp:485-487) and b (columns) is INSIDE when d2 < d2_thres and d2_color < d2_c_thres (cvo.cpp:395-396, 423, 428), its value
is a_ij = ck * k (cvo.cpp:429-431), and a point's support is the sum and the number of its inside pairs.  Built on
second_reading.pair_arrays and the gates second_reading.inner_product uses; no neighbour search, every pair is formed and masked.
"""
from __future__ import annotations

import numpy as np

import second_reading as sr

f32 = np.float32
f64 = np.float64


def move(tran, xyz):
    """transform.linear() * p + transform.translation() (cvo.cpp:485-487) in float32, the three products added as the oracle's
    function_inner_product adds them (oracle/cvo_oracle.cpp: aff_apply, t0 + (t1 + t2), then the translation)."""
    M = np.asarray(tran, f32).reshape(3, 4)
    p = np.asarray(xyz, f32)
    cols = []
    for r in range(3):
        t0 = M[r, 0] * p[:, 0]; t1 = M[r, 1] * p[:, 1]; t2 = M[r, 2] * p[:, 2]
        cols.append((t0 + (t1 + t2)) + M[r, 3])
    return np.stack(cols, axis=1).astype(f32)


def point_support(xa, fa, xb, fb, ell, tran_a=None, P=sr.Params):
    """(sum_a, count_a, sum_b, count_b): row sums and column sums of the inside pairs' values in float64, and their numbers.
    A point without an inside pair has 0 and 0 (no "count 0 reads 1" rule here: that belongs to the cloud's total)."""
    xa = np.asarray(xa, f32); xb = np.asarray(xb, f32); fa = np.asarray(fa, f32); fb = np.asarray(fb, f32)
    if tran_a is not None:
        xa = move(tran_a, xa)
    s2 = f32(P.sigma * P.sigma)
    d2_thres = f32(-2.0 * f64(ell) * f64(ell) * f64(np.log(f32(f32(P.sp_thres / P.sigma) / P.sigma))))         # cvo.cpp:395
    _, _, d2_c_thres = sr.gates(ell, P)                                                                         # cvo.cpp:396
    d2, d2c = sr.pair_arrays(xa, fa, xb, fb)
    inside = (d2 < d2_thres) & (d2c < d2_c_thres)                                                               # cvo.cpp:423, 428
    k = (f64(s2) * np.exp(-d2.astype(f64) / (2.0 * f64(ell) * f64(ell)))).astype(f32)                           # cvo.cpp:429
    ck = (f64(f32(P.c_sigma * P.c_sigma)) * np.exp(-d2c.astype(f64) / (2.0 * f64(P.c_ell) * f64(P.c_ell)))).astype(f32)   # :430
    a = np.where(inside, ck * k, f32(0)).astype(f64)                                                            # cvo.cpp:431
    return a.sum(axis=1), inside.sum(axis=1).astype(np.int64), a.sum(axis=0), inside.sum(axis=0).astype(np.int64)
