"""Small clouds whose 32-point group boxes are TIGHT: TEST INFRASTRUCTURE for tests/test_sweep_cases.py (which shows on the CPU that the
box-culled sweep of cvo_sweep.hpp really skips on them, and that wrong bounds would lose hits) and tests/test_gpu_sweep_cases.py (which holds
every consumer of the sweep to a dense reading on them).  synth.make_small_pair's clouds are in random order: each group's box spans the
scene and the cull never skips.

Ray-fan geometry.  The column (fixed) cloud has G groups of 32 points; the 32 points of a group share one ray slope y/z = s, the slopes
spread evenly over [-S, S]; z is uniform in [z0, z0 + span], x in +-0.5 z; points ordered by slope, then x: a group's slope box is a
point, so the slope test decides.  Every column point has a partner row at 0.97 R from it in the (y, z) plane along +-(1, -s)/sqrt(1 + s^2),
the direction in which the slope changes fastest; R = sqrt(d2_thres) of the ell in use (so a case is a function of ell).  The row (moving)
cloud is ordered by its own slope (rows at or behind the camera plane last): a wave of 64 rows has a narrow slope box and a wide z box.

Features: a smooth colour field of the position plus noise.  The colour gate d2_c_thres = -2 c_ell^2 log(sp_thres) is 3.9e5, far above
anything 8-bit-like colours reach, so the noise is wide: the difference of two noisy features is N(0, 2 NOISE^2) per channel, d2c is
2 NOISE^2 chi2_5, whose median 4.35 meets the gate at NOISE = 210 -- about half the geometric hits pass the colour gate.  Half the rows
carry their partner's colours instead (and noise of 2): an alignment keeps a pair only when ck k > sp_thres (cvo.cpp:175), which at 0.97 R
needs ck > 0.987 -- those twins are the pairs the align kernel's lists hold, so its own cull is tested on the same geometry.

Everything is numpy with fixed seeds; the arrays are float32 in the layouts set_pcd takes ((n, 3) and (5, n)), both clouds in one frame.
"""
from __future__ import annotations

import numpy as np

import second_reading as sr
from helpers import make_tf

f32 = np.float32
ELLS = (0.03, 0.15)
NOISE = 210.0
#           G,   S,   z0,  span, seed
FANS = {"fan_tum": (20, 0.5, 0.6, 0.8, 1), "fan_steep": (20, 3.0, 0.3, 0.4, 2), "fan_near": (20, 8.0, 0.05, 0.05, 3)}
FAR_SHIFT = np.array([30.0, -20.0, 60.0])
NAMES = ("fan_tum", "fan_steep", "fan_near", "fan_straddle", "fan_far", "fan_ragged_97", "fan_ragged_2113")
BIG = tuple(n for n in NAMES if n != "fan_ragged_97")       # 640 columns or more


def radius(ell) -> float:
    """sqrt(d2_thres) of function_inner_product at ell (cvo.cpp:395)"""
    P = sr.Params
    return float(np.sqrt(f32(-2.0 * np.float64(ell) * np.float64(ell) * np.float64(np.log(f32(f32(P.sp_thres / P.sigma) / P.sigma))))))


def colour(p, rng):
    """(5, n) float32: make_small_pair's kind of field, and NOISE"""
    f = np.stack([128 + 60 * np.sin(3 * p[:, 0] + 1.0) + 30 * np.cos(5 * p[:, 1]), 128 + 50 * np.sin(4 * p[:, 1] + 0.3) + 30 * np.cos(2 * p[:, 2]),
                  128 + 40 * np.sin(2 * p[:, 0] - 2 * p[:, 1]), 20 * np.cos(3 * p[:, 0]), 20 * np.sin(3 * p[:, 1])], axis=0)
    return np.ascontiguousarray(f + rng.normal(0, NOISE, size=f.shape), dtype=f32)


def fan(G, S, z0, span, ell, seed):
    """(columns float64 (32 G, 3), their partners float64 (32 G, 3), row k the partner of column k, arange(32 G): the rows' partner columns)"""
    rng = np.random.default_rng(seed)
    n = 32 * G
    s = np.repeat(np.linspace(-S, S, G), 32)
    z = rng.uniform(z0, z0 + span, n)
    x = rng.uniform(-0.5, 0.5, n) * z
    k = np.lexsort((x, s))                                          # by slope, then x
    s, z, x = s[k], z[k], x[k]
    cols = np.stack([x, s * z, z], axis=1)
    d = 0.97 * radius(ell) * rng.choice([-1.0, 1.0], n) / np.sqrt(1.0 + s * s)
    return cols, cols + np.stack([np.zeros(n), d, -d * s], axis=1), np.arange(n)


def by_slope(rows):
    """the order of the rows by their own ray slope; rows at or behind the camera plane (no slope) last, by y"""
    front = rows[:, 2] > 1.0e-3
    key = np.where(front, rows[:, 1] / np.where(front, rows[:, 2], 1.0), np.inf)
    return np.lexsort((rows[:, 1], key))


def geometry(name, ell):
    """(columns, rows, the column each row is the partner of), positions in float64"""
    if name in FANS:
        G, S, z0, span, seed = FANS[name]
        cols, rows, partner = fan(G, S, z0, span, ell, seed)
    elif name == "fan_straddle":                                     # fan_near pushed towards the camera: about 4 % of the columns end at z <= 1e-3,
        G, S, z0, span, seed = FANS["fan_near"]                      # so some groups hold points on both sides of the plane and some do not
        cols, rows, partner = fan(G, S, z0, span, ell, seed)
        shift = np.array([0.0, 0.0, -z0 + 1.0e-3 - 0.04 * span])
        cols, rows = cols + shift, rows + shift
    elif name == "fan_far":                                          # box gaps rounded at coordinates of tens of metres
        G, S, z0, span, seed = FANS["fan_tum"]
        cols, rows, partner = fan(G, S, z0, span, ell, seed)
        cols, rows = cols + FAR_SHIFT, rows + FAR_SHIFT
    elif name == "fan_ragged_97":                                    # 33 rows (a 32-point group and one) on the last columns of 97 (three groups and one)
        cols, rows, partner = fan(4, 0.5, 0.6, 0.8, ell, 4)
        cols, rows, partner = cols[:97], rows[97 - 33:97], partner[97 - 33:97]
    elif name == "fan_ragged_2113":                                  # 65 rows (a wave and one) on the last columns of 2 113: 67 groups, so groups 64 .. 66 are
        cols, rows, partner = fan(67, 0.5, 0.6, 0.8, ell, 5)                  # met only in box_sweep's second ballot round, and group 63 at the end of its first
        cols, rows, partner = cols[:2113], rows[2113 - 65:2113], partner[2113 - 65:2113]
    else:
        raise KeyError(name)
    k = by_slope(rows)
    return cols, rows[k], partner[k]


def case(name, ell):
    """(fixed_xyz, fixed_feat, moving_xyz, moving_feat): the columns are the fixed cloud, their partners the moving one"""
    cols, rows, partner = geometry(name, ell)
    rng = np.random.default_rng(1000 + NAMES.index(name))
    local = FAR_SHIFT if name == "fan_far" else 0.0                  # the colour field is the scene's, wherever the scene is
    ff, mf = colour(cols - local, rng), colour(rows - local, rng)
    twin = rng.random(rows.shape[0]) < 0.5                           # half the rows carry their partner's colours (and a little noise)
    mf[:, twin] = ff[:, partner[twin]] + rng.normal(0, 2.0, size=(5, int(twin.sum()))).astype(f32)
    return np.ascontiguousarray(cols, dtype=f32), ff, np.ascontiguousarray(rows, dtype=f32), mf


def transform():
    """the small known motion of the moved cases (3 x 4 float32, moving -> fixed)"""
    return make_tf([0.2, 1, 0.1], 0.01, [0.004, -0.002, 0.003])


def away():
    """a transform that separates the clouds entirely: 10 m along x, where the widest case spans 3 m"""
    t = np.eye(3, 4, dtype=f32); t[0, 3] = 10.0
    return t


def moved(c, tf=None):
    """the case with its moving cloud stored displaced by the inverse of tf: handing tf to a call brings it back (to float32 rounding), and
    the boxes the kernel sees are the displaced cloud's own"""
    tf = np.asarray(transform() if tf is None else tf, np.float64)
    fx, ff, mx, mf = c
    stored = (mx.astype(np.float64) - tf[:, 3]) @ tf[:, :3]          # R^T (p - t)
    return fx, ff, np.ascontiguousarray(stored, dtype=f32), mf
