"""Seeded inputs for the two epilogue pieces of the "Eigen 3.3.7" arithmetic mode (cvo_slam_amd/csrc/cvo_eigen337.hpp), shared by the host
check (tests/test_arith_mode_host.py) and the device check (tests/test_gpu_arith_mode.py).  Both compare bit for bit with the oracle's
reference-noise variants (pyoracle.cubic_step_f32eig, pyoracle.dist_se3_f32logm)."""
import glob
import os

import numpy as np

from conftest import GOLDEN

N_CASES = 100_000


def trace_coefficients():
    """{c3, c2, c1, c0} as the epilogue forms them (cvo.cpp:318) from the B..E of every line-search trace row of the golden pairs."""
    rows = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "small_pair_*.npz"))) + [os.path.join(GOLDEN, "tum_pair_0.npz")]:
        d = np.load(path)
        for B, C, D, E in d["trace_BCDE"].astype(np.float64):
            rows.append([np.float32(4.0 * np.float32(E)), np.float32(3.0 * np.float32(D)), np.float32(2.0 * np.float32(C)), np.float32(B)])
    return np.asarray(rows, np.float32)


def _from_roots(c3, r1, r2, r3):
    """c3 (t - r1)(t - r2)(t - r3) as {c3, c2, c1, c0}"""
    return np.stack([c3, -c3 * (r1 + r2 + r3), c3 * (r1 * r2 + r1 * r3 + r2 * r3), -c3 * r1 * r2 * r3], axis=1)


def cubic_cases(n=N_CASES, seed=1):
    """n x {c3, c2, c1, c0, min_step}: the golden traces (as they are, and perturbed), double and near-double roots, complex pairs,
    no positive root (-> min_step), a tiny c3, roots above the 0.8 clamp, and plain random coefficients."""
    rng = np.random.default_rng(seed)
    tr = trace_coefficients()
    parts = [tr]
    k = n // 8
    idx = rng.integers(0, len(tr), k)
    parts.append(tr[idx] * (1.0 + rng.normal(0, 1e-3, (k, 4))))                                  # the line search's own coefficients, perturbed
    c3 = -np.exp(rng.uniform(np.log(1e-2), np.log(1e4), k))                                     # (the line search's quartic has E < 0: c3 < 0)
    r = rng.uniform(0.01, 1.5, k)
    parts.append(_from_roots(c3, r, r, rng.uniform(-2, 2, k)))                                   # double roots
    parts.append(_from_roots(c3, r, r * (1 + rng.uniform(-1e-5, 1e-5, k)), rng.uniform(-2, 2, k)))   # near-double roots
    a, b = rng.uniform(-1, 1, k), np.exp(rng.uniform(np.log(1e-6), np.log(1.0), k))
    re3 = rng.uniform(-1, 1.5, k)
    parts.append(np.stack([c3, c3 * (-2 * a - re3), c3 * (a * a + b * b + 2 * a * re3), -c3 * re3 * (a * a + b * b)], axis=1))   # complex pair + one real root
    parts.append(_from_roots(c3, -rng.uniform(0.01, 3, k), -rng.uniform(0.01, 3, k), -rng.uniform(0.01, 3, k)))                  # no positive root
    tiny = _from_roots(np.ones(k), rng.uniform(-1, 1, k), rng.uniform(-1, 1, k), rng.uniform(-1, 1, k))
    tiny[:, 0] = rng.choice([-1, 1], k) * np.exp(rng.uniform(np.log(1e-38), np.log(1e-6), k))   # tiny c3 (up to overflow of the monic row)
    parts.append(tiny)
    parts.append(_from_roots(c3, rng.uniform(0.8, 5, k), rng.uniform(0.8, 5, k), -rng.uniform(0.01, 3, k)))                      # clamp to 0.8
    coef = np.concatenate(parts).astype(np.float32)
    rest = n - len(coef)
    if rest > 0:
        coef = np.concatenate([coef, rng.normal(0, 1, (rest, 4)).astype(np.float32) * np.exp(rng.uniform(-5, 5, (rest, 1))).astype(np.float32)])
    cases = np.zeros((len(coef), 5), np.float32)
    cases[:, :4] = coef
    cases[:, 4] = 0.2
    cases[: len(cases) // 50, 4] = rng.uniform(0.05, 1.0, len(cases) // 50).astype(np.float32)    # other min_step values
    return cases


def dist_cases(oracle, n=N_CASES, seed=2):
    """n x {dR row-major, dT} from Exp_SEK3 (oracle.exp_sek3) of random twists: rotation angles from 1e-9 (below the theta < 1e-6 branch) to 1,
    translations from 1e-9 to 1, the identity, and the pose updates of the golden traces' first iterations."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 12), np.float32)
    out[0, [0, 4, 8]] = 1.0                                                                      # identity
    for i in range(1, n):
        d = rng.normal(size=3)
        w = d / np.linalg.norm(d) * np.exp(rng.uniform(np.log(1e-9), np.log(1.0)))
        d = rng.normal(size=3)
        v = d / np.linalg.norm(d) * np.exp(rng.uniform(np.log(1e-9), np.log(1.0)))
        if i % 10 == 1:
            v = np.zeros(3)                                                                     # pure rotations
        dR, dT = oracle.exp_sek3(w.astype(np.float32), v.astype(np.float32), float(rng.uniform(0.01, 0.8)))
        out[i, :9] = dR.reshape(9)
        out[i, 9:] = dT
    return out


def bits(x):
    """float32 bit patterns, every NaN folded to one (a failed logarithm is NaN on both sides)"""
    x = np.asarray(x, np.float32).copy()
    x[np.isnan(x)] = np.float32("nan")
    return x.view(np.uint32)
