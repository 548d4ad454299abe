"""Pose models, read densely in numpy: TEST INFRASTRUCTURE for tests/test_gpu_pose_models.py, validated against central differences of the energy
by tests/test_pose_model_reading.py.

The definition (include/cvo_hip.h, "pose models"): value, gradient and Hessian at xi = 0 of f(xi) = the sum of a_ij = ck * k over the pairs inside
both gates, the moving cloud under Exp(xi^) o T, the inside set frozen.  Built on support_reading.move, second_reading.pair_arrays and
second_reading.gates like the other readings; the float sequence is the definition's: a pair's terms in float32 with the products and sums as
pair_hessian_add_weighted (cvo_sweep.hpp) writes them, every sum over pairs in float64.  Beside each sum its MAGNITUDE: the same formulas with
every factor replaced by its absolute value and every subtraction by an addition -- the scale the float32 rounding of the terms lives on.
"""
from __future__ import annotations

import numpy as np

import second_reading as sr
import support_reading

f32 = np.float32
f64 = np.float64


def inside_pairs(moving, fixed, tran, ell, P=sr.Params):
    """(pa float32[n, 3], pb float32[n, 3], a float32[n], ck float32[n], row sums float64[N]) of the n inside pairs of the moved cloud, row-major"""
    xa = support_reading.move(tran, np.asarray(moving[0], f32)); xb = np.asarray(fixed[0], f32)
    fa = np.asarray(moving[1], f32); fb = np.asarray(fixed[1], f32)
    s2 = f32(P.sigma * P.sigma)
    d2_thres = f32(-2.0 * f64(ell) * f64(ell) * f64(np.log(f32(f32(P.sp_thres / P.sigma) / P.sigma))))         # cvo.cpp:395
    _, _, d2_c_thres = sr.gates(ell, P)                                                                         # cvo.cpp:396
    d2, d2c = sr.pair_arrays(xa, fa, xb, fb)
    inside = (d2 < d2_thres) & (d2c < d2_c_thres)                                                               # cvo.cpp:423, 428
    k = (f64(s2) * np.exp(-d2.astype(f64) / (2.0 * f64(ell) * f64(ell)))).astype(f32)                           # cvo.cpp:429
    ck = (f64(f32(P.c_sigma * P.c_sigma)) * np.exp(-d2c.astype(f64) / (2.0 * f64(P.c_ell) * f64(P.c_ell)))).astype(f32)   # :430
    a = (ck * k).astype(f32)                                                                                    # cvo.cpp:431
    rows = np.where(inside, a, f32(0)).astype(f64).sum(axis=1)
    ii, jj = np.nonzero(inside)
    return xa[ii], xb[jj], a[ii, jj], ck[ii, jj], rows


def pair_terms(pa, pb, il2, mag=False):
    """(cr[n, 3], db[n, 3], B[n, 6, 6]) in float32: pa x pb, pb - pa and the 21 second-order terms of a pair laid out as the 6 x 6 matrix
    (A at (omega, omega), D at (v, v), C at (v, omega), its transpose at (omega, v): cvo.cpp:665-704).  mag: the magnitudes instead."""
    if mag:
        pa, pb = np.abs(pa), np.abs(pb)

    def sub(x, y):
        return x + y if mag else x - y

    def neg(x):
        return x if mag else -x
    a0, a1, a2 = pa[:, 0], pa[:, 1], pa[:, 2]; b0, b1, b2 = pb[:, 0], pb[:, 1], pb[:, 2]
    cr = [sub(a1 * b2, a2 * b1), sub(a2 * b0, a0 * b2), sub(a0 * b1, a1 * b0)]
    db = [sub(b0, a0), sub(b1, a1), sub(b2, a2)]
    dots = [a1 * b1 + a2 * b2, a0 * b0 + a2 * b2, a0 * b0 + a1 * b1]
    n = pa.shape[0]
    A = np.zeros((n, 3, 3), f32); Cm = np.zeros((n, 3, 3), f32); Dm = np.zeros((n, 3, 3), f32)
    for q in range(3):
        A[:, q, q] = sub(il2 * cr[q] * cr[q], dots[q])                                                          # cvo.cpp:670-672
        for r in range(q + 1, 3):                                                                                # :673-675, the 0.5 * product in double
            A[:, q, r] = A[:, r, q] = ((il2 * cr[q] * cr[r]).astype(f64) + 0.5 * (pa[:, q] * pb[:, r] + pa[:, r] * pb[:, q]).astype(f64)).astype(f32)
        Cm[:, q, q] = il2 * cr[q] * db[q]                                                                        # :680-682
    Cm[:, 0, 1] = neg(a2) + il2 * db[0] * cr[1]; Cm[:, 0, 2] = a1 + il2 * db[0] * cr[2]                          # :683-688
    Cm[:, 1, 0] = a2 + il2 * db[1] * cr[0];      Cm[:, 1, 2] = neg(a0) + il2 * db[1] * cr[2]
    Cm[:, 2, 0] = neg(a1) + il2 * db[2] * cr[0]; Cm[:, 2, 1] = a0 + il2 * db[2] * cr[1]
    for p in range(3):
        for q in range(p, 3):                                                                                    # :692-697, the upper half and its mirror
            t = il2 * db[p] * db[q]
            Dm[:, p, q] = Dm[:, q, p] = sub(t, f32(1)) if p == q else t
    B = np.zeros((n, 6, 6), f32)
    B[:, :3, :3] = A; B[:, 3:, :3] = Cm; B[:, :3, 3:] = np.transpose(Cm, (0, 2, 1)); B[:, 3:, 3:] = Dm            # :701-704
    return np.stack(cr, axis=1).astype(f32), np.stack(db, axis=1).astype(f32), B


def hat(g, mag=False):
    s = 1.0 if mag else -1.0
    return np.array([[0, s * g[2], g[1]], [g[2], 0, s * g[0]], [s * g[1], g[0], 0]], f64)


def model(moving, fixed, tran, ell, with_s=1.0, P=sr.Params):
    """dict(value float32, num int, grad float64[6], hess float64[6, 6], mag_grad, mag_hess) of one pose; moving, fixed: (xyz, feat).
    with_s: the factor on S (1: the definition; 0 or -1 only for the test that shows what S is worth)."""
    pa, pb, a, _, rows = inside_pairs(moving, fixed, tran, ell, P)
    ell32 = f32(ell)
    il2 = f32(1) / (ell32 * ell32)
    w = il2 * a                                                                                                   # float32: the energy's own weight
    out = {"value": f32(f64(rows.sum(dtype=f64))), "num": int(a.shape[0]) if a.shape[0] else 1}
    for name, mag in (("", False), ("mag_", True)):
        cr, db, B = pair_terms(pa, pb, il2, mag)
        grad = np.concatenate([(w[:, None] * cr).astype(f64).sum(axis=0), (w[:, None] * db).astype(f64).sum(axis=0)])
        hess = (w[:, None, None] * B).astype(f64).sum(axis=0)
        S = np.zeros((6, 6)); S[3:, :3] = 0.5 * hat(grad[3:], mag); S[:3, 3:] = S[3:, :3].T
        out[name + "grad"] = grad; out[name + "hess"] = hess + (1.0 if mag else with_s) * S
    return out


def models(moving, fixed, trans, ell):
    """the models of K transforms as arrays: (values f32[K], nums i32[K], grads[K, 6], hess[K, 6, 6], mag_grads, mag_hess)"""
    got = [model(moving, fixed, t, ell) for t in np.asarray(trans, f32).reshape(-1, 3, 4)]
    return (np.array([g["value"] for g in got], f32), np.array([g["num"] for g in got], np.int32), np.stack([g["grad"] for g in got]),
            np.stack([g["hess"] for g in got]), np.stack([g["mag_grad"] for g in got]), np.stack([g["mag_hess"] for g in got]))


def frozen_energy(moving, fixed, tran, ell, P=sr.Params):
    """f(xi) in float64 for the inside set of `tran`: a function of a 6-vector xi = [omega; v], the moved cloud under Exp(xi^) (helpers.se3_exp)"""
    from helpers import se3_exp
    pa, pb, _, ck, _ = inside_pairs(moving, fixed, tran, ell, P)
    pa = pa.astype(f64); pb = pb.astype(f64); ck = ck.astype(f64)
    s2 = f64(f32(P.sigma * P.sigma)); den = 2.0 * f64(ell) * f64(ell)

    def f(xi):
        E = se3_exp(np.asarray(xi[:3], f64), np.asarray(xi[3:], f64), 1.0)
        q = pa @ E[:3, :3].T + E[:3, 3]
        return float((ck * s2 * np.exp(-((q - pb) ** 2).sum(axis=1) / den)).sum())
    return f


def central_differences(f, h=1e-4):
    """(grad[6], hess[6, 6]) of f at 0 by central differences of step h"""
    e = np.eye(6) * h
    f0 = f(np.zeros(6))
    fp = [f(e[q]) for q in range(6)]; fm = [f(-e[q]) for q in range(6)]
    grad = np.array([(fp[q] - fm[q]) / (2 * h) for q in range(6)])
    hess = np.zeros((6, 6))
    for p in range(6):
        hess[p, p] = (fp[p] - 2 * f0 + fm[p]) / (h * h)
        for q in range(p + 1, 6):
            hess[p, q] = hess[q, p] = (f(e[p] + e[q]) - f(e[p] - e[q]) - f(e[q] - e[p]) + f(-e[p] - e[q])) / (4 * h * h)
    return grad, hess
