"""What to do with a pose model (Cvo.pose_models / CvoBatch.pose_models / CvoBatch.result_models): a Newton or Levenberg-Marquardt step on the
alignment energy and its retraction onto SE(3).  Plain numpy: no device code.

A model's grad and hess are derivatives of the energy along Exp(xi^) o T, xi = [omega; v] a twist in the fixed frame.  The energy is maximised,
so the step solves (-hess + damping I) delta = grad, and the new pose is retract(delta, T)."""
from __future__ import annotations

import numpy as np


def newton_step(grad, hess, damping: float = 0.0) -> np.ndarray:
    """delta (6,) float64 solving (-hess + damping * I) delta = grad.  damping 0: the Newton step, meaningful where hess is negative definite;
    a positive damping is the Levenberg-Marquardt step, which tends to grad / damping (steepest ascent) as damping grows."""
    g = np.asarray(grad, np.float64).reshape(6); H = np.asarray(hess, np.float64).reshape(6, 6)
    return np.linalg.solve(-H + float(damping) * np.eye(6), g)


def hat(w) -> np.ndarray:
    w = np.asarray(w, np.float64).reshape(3)
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def exp_se3(delta):
    """(R 3 x 3, t 3) of Exp(delta^), delta = [omega; v], by the closed form: R = I + A W + B W^2, t = (I + B W + C W^2) v with W = hat(omega),
    A = sin(th) / th, B = (1 - cos(th)) / th^2, C = (th - sin(th)) / th^3; their series below th = 1e-4."""
    d = np.asarray(delta, np.float64).reshape(6)
    W = hat(d[:3]); W2 = W @ W
    th2 = float(d[:3] @ d[:3]); th = np.sqrt(th2)
    if th < 1e-4:
        A = 1.0 - th2 / 6.0; B = 0.5 - th2 / 24.0; Cc = 1.0 / 6.0 - th2 / 120.0
    else:
        A = np.sin(th) / th; B = (1.0 - np.cos(th)) / th2; Cc = (th - np.sin(th)) / (th2 * th)
    return np.eye(3) + A * W + B * W2, (np.eye(3) + B * W + Cc * W2) @ d[3:]


def retract(delta, T) -> np.ndarray:
    """Exp(delta^) o T as a 3 x 4 float64 transform (T: 3 x 4, moving -> fixed)"""
    R, t = exp_se3(delta)
    M = np.asarray(T, np.float64).reshape(3, 4)
    return np.hstack([R @ M[:, :3], (R @ M[:, 3] + t)[:, None]])
