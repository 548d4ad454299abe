"""Inputs shared by the tracker-stream tests (tests/test_tracks_host.py, tests/test_gpu_tracks.py): seeded reset_initial cases."""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rotations(rng, n, max_angle):
    """n float32 rotation matrices by Rodrigues' formula evaluated in float32: orthogonal only to float rounding."""
    axis = rng.normal(size=(n, 3)); axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    axis = axis.astype(np.float32)
    ang = rng.uniform(0.0, max_angle, n).astype(np.float32)
    K = np.zeros((n, 3, 3), np.float32)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    s = np.sin(ang).astype(np.float32)[:, None, None]; c = (np.float32(1) - np.cos(ang).astype(np.float32))[:, None, None]
    return (np.eye(3, dtype=np.float32)[None] + s * K + c * (K @ K)).astype(np.float32)


def reset_initial_cases(n=100_000, seed=611):
    """(transform, odometry): (n, 3, 4) float32 each -- the keyframe object's carried transform and the odometry result handed to reset_initial
    (cvo.cpp:611-618).  Rotations up to pi, translations up to a few metres; the first case is the identity pair, a tenth are small motions
    like consecutive frames'."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(2):
        axis_ang = _rotations(rng, n, np.pi)
        small = _rotations(rng, n, 0.05)
        pick = (rng.uniform(size=n) < 0.1)[:, None, None]
        R = np.where(pick, small, axis_ang).astype(np.float32)
        t = (rng.normal(size=(n, 3)) * np.where(pick[:, :, 0], 0.05, 1.5)).astype(np.float32)
        out.append(np.concatenate([R, t[:, :, None]], axis=2).astype(np.float32))
    out[0][0] = np.eye(3, 4, dtype=np.float32); out[1][0] = np.eye(3, 4, dtype=np.float32)
    return np.ascontiguousarray(out[0]), np.ascontiguousarray(out[1])


def oracle_reset_initial(oracle, transform, odometry):
    """The oracle's orc_reset_initial for every case: R (n, 3, 3), T (n, 3), returned inverse (n, 3, 4)."""
    o = oracle.OracleCvo()
    n = transform.shape[0]
    R = np.zeros((n, 3, 3), np.float32); T = np.zeros((n, 3), np.float32); inv = np.zeros((n, 3, 4), np.float32)
    for i in range(n):
        o.reset_transform(transform[i])
        inv[i] = o.reset_initial(odometry[i])
        st = o.get_state()
        R[i] = st["R"]; T[i] = st["T"]
    return R, T, inv
