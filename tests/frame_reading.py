"""The dense numpy reading of a frame read in place (cvo_hip.h, "Reducing frames"): the definition the frame kernels are held to bit for bit.

A frame is a colour image (h, w, 3) uint8 in B, G, R order, a depth image (h, w) uint16, a camera (scaling_factor, fx, fy, cx, cy) and a step
in 1 .. 16.  With ws = ceil(w / step), hs = ceil(h / step) the dense cloud has n = ws * hs points; point i is pixel
(x, y) = ((i % ws) * step, (i // ws) * step), p = y * w + x its flat index.
  position : z = (float)d / scaling_factor; X = ((float)x - cx) * z / fx; Y = ((float)y - cy) * z / fy -- f32, each operation rounded, in this
             order.  d == 0: X = Y = Z = quiet NaN (0x7FC00000).
  features : B, G, R as floats; then the generator's level-0 gradients on the FLAT index: I[q] = (float)((B*4899 + G*9617 + R*1868 + 8192) >> 14),
             and for w <= p < w*(h-1): dx = 0.5f*(I[p+1] - I[p-1]), dy = 0.5f*(I[p+w] - I[p-w]); elsewhere 0.  Rows are not special: at x = 0 the
             left neighbour is the previous row's last pixel.  Gradients come from the full-resolution neighbours whatever the step.
"""
import numpy as np

QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def sub_grid(w, h, step=1):
    """(ws, hs, x (n,), y (n,)) of the sub-grid's pixels in point order"""
    assert 1 <= step <= 16
    ws, hs = -(-w // step), -(-h // step)
    i = np.arange(ws * hs)
    return ws, hs, (i % ws) * step, (i // ws) * step


def gray(bgr):
    """(h * w,) float32: the generator's 8-bit gray of every pixel, by flat index"""
    c = np.asarray(bgr, np.uint8).reshape(-1, 3).astype(np.int64)
    return ((c[:, 0] * 4899 + c[:, 1] * 9617 + c[:, 2] * 1868 + 8192) >> 14).astype(np.float32)


def gradients(bgr):
    """(dx, dy), each (h * w,) float32, by flat index"""
    h, w = bgr.shape[:2]
    I = gray(bgr)
    dx = np.zeros(w * h, np.float32); dy = np.zeros(w * h, np.float32)
    p = np.arange(w, w * (h - 1))
    dx[p] = np.float32(0.5) * (I[p + 1] - I[p - 1])
    dy[p] = np.float32(0.5) * (I[p + w] - I[p - w])
    return dx, dy


def dense_reading(bgr, depth, camera, step=1):
    """(xyz (n, 3) float32, feat (n, 5) float32) of the frame's dense cloud"""
    bgr = np.asarray(bgr, np.uint8); depth = np.asarray(depth, np.uint16)
    h, w = depth.shape
    assert bgr.shape == (h, w, 3)
    s, fx, fy, cx, cy = (np.float32(v) for v in camera)
    ws, hs, x, y = sub_grid(w, h, step)
    p = y * w + x
    d = depth.reshape(-1)[p]
    with np.errstate(all="ignore"):
        z = d.astype(np.float32) / s
        X = (x.astype(np.float32) - cx) * z / fx
        Y = (y.astype(np.float32) - cy) * z / fy
    xyz = np.stack([X, Y, z], axis=1).astype(np.float32)
    xyz[d == 0] = QNAN
    dx, dy = gradients(bgr)
    feat = np.concatenate([bgr.reshape(-1, 3)[p].astype(np.float32), dx[p, None], dy[p, None]], axis=1)
    return np.ascontiguousarray(xyz), np.ascontiguousarray(feat, np.float32)


def rows_of_pixels(w, h, step, px):
    """the dense cloud's row of every pixel px (m, 2) = (x, y) of the sub-grid"""
    px = np.asarray(px).astype(np.int64)
    assert (px % step == 0).all()
    return (px[:, 1] // step) * (-(-w // step)) + px[:, 0] // step
