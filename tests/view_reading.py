"""The dense numpy reading of a view (cvo_view_device_clouds): the definition the kernels are held to byte for byte (include/cvo_hip.h, "Viewing
clouds").  Every step is float32 and rounded where the header says so: numpy float32 arrays against float32 scalars round each product,
quotient and sum.

  moved position  support_reading.move: x' = (M[r,0]*x + (M[r,1]*y + M[r,2]*z)) + M[r,3], the fuser's rule
  valid           the 8 source floats and the 3 moved floats finite and below 2^15
  in view         z_near <= z' <= z_far; u = (x' * fx) / z' + cx, v = (y' * fy) / z' + cy, both below 2^20; px = floor(u + 0.5), py likewise,
                  inside the image
  z-cell          (px // cell, py // cell), numbered (py // cell) * gw + px // cell
  front           the least uint64 key (bits of z' << 32) | index of a z-cell: np.minimum.at
  visible         FRONT: the fronts.  SURFACE: z' <= zf + slack * zf
  rows            the visible points in input order
"""
import numpy as np

import fuse_reading as fr
import support_reading as sup
import voxel_reading as vr

FRONT, SURFACE = 0, 1
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
f32 = np.float32

# (scaling_factor, fx, fy, cx, cy) of the two image sizes the GPU tests view into
SIZE_SMALL, CAM_SMALL = (64, 48), (5000.0, 58.3, 57.1, 31.2, 23.7)
SIZE_WIDE, CAM_WIDE = (100, 70), (1000.0, 95.3, 96.1, 48.7, 36.2)


def params(width, height, cell=1, mode=FRONT, slack=0.0, z_near=0.05, z_far=30.0, depth_tol=0.02):
    """cvo_view_params as a dict"""
    assert 1 <= width <= 8192 and 1 <= height <= 8192 and 1 <= cell <= 16 and mode in (FRONT, SURFACE)
    assert 0 < z_near < z_far <= 32768.0 and slack >= 0 and depth_tol >= 0
    return dict(width=int(width), height=int(height), cell=int(cell), mode=int(mode), slack=f32(slack), z_near=f32(z_near), z_far=f32(z_far),
                depth_tol=f32(depth_tol))


def grid(p):
    return -(-p["width"] // p["cell"]), -(-p["height"] // p["cell"])


def project(moved, valid, camera, p):
    """(in_view (n,) bool, px (n,), py (n,) int64 -- 0 where not in view) of moved positions"""
    s, fx, fy, cx, cy = (f32(v) for v in camera)
    z = moved[:, 2]
    with np.errstate(all="ignore"):
        ok = valid & (p["z_near"] <= z) & (z <= p["z_far"])
        u = (moved[:, 0] * fx) / z + cx
        v = (moved[:, 1] * fy) / z + cy
        ok &= (np.abs(u) < f32(1048576.0)) & (np.abs(v) < f32(1048576.0))
        fu = np.floor(u + f32(0.5)); fv = np.floor(v + f32(0.5))
    px = np.where(ok, fu, 0).astype(np.int64); py = np.where(ok, fv, 0).astype(np.int64)
    ok &= (px >= 0) & (px < p["width"]) & (py >= 0) & (py < p["height"])
    return ok, np.where(ok, px, 0), np.where(ok, py, 0)


def relation_of(z, d, camera, depth_tol):
    """the relation of rows with depth z (n,) float32 to the observed uint16 d (n,)"""
    s = f32(camera[0])
    zo = d.astype(f32) / s
    t = f32(depth_tol) * zo
    rel = np.where(z < zo - t, 1, np.where(z > zo + t, 3, 2))
    return np.where(d == 0, 0, rel).astype(np.int32)


def view_reading(cloud, pose, camera, p, observed=None):
    """cloud: (xyz (n, 3), feat (n, 5)); pose 3 x 4 or 4 x 4; camera (scaling_factor, fx, fy, cx, cy); p: params(); observed: uint16 (h, w) or
    None.  dict(xyz, feat, source, pixel, map, depth (gh, gw), index (gh, gw), n_out[, relation, relation_counts])"""
    P = vr.points8(*cloud)
    n = P.shape[0]
    gw, gh = grid(p)
    with np.errstate(all="ignore"):
        moved = sup.move(fr.pose34(pose), P[:, :3]).reshape(-1, 3)
        valid = (np.abs(P) < f32(32768.0)).all(axis=1) & (np.abs(moved) < f32(32768.0)).all(axis=1)
    inview, px, py = project(moved, valid, camera, p)
    cell = (py // p["cell"]) * gw + px // p["cell"]
    z = np.ascontiguousarray(moved[:, 2])
    key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    zb = np.full(gw * gh, EMPTY, np.uint64)
    np.minimum.at(zb, cell[inview], key[inview])
    front = zb[cell]                                                   # (of cell 0 where not in view: masked below)
    if p["mode"] == FRONT:
        vis = inview & ((front & np.uint64(0xFFFFFFFF)) == np.arange(n, dtype=np.uint64))
    else:
        zf = (front >> np.uint64(32)).astype(np.uint32).view(f32)
        with np.errstate(all="ignore"):
            vis = inview & (z <= zf + p["slack"] * zf)
    rows = np.flatnonzero(vis)
    m = np.where(valid, -2, -3).astype(np.int32)
    m[inview] = -1
    m[rows] = np.arange(rows.shape[0], dtype=np.int32)
    filled = zb != EMPTY
    depth = np.where(filled, (zb >> np.uint64(32)).astype(np.uint32).view(f32), f32(0.0)).astype(f32).reshape(gh, gw)
    index = np.where(filled, (zb & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32).reshape(gh, gw)
    out = dict(xyz=np.ascontiguousarray(moved[rows]), feat=np.ascontiguousarray(P[rows, 3:]), source=rows.astype(np.int32),
               pixel=(py[rows] * p["width"] + px[rows]).astype(np.int32), map=m, depth=np.ascontiguousarray(depth), index=np.ascontiguousarray(index),
               n_out=int(rows.shape[0]))
    if observed is not None:
        obs = np.asarray(observed, np.uint16)
        assert obs.shape == (p["height"], p["width"])
        out["relation"] = relation_of(z[rows], obs[py[rows], px[rows]], camera, p["depth_tol"])
        out["relation_counts"] = np.bincount(out["relation"], minlength=4).astype(np.int32)
    return out


def shares(cloud, pose, camera, p):
    """(hidden share of the in-view points, outside share of the valid points, invalid share of all points) of a view"""
    m = view_reading(cloud, pose, camera, p)["map"]
    inview = (m >= -1).sum(); valid = (m >= -2).sum()
    return (m == -1).sum() / max(1, inview), (m == -2).sum() / max(1, valid), (m == -3).sum() / max(1, m.shape[0])


# ---- scenes the view tests share
def two_walls(rng, n, camera, size):
    """n points in the camera's frame: a wavy back wall about 3 m away over the whole image and a fifth beyond each border (0.55 n), a nearer
    wall at about 1.5 m over the middle 80 % of either side (0.33 n), points behind the camera (0.06 n) and points with a NaN, an inf or a 2^15
    among their 8 floats (the rest), shuffled.  (xyz (n, 3), feat (n, 5))"""
    s, fx, fy, cx, cy = camera
    w, h = size
    kind = rng.choice(4, n, p=[0.55, 0.33, 0.06, 0.06])
    wide = kind != 1
    u = np.where(wide, rng.uniform(-0.2 * w, 1.2 * w, n), rng.uniform(0.1 * w, 0.9 * w, n))
    v = np.where(wide, rng.uniform(-0.2 * h, 1.2 * h, n), rng.uniform(0.1 * h, 0.9 * h, n))
    z = np.where(kind == 1, 1.5 + 0.05 * np.sin(u / 7.0), 3.0 + 0.1 * np.sin(u / 9.0) * np.cos(v / 5.0))
    z = np.where(kind == 2, -z, z)
    x = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], axis=1).astype(f32)
    f = rng.uniform(0, 255, (n, 5)).astype(f32)
    P = np.concatenate([x, f], axis=1)
    bad = np.flatnonzero(kind == 3)
    vals = np.array([np.nan, np.inf, -np.inf, 32768.0, -40000.0], f32)
    P[bad, rng.integers(0, 8, bad.shape[0])] = vals[rng.integers(0, 5, bad.shape[0])]
    return np.ascontiguousarray(P[:, :3]), np.ascontiguousarray(P[:, 3:])


SCENE_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 3000)                 # empty, one point, wave edges, block edges, many blocks
# the two calls of 8 views each that cover SCENE_SIZES; the 3000-point cloud goes into two views of either call, under different poses
SCENE_CALLS = ((0, 1, 63, 64, 65, 255, 3000, 3000), (256, 257, 3000, 3000, 65, 1, 0, 255))
SHARES_AT = dict(cell=3, mode=SURFACE, slack=0.05)                    # where the scene conditions of tests/test_view_reading.py are taken


def scene(which):
    """the scene the GPU tests view into the small (64 x 48) or the wide (100 x 70) image: dict(size, camera, clouds {n: (xyz, feat)} for n in
    SCENE_SIZES, poses: 8 small rigid moves, one per view of a call)"""
    size, camera, seed = {"small": (SIZE_SMALL, CAM_SMALL, 31), "wide": (SIZE_WIDE, CAM_WIDE, 32)}[which]
    rng = np.random.default_rng(seed)
    clouds = {n: two_walls(rng, n, camera, size) for n in SCENE_SIZES}
    return dict(size=size, camera=camera, clouds=clouds, poses=[fr.rigid(rng, 0.03, 0.05) for _ in range(8)])


# ---- the edges of the definition, point by point: under the identity pose, EDGE_CAM (u = 64 x / z + 32, v = 64 y / z + 24: exact in f32 for
# these points) and EDGE_SIZE, with z_range (0.05, 30) unless said otherwise
EDGE_SIZE, EDGE_CAM = (64, 48), (1000.0, 64.0, 64.0, 32.0, 24.0)
EDGE_FAR_MOVE = np.array([[1, 0, 0, 32767.5], [0, 1, 0, 0], [0, 0, 1, 0]], f32)   # x' reaches 2^15 for x >= 0.5


def edge_cloud():
    """(xyz (n, 3), feat (n, 5), names): names[i] says what point i is there for"""
    down = lambda v: np.nextafter(f32(v), f32(-np.inf)); up = lambda v: np.nextafter(f32(v), f32(np.inf))
    xl, xr = f32((-0.5 - 32) / 64), f32((63.5 - 32) / 64)             # u = -0.5: px 0; u = 63.5: px 64
    yt, yb = f32((-0.5 - 24) / 64), f32((47.5 - 24) / 64)
    pts = [("u = -0.5: inside, px 0", (xl, 0, 1)), ("u just below -0.5: outside", (down(xl), 0, 1)),
           ("u = width - 0.5: outside", (xr, 0, 1)), ("u two steps below width - 0.5 (one step sums to a tie that rounds up): inside, px 63", (down(down(xr)), 0, 1)),
           ("v = -0.5: inside, py 0", (0.25, yt, 1)), ("v just below -0.5: outside", (0.25, down(yt), 1)),
           ("v = height - 0.5: outside", (0.25, yb, 1)), ("v two steps below height - 0.5: inside, py 47", (0.25, down(down(yb)), 1)),
           ("z' = z_near: in range", (0, 0, f32(0.05))), ("z' just below z_near: out of range", (0, 0, down(0.05))),
           ("z' = z_far: in range, px 40", (3.75, 0, f32(30.0))), ("z' just above z_far: out of range", (3.75, 0, up(30.0))),
           ("twin a: the front", (0.1, 0.1, 2)), ("twin b: same pixel, same z', higher index", (0.1, 0.1, 2)),
           ("behind the twins by a quarter", (0.125, 0.125, 2.5)), ("behind the twins by 2.5 %", (0.1025, 0.1025, 2.05)),
           ("z' tiny: |u| past 2^20", (1.0, 0, f32(2e-6))), ("z' tiny, on the axis", (0, 0, f32(2e-6))),
           ("NaN", (np.nan, 0, 1)), ("a source float past 2^15", (0.2, 40000.0, 1)), ("x' past 2^15 under EDGE_FAR_MOVE", (0.75, 0.1, 1)),
           ("x' below 2^15 under EDGE_FAR_MOVE", (0.25, -0.1, 1))]
    xyz = np.array([p for _, p in pts], f32)
    feat = np.arange(5 * len(pts), dtype=f32).reshape(-1, 5)
    feat[18, 2] = np.inf                                               # ("NaN" has a bad feature too)
    return xyz, feat, [name for name, _ in pts]


def shifted_rendering(cloud, pose, camera, size):
    """an observed depth image for the relation tests: the scene's own FRONT rendering at cell 1 as uint16, cut into four bands of columns --
    as rendered (agrees), 1.2 times deeper (the points are in front), 0.8 times (behind), and no depth at all (unknown)"""
    w, h = size
    z = view_reading(cloud, pose, camera, params(w, h))["depth"]
    d = np.rint(z.astype(np.float64) * camera[0])
    band = (np.arange(w) * 4) // w
    d = d * np.array([1.0, 1.2, 0.8, 0.0])[band][None, :]
    assert d.max() < 65535
    return np.ascontiguousarray(d.astype(np.uint16))
