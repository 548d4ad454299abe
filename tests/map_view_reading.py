"""The reading of a view of a resident map (cvo_maps_view): the definition the kernels are held to byte for byte (include/cvo_hip.h, "Viewing
maps").  It adds nothing of its own: with E the reading's uncapped extract of the map under the view's filter (map_reading.Map.extract) and V
the reading of a view of E's rows (view_reading.view_reading),

  n_out, xyz, feat, pixel, relation, relation_counts, depth   V's
  source          E.row[V.source]
  index           E.row[V.index] where V.index >= 0, -1 elsewhere
  map             -4 everywhere ("filtered or dead") except map[E.row] = V.map
  carve           0 everywhere except at E.row[V.source[V.relation == 1]]

E.row is ascending, so the lowest row number of a z-cell's tie is the lowest extract index: the same front.  The reading also asserts what the
kernels rely on: every kept row's five feature means are below 2^15 (the header's argument), which lets them judge validity by the position alone.
"""
import numpy as np

import fuse_reading as fr
import map_reading as mr
import view_reading as vw
import voxel_reading as vr

FILTERED = -4


def filter_of(min_points=1, min_views=1, min_last_stamp=0):
    return dict(min_points=int(min_points), min_views=int(min_views), min_last_stamp=int(min_last_stamp))


def map_view_reading(M, flt, pose, camera, p, observed=None, E=None):
    """M: map_reading.Map; flt: filter_of(); pose, camera, p, observed: view_reading's.  view_reading's dict with source, index and map in the
    map's row numbers, `carve` (rows,) uint8 with observed, and E and V themselves for the tests' scene conditions.  E: M.extract(**flt), if
    the caller has it already"""
    E = M.extract(**flt) if E is None else E
    assert (np.abs(E["feat"]) < np.float32(32768.0)).all(), "a kept row's feature mean is not below 2^15"
    V = vw.view_reading((E["xyz"], E["feat"]), pose, camera, p, observed)
    row = E["row"].astype(np.int64)
    out = {k: V[k] for k in ("n_out", "xyz", "feat", "pixel", "depth")}
    out["source"] = row[V["source"]].astype(np.int32)
    out["index"] = np.where(V["index"] >= 0, row[np.maximum(V["index"], 0)] if row.size else -1, -1).astype(np.int32)
    m = np.full(M.rows, FILTERED, np.int32); m[row] = V["map"]
    out["map"] = m
    if observed is not None:
        out["relation"] = V["relation"]; out["relation_counts"] = V["relation_counts"]
        carve = np.zeros(M.rows, np.uint8); carve[row[V["source"][V["relation"] == 1]]] = 1
        out["carve"] = carve
    out["E"] = E; out["V"] = V
    return out


def fronts_lost_to(M, flt, clause, pose, camera, p):
    """how many z-cell fronts of the view under `flt` with `clause` (one of its keys) switched off are rows that the clause filters: the clause
    takes away rows that would otherwise be the front"""
    off = dict(flt); off[clause] = {"min_points": 1, "min_views": 0, "min_last_stamp": -2 ** 31}[clause]
    loose = map_view_reading(M, off, pose, camera, p)
    kept = set(M.extract(**flt)["row"].tolist())
    fronts = loose["index"][loose["index"] >= 0]
    return sum(1 for r in fronts.tolist() if r not in kept)


# ---- scenes the CPU and the GPU tests share
VOXEL = 0.05


def valid_walls(rng, n, camera, size):
    """n valid points of view_reading.two_walls (the walls and the points behind the camera; a map takes no invalid point in)"""
    x, f = vw.two_walls(rng, 2 * n + 64, camera, size)
    ok = (np.abs(np.concatenate([x, f], axis=1)) < np.float32(32768.0)).all(axis=1)
    assert ok.sum() >= n
    return np.ascontiguousarray(x[ok][:n]), np.ascontiguousarray(f[ok][:n])


def lattice_member(rng, n, camera, size, voxel=VOXEL):
    """n points of the two walls, each alone in its cell of the `voxel` grid (near the cell's centre): integrated, a map of exactly n rows
    whose row r is point r.  (xyz (n, 3), feat (n, 5))"""
    if n == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 5), np.float32)
    x, f = valid_walls(rng, 3 * n + 64, camera, size)
    c = np.floor(x / np.float32(voxel)).astype(np.int64)
    _, first = np.unique(c, axis=0, return_index=True)
    first = np.sort(first)[:n]
    assert first.shape[0] == n
    centre = (c[first].astype(np.float64) + 0.5 + rng.uniform(-0.2, 0.2, (n, 3))) * voxel
    x = np.ascontiguousarray(centre.astype(np.float32)); f = np.ascontiguousarray(f[first])
    ok, _, key = vr.cells(vr.points8(x, f), voxel)
    assert ok.all() and np.unique(key).shape[0] == n
    return x, f


def wall_windows(rng, camera, size, members=6, n=4000, stride=0.15, width=0.5, noise=0.004):
    """map_reading.sliding_windows over the two walls: member m holds the valid points whose image column lies in a band of `width` of the image
    starting at stride * m - 0.2 (the walls reach a fifth beyond either border), with noise, in a camera frame of its own.  Neighbours share
    most of their cells; the poses bring every member back into the scene's frame.  ([(xyz, feat)], [4 x 4 pose])"""
    bx, bf = valid_walls(rng, n, camera, size)
    s, fx, fy, cx, cy = camera
    u = (bx[:, 0] * fx / np.abs(bx[:, 2]) + cx) / size[0]
    out, poses = [], []
    for m in range(members):
        lo = -0.2 + stride * m
        pick = (u >= lo) & (u < lo + width)
        x = bx[pick] + rng.normal(scale=noise, size=(int(pick.sum()), 3)).astype(np.float32)
        P = fr.rigid(rng, 0.1, 0.2)
        inv = np.linalg.inv(P.astype(np.float64))
        out.append((np.ascontiguousarray((x @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)), np.ascontiguousarray(bf[pick]))); poses.append(P)
    return out, poses


def scene(which):
    """what the GPU tests view into the small (64 x 48) or the wide (100 x 70) image: dict(size, camera, lattice {n: (xyz, feat)} for n in
    view_reading.SCENE_SIZES, poses: 8 small rigid moves, windows: (members, poses) of wall_windows)"""
    size, camera, seed = {"small": (vw.SIZE_SMALL, vw.CAM_SMALL, 51), "wide": (vw.SIZE_WIDE, vw.CAM_WIDE, 52)}[which]
    rng = np.random.default_rng(seed)
    lattice = {n: lattice_member(rng, n, camera, size) for n in vw.SCENE_SIZES}
    poses = [fr.rigid(rng, 0.03, 0.05) for _ in range(8)]
    return dict(size=size, camera=camera, lattice=lattice, poses=poses, windows=wall_windows(rng, camera, size))


def history(windows, max_rows=20000, voxel=VOXEL):
    """a map with a history on wall_windows' members: 0 .. 3 go in one by one with stamps 0 .. 3, member 1 is removed (rows die, counts and
    views fall), member 4 goes in with stamp 9.  The steps as (sign, member, stamp), and the reading's map after them"""
    steps = [(1, 0, 0), (1, 1, 1), (1, 2, 2), (1, 3, 3), (-1, 1, 1), (1, 4, 9)]
    members, poses = windows
    M = mr.Map(max_rows, voxel)
    for sign, m, st in steps:
        M.update([members[m]], [poses[m]], [st], sign)
    return steps, M


# the filters of the "dead rows and filters" tests: each clause alone, and all three
FILTERS = (filter_of(1, 0, -2 ** 31), filter_of(2, 0, -2 ** 31), filter_of(1, 2, -2 ** 31), filter_of(1, 0, 3), filter_of(2, 2, 2))
CLAUSE_OF = {1: "min_points", 2: "min_views", 3: "min_last_stamp"}     # the clause that FILTERS[k] has alone


# ---- past the extract's cap: the construction of test_maps_past_65536_rows -- three clouds of about 30 000 points uniform in an 8 m cube fill
# some 70 000 cells of 0.145 m -- seen from 5.5 m in front of the cube's centre into 320 x 240
PAST_VOXEL, PAST_MAX_ROWS, PAST_SIZE, PAST_CAMERA = 0.145, 80000, (320, 240), (5000.0, 262.5, 262.5, 159.5, 119.5)
PAST_POSE = np.array([[1, 0, 0, 0.1], [0, 1, 0, -0.05], [0, 0, 1, 5.5]], np.float32)


def past_the_cap():
    """(members, poses): one integration of them makes a map whose loosest filter keeps more than 65 535 rows"""
    rng = np.random.default_rng(75)
    members = []
    for k, n in enumerate((30001, 29999, 30003)):
        r = np.random.default_rng(90 + k)
        members.append((r.uniform(-4.0, 4.0, (n, 3)).astype(np.float32), r.uniform(0.0, 255.0, (n, 5)).astype(np.float32)))
    return members, [fr.rigid(rng, 0.05, 0.1) for _ in members]
