"""The dense numpy reading of the voxel-grid reduction (cvo_reduce_device_clouds): the definition the kernels are held to bit for bit.

One cloud: n points of 3 position and 5 feature floats, a voxel size (f32, finite, > 0), a mode and min_points >= 1.
  valid point : its 8 floats are finite and below 2^15 in magnitude, and each c = floorf(x / voxel) (correctly rounded f32 division, floor not
                truncation) has |c| < 2^20.  Invalid points belong to no cell.
  cell        : the integer triple (cx, cy, cz); its members are the valid points with that triple; cells with fewer than min_points members
                are dropped.
  row order   : ascending lowest member index; count[r] is the member count.
  MEAN        : every member value v becomes q = llrint((double)v * 2^24); the q are added as 64-bit integers; the row's value is
                (float)((double)sum / ((double)count * 16777216.0)).  source[r] is the lowest member index.
  CENTRAL     : the row is a copy of the member nearest the cell's centre (c + 0.5f) * voxel (f32); d2 = dx*dx + dy*dy + dz*dz in f32, un-fused,
                added in that order; the least (d2 bits, index) wins, so a tie goes to the lowest index.  source[r] is that member's index.
  map[i]      : the row of point i's cell, -1 for an invalid point or a dropped cell.
"""
import numpy as np

MEAN, CENTRAL = 0, 1
MODES = {"mean": MEAN, "central": CENTRAL}


def points8(xyz, feat):
    """(n, 8) float32: positions, then features (feat is (n, 5), points first)"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3); feat = np.asarray(feat, np.float32).reshape(-1, 5)
    assert xyz.shape[0] == feat.shape[0]
    return np.ascontiguousarray(np.concatenate([xyz, feat], axis=1))


def cells(P, voxel):
    """(valid (n,) bool, c (n, 3) float32 cell coordinates (0 where invalid), key (n,) int64: the three coordinates + 2^20 in 21 bits each)"""
    v = np.float32(voxel)
    assert np.isfinite(v) and v > 0
    with np.errstate(all="ignore"):
        ok = (np.abs(P) < np.float32(32768.0)).all(axis=1)              # (NaN and inf compare false)
        c = np.floor(P[:, :3] / v).astype(np.float32)
        ok &= (np.abs(c) < np.float32(1048576.0)).all(axis=1)
    c = np.where(ok[:, None], c, np.float32(0)).astype(np.float32)
    ci = c.astype(np.int64) + (1 << 20)
    return ok, c, (ci[:, 0] << 42) | (ci[:, 1] << 21) | ci[:, 2]


def reduce_reading(xyz, feat, voxel, mode=MEAN, min_points=1):
    """dict(xyz (rows, 3) f32, feat (rows, 5) f32, count, source (rows,) i32, map (n,) i32, n_out)"""
    mode = MODES.get(mode, mode)
    assert mode in (MEAN, CENTRAL) and min_points >= 1
    P = points8(xyz, feat); n = P.shape[0]
    ok, c, key = cells(P, voxel)
    idx = np.flatnonzero(ok)
    _, first, inv, cnt = np.unique(key[idx], return_index=True, return_inverse=True, return_counts=True)
    lowest = idx[first]                                                  # (unique's first occurrence: the lowest member index)
    keep = cnt >= min_points
    order = np.argsort(lowest[keep], kind="stable")
    kept = np.flatnonzero(keep)[order]                                   # cells in row order
    rows = kept.shape[0]
    row_of_cell = np.full(cnt.shape[0], -1, np.int64); row_of_cell[kept] = np.arange(rows)
    map_ = np.full(n, -1, np.int32); map_[idx] = row_of_cell[inv.reshape(-1)]
    m = np.flatnonzero(map_ >= 0)
    count = cnt[kept].astype(np.int32)
    if mode == MEAN:
        with np.errstate(all="ignore"):                                  # (invalid points have no q that counts)
            q = np.rint(P.astype(np.float64) * 16777216.0).astype(np.int64)
        sums = np.zeros((rows, 8), np.int64)
        np.add.at(sums, map_[m], q[m])
        out = (sums.astype(np.float64) / (count.astype(np.float64) * 16777216.0)[:, None]).astype(np.float32)
        source = lowest[kept].astype(np.int32)
    else:
        v = np.float32(voxel)
        with np.errstate(all="ignore"):
            d = P[:, :3] - (c + np.float32(0.5)) * v
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        rank = (np.ascontiguousarray(d2, np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
        best = np.full(rows, np.iinfo(np.uint64).max, np.uint64)
        np.minimum.at(best, map_[m], rank[m])
        source = (best & np.uint64(0xFFFFFFFF)).astype(np.int32)
        out = P[source]
    return dict(xyz=np.ascontiguousarray(out[:, :3]), feat=np.ascontiguousarray(out[:, 3:]), count=count, source=source, map=map_, n_out=rows)


def count_reading(xyz, feat, voxel, min_points=1):
    """the occupied-cell count: cells with at least min_points members"""
    P = points8(xyz, feat)
    ok, _, key = cells(P, voxel)
    _, cnt = np.unique(key[ok], return_counts=True)
    return int((cnt >= min_points).sum())
