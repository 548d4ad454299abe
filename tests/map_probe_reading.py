"""The reading of a probe of a resident map (cvo_maps_probe_clouds / cvo_maps_probe_frames): the definition the kernel is held to byte for byte
(include/cvo_hip.h, "Probing maps").  It rests on the readings below it and adds nothing of its own:

  the member's points   fuse_reading.moved_concat of the one posed member (a frame: frame_reading.dense_reading's cloud): the moved positions,
                        NaN where a source float is bad
  validity and cell     voxel_reading.cells at the map's voxel; an invalid point has row -3
  the map               map_reading.Map: its dict key -> row, and Map.extract under the probe's filter for the kept rows and their means
  reach 0               the point's own cell: no row -1, a row the filter drops -4, else the row
  reach 1               the 27 cells around it, those with a coordinate of magnitude 2^20 or more skipped; among the kept rows the least
                        (d2 bits, row) wins, d2 = (dx*dx + dy*dy) + dz*dz in f32 with dx = x' - mean_x; none kept: -4 if a cell had a row, else -1
  dist2, count, views, last_stamp   the winner's (inf bits and zeros where row < 0); hit: a byte per map row, 1 where a point has that row
  counts                found, absent (-1), filtered (-4), invalid (-3)

The reading also asserts what the kernel relies on: every kept row's feature means are below 2^15 (the header's argument under "Viewing maps").
"""
import numpy as np

import frame_reading as frd
import fuse_reading as fr
import voxel_reading as vr

ABSENT, INVALID, FILTERED = -1, -3, -4
INF_BITS = 0x7F800000
OFFSETS_27 = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]


def frame_member(bgr, depth, camera, step=1):
    """a frame as a probe's member: its dense cloud"""
    return frd.dense_reading(bgr, depth, camera, step)


def probe_reading(M, flt, member, pose, reach=0):
    """M: map_reading.Map; flt: dict(min_points, min_views, min_last_stamp); member: (xyz (n, 3), feat (n, 5)); pose: 3 x 4 or 4 x 4.
    dict(row, count, views, last_stamp (n,) i32, dist2 (n,) f32, hit (M.rows,) u8, counts (4,) i32, moved (n, 3) f32, cell (n, 3) i64, valid)"""
    assert reach in (0, 1)
    xyz, feat, _, _ = fr.moved_concat([member], [pose])
    ok, c, _ = vr.cells(vr.points8(xyz, feat), M.voxel)
    n = xyz.shape[0]
    E = M.extract(**flt)
    assert (np.abs(E["feat"]) < np.float32(32768.0)).all() and (np.abs(E["xyz"]) < np.float32(32768.0)).all(), "a kept row's mean is not below 2^15"
    kept = np.zeros(M.rows, bool); kept[E["row"]] = True
    mean = np.zeros((M.rows, 3), np.float32); mean[E["row"]] = E["xyz"]
    keys = np.asarray(M.key, np.int64).reshape(-1)
    order = np.argsort(keys, kind="stable"); sk = keys[order]

    def rows_of(k):
        if sk.size == 0:
            return np.full(k.shape, -1, np.int64)
        pos = np.minimum(np.searchsorted(sk, k), sk.size - 1)
        return np.where(sk[pos] == k, order[pos], -1)

    ci = c.astype(np.int64)
    none = np.iinfo(np.uint64).max
    best = np.full(n, none, np.uint64); any_row = np.zeros(n, bool)
    for d in ([(0, 0, 0)] if reach == 0 else OFFSETS_27):
        nb = ci + np.asarray(d, np.int64)
        look = ok & (np.abs(nb) < (1 << 20)).all(axis=1)               # a neighbour outside the grid is in no map: its key is never formed
        shifted = np.where(look[:, None], nb, 0) + (1 << 20)
        r = np.where(look, rows_of((shifted[:, 0] << 42) | (shifted[:, 1] << 21) | shifted[:, 2]), -1)
        any_row |= r >= 0
        k = (r >= 0) & kept[np.maximum(r, 0)] if M.rows else np.zeros(n, bool)
        with np.errstate(all="ignore"):
            dv = xyz - mean[np.maximum(r, 0)] if M.rows else xyz
            d2 = ((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2]).astype(np.float32)
        cand = (np.ascontiguousarray(d2).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.maximum(r, 0).astype(np.uint64)
        best = np.where(k & (cand < best), cand, best)
    found = best != none
    row = np.where(found, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), np.where(any_row, FILTERED, ABSENT))
    row = np.where(ok, row, INVALID).astype(np.int32)
    at = np.maximum(row, 0)
    bits = np.where(found & ok, (best >> np.uint64(32)).astype(np.uint32), np.uint32(INF_BITS)).astype(np.uint32)
    count = np.asarray(M.count, np.int64).reshape(-1); last = np.asarray(M.last, np.int64).reshape(-1)
    views = np.asarray([bin(m).count("1") for m in M.mask], np.int64).reshape(-1)
    pick = lambda a: np.where(row >= 0, a[at] if M.rows else 0, 0).astype(np.int32)
    hit = np.zeros(M.rows, np.uint8); hit[row[row >= 0]] = 1
    counts = np.asarray([(row >= 0).sum(), (row == ABSENT).sum(), (row == FILTERED).sum(), (row == INVALID).sum()], np.int32)
    return dict(row=row, dist2=bits.view(np.float32), count=pick(count), views=pick(views), last_stamp=pick(last), hit=hit, counts=counts,
                moved=xyz, cell=ci, valid=ok)
