"""The reading of merging resident maps (include/cvo_hip.h, "Merging maps") on map_reading.Map: the definition the kernels are held to byte for
byte.  It rests on tests/map_reading.py and adds one function and the key's shift:

  kept rows      all_rows: every row of the source, dead ones included; otherwise extract's rule (count >= max(1, min_points), popcount(view_mask)
                 >= min_views, last_stamp >= min_last_stamp), which a dead row never passes
  call-cell      the key with each 21-bit cell field c replaced by ((c - 2^20) >> level) + 2^20, an arithmetic shift; it holds the integer sums of
                 the kept rows' sums and counts, the OR of their view_mask, hi = their largest last_stamp, lo = the least born among those with
                 count >= 1, or among all of them when none has members
  order          call-cells in order of their lowest source row
  into dst       absent: born behind dst's rows with (key, sums, count, mask, last = hi, born = lo); present: sums and count added, mask OR-ed,
                 last = max(last, hi), born = lo when the row was dead and the incoming count is at least 1
  refusals       rows above dst's max_rows, a resulting count above 16777215 (a call-cell's own included): Refused, every map as it was
"""
import numpy as np

import map_reading as mr

MAX_LEVEL = 4
BIAS = 1 << 20


def key_of(c):
    """the 63-bit key of a cell (cx, cy, cz), |c| < 2^20"""
    return ((int(c[0]) + BIAS) << 42) | ((int(c[1]) + BIAS) << 21) | (int(c[2]) + BIAS)


def cell_of(key):
    return tuple(((int(key) >> s) & 0x1FFFFF) - BIAS for s in (42, 21, 0))


def shifted(key, level):
    """the key of the cell at a voxel 2^level times as large (python's >> on a negative integer is arithmetic)"""
    return key_of([c >> level for c in cell_of(key)])


def kept(src, all_rows=True, min_points=1, min_views=0, min_last_stamp=0):
    if all_rows:
        return list(range(src.rows))
    return [r for r in range(src.rows) if src.count[r] >= max(1, min_points) and bin(src.mask[r]).count("1") >= min_views and src.last[r] >= min_last_stamp]


def call_cells(src, level, rows):
    """the call-cells of the kept rows, in order: a list of dict(key, sums, count, mask, hi, lo)"""
    cells, at = [], {}
    for r in rows:
        k = shifted(src.key[r], level)
        if k not in at:
            at[k] = len(cells)
            cells.append(dict(key=k, sums=np.zeros(8, np.int64), count=0, mask=0, hi=0, lo_live=None, lo_all=None))
        c = cells[at[k]]
        c["sums"] = c["sums"] + np.asarray(src.sums[r], np.int64); c["count"] += int(src.count[r]); c["mask"] |= int(src.mask[r])
        c["hi"] = max(c["hi"], int(src.last[r]))
        b = int(src.born[r])
        c["lo_all"] = b if c["lo_all"] is None else min(c["lo_all"], b)
        if src.count[r] >= 1:
            c["lo_live"] = b if c["lo_live"] is None else min(c["lo_live"], b)
    for c in cells:
        c["lo"] = c["lo_all"] if c["lo_live"] is None else c["lo_live"]
    return cells


def check_voxels(dst, src, level):
    if not 0 <= level <= MAX_LEVEL:
        raise ValueError(f"level {level} is outside 0 .. {MAX_LEVEL}")
    if np.float32(np.ldexp(np.float32(src.voxel), level)).tobytes() != np.float32(dst.voxel).tobytes():
        raise ValueError("voxel bits do not match")


def merge(dst, src, level=0, all_rows=True, min_points=1, min_views=0, min_last_stamp=0):
    """the kept rows of src added into dst; Refused leaves dst as it was.  dst and src are map_reading.Maps (not the same one)"""
    assert dst is not src
    check_voxels(dst, src, level)
    cells = call_cells(src, level, kept(src, all_rows, min_points, min_views, min_last_stamp))
    at = [dst.index.get(c["key"], -1) for c in cells]
    if dst.rows + sum(1 for r in at if r < 0) > dst.max_rows:
        raise mr.Refused("rows above max_rows")
    if any(c["count"] + (dst.count[r] if r >= 0 else 0) > mr.MAX_COUNT for c, r in zip(cells, at)):
        raise mr.Refused("count above 16777215")
    for c, r in zip(cells, at):
        if r < 0:
            dst.index[c["key"]] = dst.rows
            dst.key.append(c["key"]); dst.sums.append(c["sums"].copy()); dst.count.append(c["count"]); dst.mask.append(c["mask"])
            dst.last.append(c["hi"]); dst.born.append(c["lo"])
        else:
            if dst.count[r] == 0 and c["count"] >= 1:
                dst.born[r] = c["lo"]
            dst.sums[r] = dst.sums[r] + c["sums"]; dst.count[r] += c["count"]; dst.mask[r] |= c["mask"]; dst.last[r] = max(dst.last[r], c["hi"])
    return dst


def coarser(src, level, max_rows=None):
    """a new Map at ldexp(voxel, level) with every row of src merged in"""
    out = mr.Map(src.max_rows if max_rows is None else max_rows, np.float32(np.ldexp(np.float32(src.voxel), level)))
    return merge(out, src, level)


def copy_of(M):
    out = mr.Map(M.max_rows, M.voxel)
    out.key, out.count, out.mask, out.last, out.born = list(M.key), list(M.count), list(M.mask), list(M.last), list(M.born)
    out.sums = [np.array(q, np.int64) for q in M.sums]
    out.index = dict(M.index)
    return out


# ---- the history the tests share: a window of `window` over the members of map_reading.sliding_windows, plain removal
def window_history(M, members, poses, window=4, upto=None):
    """member m integrated with stamp m, member m - window removed behind it; -> M"""
    for m in range(len(members) if upto is None else upto):
        M.update([members[m]], [poses[m]], [m], 1)
        if m >= window:
            M.update([members[m - window]], [poses[m - window]], [m - window], -1)
    return M
