"""The numpy and dict reading of resident maps (cvo_maps): the definition the kernels are held to byte for byte (include/cvo_hip.h, "Resident
maps").  It rests on the two readings below it and adds only what is new:

  a map          an ordered list of rows -- key, 8 int64 sums of llrint(v * 2^24), count, view_mask, last_stamp, born -- and a dict key -> row
  the call's own cells   of a group of posed members: voxel_reading.cells over fuse_reading.moved_concat, the cells in order of their lowest
                 global index, each with its sums, its member count and the set of member numbers that touched it
  integrate      a cell whose key is in the map is added to its row (count += members, view_mask |= bits of stamp & 63, last_stamp = max, born =
                 least stamp when the row was dead); an absent one is born behind the map's rows, in the call's order
  remove         the same subtracted; the stamps' bits cleared; last_stamp and born stay; count 0 is a dead row that keeps its place and key
  remove what is still there (sign -2)   per call-cell with B the bits of the stamps that touched it: key absent, or the row's mask has none
                 of B: skipped; all of B: removed; some of B: Refused
  refusals       rows above max_rows, a count above 16777215, a removal of an absent cell or of more members than the count: Refused, the
                 map as it was
  extract        rows with count >= max(1, min_points), popcount(view_mask) >= min_views, last_stamp >= min_last_stamp, in row order;
                 values (float)((double)sum / ((double)count * 16777216.0))
  compact        a row stays when count >= 1, last_stamp >= min_last_stamp, (views >= min_views or born >= probation_from), and not drop[row]
"""
import numpy as np

import fuse_reading as fr
import voxel_reading as vr

MAX_COUNT = 16777215


class Refused(Exception):
    pass


def call_cells(members, poses, voxel):
    """the group's own cells in rank order: (keys (c,) int64, sums (c, 8) int64, counts (c,) int64, touched: list of sorted member numbers)"""
    xyz, feat, member, _ = fr.moved_concat(members, poses)
    P = vr.points8(xyz, feat)
    ok, _, key = vr.cells(P, voxel)
    idx = np.flatnonzero(ok)
    if idx.size == 0:
        return np.zeros(0, np.int64), np.zeros((0, 8), np.int64), np.zeros(0, np.int64), []
    uniq, first, inv = np.unique(key[idx], return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(first, kind="stable")                             # ascending lowest global index
    rank = np.empty_like(order); rank[order] = np.arange(order.shape[0])
    cell = rank[inv]                                                     # the rank of each valid point's cell
    with np.errstate(all="ignore"):
        q = np.rint(P[idx].astype(np.float64) * 16777216.0).astype(np.int64)
    sums = np.zeros((uniq.shape[0], 8), np.int64)
    np.add.at(sums, cell, q)
    counts = np.bincount(cell, minlength=uniq.shape[0]).astype(np.int64)
    touched = [[] for _ in range(uniq.shape[0])]
    for m in np.unique(member[idx]).tolist():
        for c in np.unique(cell[member[idx] == m]).tolist():
            touched[c].append(m)
    return uniq[order], sums, counts, touched


class Map:
    def __init__(self, max_rows, voxel):
        self.max_rows, self.voxel = int(max_rows), np.float32(voxel)
        self.clear()

    def clear(self):
        self.key, self.sums, self.count, self.mask, self.last, self.born, self.index = [], [], [], [], [], [], {}

    @property
    def rows(self):
        return len(self.key)

    @property
    def live(self):
        return sum(1 for c in self.count if c >= 1)

    def update(self, members, poses, stamps, sign=1):
        """integrate (sign 1) or remove (sign -1) one group; Refused leaves the map as it was"""
        assert sign in (1, -1, -2) and len(stamps) == len(members) and all(int(s) >= 0 for s in stamps)
        keys, sums, counts, touched = call_cells(members, poses, self.voxel)
        at = [self.index.get(int(k), -1) for k in keys.tolist()]
        if sign == -2:                                                   # what is gone, or was made again by others, is skipped
            for c, r in enumerate(at):
                if r < 0:
                    continue
                bits = 0
                for m in touched[c]:
                    bits |= 1 << (int(stamps[m]) & 63)
                have = self.mask[r] & bits
                if have == 0:
                    at[c] = -1
                elif have != bits:
                    raise Refused("partly present")
        if sign > 0:
            if self.rows + sum(1 for r in at if r < 0) > self.max_rows:
                raise Refused("rows above max_rows")
            if any(r >= 0 and self.count[r] + int(c) > MAX_COUNT for r, c in zip(at, counts.tolist())):
                raise Refused("count above 16777215")
        else:
            if sign == -1 and any(r < 0 for r in at):
                raise Refused("absent cell")
            if any(r >= 0 and int(c) > self.count[r] for r, c in zip(at, counts.tolist())):
                raise Refused("more members than the count")
        for c, (k, r) in enumerate(zip(keys.tolist(), at)):
            st = [int(stamps[m]) for m in touched[c]]
            bits = 0
            for s in st:
                bits |= 1 << (s & 63)
            if r < 0 and sign < 0:
                continue
            if r < 0:
                self.index[int(k)] = self.rows
                self.key.append(int(k)); self.sums.append(sums[c].copy()); self.count.append(int(counts[c])); self.mask.append(bits)
                self.last.append(max(st)); self.born.append(min(st))
            elif sign > 0:
                if self.count[r] == 0:
                    self.born[r] = min(st)
                self.sums[r] = self.sums[r] + sums[c]; self.count[r] += int(counts[c]); self.mask[r] |= bits; self.last[r] = max(self.last[r], max(st))
            else:
                self.sums[r] = self.sums[r] - sums[c]; self.count[r] -= int(counts[c]); self.mask[r] &= ~bits

    def _arrays(self, keep):
        n = len(keep)
        sums = np.asarray([self.sums[r] for r in keep], np.int64).reshape(n, 8)
        count = np.asarray([self.count[r] for r in keep], np.int64)
        with np.errstate(all="ignore"):
            out = (sums.astype(np.float64) / (count.astype(np.float64) * 16777216.0)[:, None]).astype(np.float32)
        mask = np.asarray([self.mask[r] for r in keep], np.uint64)
        return dict(xyz=np.ascontiguousarray(out[:, :3]), feat=np.ascontiguousarray(out[:, 3:]), count=count.astype(np.int32),
                    views=np.asarray([bin(self.mask[r]).count("1") for r in keep], np.int32), view_mask=mask,
                    last_stamp=np.asarray([self.last[r] for r in keep], np.int32), born=np.asarray([self.born[r] for r in keep], np.int32),
                    row=np.asarray(keep, np.int32), sums=sums, key=np.asarray([self.key[r] for r in keep], np.int64), n_out=n)

    def extract(self, min_points=1, min_views=1, min_last_stamp=0):
        keep = [r for r in range(self.rows) if self.count[r] >= max(1, min_points) and bin(self.mask[r]).count("1") >= min_views
                and self.last[r] >= min_last_stamp]
        return self._arrays(keep)

    def compact(self, min_last_stamp=0, min_views=0, probation_from=0, drop=None):
        """-> new_row (old rows,) int32"""
        assert drop is None or len(drop) == self.rows
        stay = [r for r in range(self.rows) if self.count[r] >= 1 and self.last[r] >= min_last_stamp
                and (bin(self.mask[r]).count("1") >= min_views or self.born[r] >= probation_from) and (drop is None or not drop[r])]
        new_row = np.full(self.rows, -1, np.int32); new_row[stay] = np.arange(len(stay), dtype=np.int32)
        for name in ("key", "sums", "count", "mask", "last", "born"):
            old = getattr(self, name); setattr(self, name, [old[r] for r in stay])
        self.index = {k: r for r, k in enumerate(self.key)}
        return new_row


OUTPUTS = ("xyz", "feat", "count", "views", "view_mask", "last_stamp", "born", "row")


def same_bytes(a, b, keys=OUTPUTS):
    """every named output of two extracts (or an extract and a fusion) equal byte for byte"""
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if k == "view_mask":
            x, y = x.astype(np.uint64), y.astype(np.uint64)              # (a torch carrier is signed)
        if x.shape != y.shape or x.dtype.itemsize != y.dtype.itemsize or x.tobytes() != y.tobytes():
            return False
    return True


def row_set(e):
    """an extract or a fusion as a set of rows, each the bytes of (xyz, feat, count)"""
    return sorted(np.asarray(e["xyz"][r]).tobytes() + np.asarray(e["feat"][r]).tobytes() + int(e["count"][r]).to_bytes(4, "little") for r in range(int(e["n_out"])))


# ---- a scene the map tests share
def sliding_windows(rng, members=10, n=3000, stride=0.1, width=1.1, noise=0.004):
    """fuse_reading.windows with a stride of its own: the same sheet seen `members` times, window m covering x in [-1 + stride * m, + width),
    with noise, each given in a camera frame of its own.  At the defaults every member holds about half the sheet's points, neighbours share
    most of their cells and the first and the last still overlap.  ([(xyz, feat)], [4 x 4 pose])"""
    base_x, base_f = fr.surface(rng, n)
    out, poses = [], []
    for m in range(members):
        lo = -1.0 + stride * m
        pick = (base_x[:, 0] >= lo) & (base_x[:, 0] < lo + width)
        x = base_x[pick] + rng.normal(scale=noise, size=(int(pick.sum()), 3)).astype(np.float32)
        P = fr.rigid(rng, 0.1, 0.2)
        inv = np.linalg.inv(P.astype(np.float64))
        out.append((np.ascontiguousarray((x @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)), np.ascontiguousarray(base_f[pick]))); poses.append(P)
    return out, poses
