"""The numpy reading of saving and restoring resident maps (include/cvo_hip.h, "Saving and restoring maps"): a map IS its ordered rows.  It rests
on tests/map_reading.py and adds the five checks and the dict, nothing more:

  snapshot   the six arrays of a map_reading.Map, row r at index r, dead rows included: keys uint64, sums (rows, 8) int64, count uint32,
             view_mask uint64, last_stamp and born int32
  restore    the Map whose rows are the arrays', in order, with the dict from key to row -- or Refused with the OR of the bits of the rules a row
             breaks:  1 bad key (bit 63 set, or one of the three 21-bit fields 0)   2 count above 16777215   4 last_stamp < 0 or born < 0
                      8 some |sum_k| > count * (2^39 - 2^15), as exact integers    16 two rows with the same key, among the rows whose key passes 1
             rows above max_rows is not one of the bits: the host refuses it before anything runs (ValueError here)
"""
import numpy as np

import map_reading as mr

BAD_KEY, BAD_COUNT, BAD_STAMP, BAD_SUM, DUPLICATE = 1, 2, 4, 8, 16
SUM_BOUND = 2 ** 39 - 2 ** 15
FIELDS = ("keys", "sums", "count", "view_mask", "last_stamp", "born")


class Refused(mr.Refused):
    def __init__(self, bits):
        super().__init__(f"bits {bits}")
        self.bits = bits


def snapshot(M):
    n = M.rows
    return dict(keys=np.asarray(M.key, np.uint64).reshape(n), sums=np.asarray(M.sums, np.int64).reshape(n, 8), count=np.asarray(M.count, np.uint32).reshape(n),
                view_mask=np.asarray(M.mask, np.uint64).reshape(n), last_stamp=np.asarray(M.last, np.int32).reshape(n), born=np.asarray(M.born, np.int32).reshape(n))


def key_ok(k):
    return k >> 63 == 0 and all((k >> s) & 0x1FFFFF for s in (42, 21, 0))


def refusal_bits(arrays):
    """the OR over the rows of the bits of the rules each breaks (0: a supported map state)"""
    keys = [int(k) for k in np.asarray(arrays["keys"]).astype(np.uint64).tolist()]
    count = [int(c) for c in np.asarray(arrays["count"]).astype(np.uint32).tolist()]
    sums = np.asarray(arrays["sums"]).astype(np.int64).reshape(len(keys), 8).tolist()
    bits = 0
    seen = set()
    for r, k in enumerate(keys):
        if not key_ok(k):
            bits |= BAD_KEY
        elif k in seen:
            bits |= DUPLICATE
        seen.add(k)
        if count[r] > mr.MAX_COUNT:
            bits |= BAD_COUNT
        if int(arrays["last_stamp"][r]) < 0 or int(arrays["born"][r]) < 0:
            bits |= BAD_STAMP
        if any(abs(int(q)) > count[r] * SUM_BOUND for q in sums[r]):   # (python integers: exact)
            bits |= BAD_SUM
    return bits


def restore(arrays, max_rows, voxel):
    n = len(arrays["keys"])
    if n > max_rows:
        raise ValueError(f"rows {n} is outside 0 .. max_rows {max_rows}")
    bits = refusal_bits(arrays)
    if bits:
        raise Refused(bits)
    M = mr.Map(max_rows, voxel)
    M.key = [int(k) for k in np.asarray(arrays["keys"]).astype(np.uint64).tolist()]
    M.sums = [np.array(q, np.int64) for q in np.asarray(arrays["sums"]).astype(np.int64).reshape(n, 8)]
    M.count = [int(c) for c in np.asarray(arrays["count"]).astype(np.uint32).tolist()]
    M.mask = [int(m) for m in np.asarray(arrays["view_mask"]).astype(np.uint64).tolist()]
    M.last = [int(v) for v in np.asarray(arrays["last_stamp"]).tolist()]
    M.born = [int(v) for v in np.asarray(arrays["born"]).tolist()]
    M.index = {k: r for r, k in enumerate(M.key)}
    return M


def same_snapshot(a, b):
    """two snapshots (numpy arrays, or torch carriers of the same bits) equal byte for byte, over the first `rows` rows where a dict names them"""
    for name in FIELDS:
        x, y = (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v) for v in (a[name], b[name]))
        x, y = x[:a.get("rows", len(x))], y[:b.get("rows", len(y))]
        if x.shape != y.shape or x.dtype.itemsize != y.dtype.itemsize or x.tobytes() != y.tobytes():
            return False
    return True


def same_map(A, B):
    """two map_reading.Maps equal field for field, the dict included"""
    return (A.key == B.key and A.count == B.count and A.mask == B.mask and A.last == B.last and A.born == B.born and A.index == B.index
            and len(A.sums) == len(B.sums) and all((p == q).all() for p, q in zip(A.sums, B.sums)))
