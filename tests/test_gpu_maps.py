"""Resident maps (cvo_maps, CvoMaps) against the reading of their definition (tests/map_reading.py) and against fuse's own bytes.  Every
comparison is exact, on bytes: positions, features, counts, views, view masks, stamps, row numbers and row counts."""
import ctypes as C

import numpy as np
import pytest

import frame_reading as frd
import fuse_reading as fr
import map_reading as mr
import pcd_cases as pc

pytestmark = pytest.mark.gpu

INVALID = 4
WANT = ("count", "views", "view_mask", "last_stamp", "born", "row")
FUSED = ("xyz", "feat", "count", "views", "view_mask")
FUSE_WANT = ("count", "views", "view_mask")
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 3000)
EYE = np.eye(4, dtype=np.float32)
MAX_ROWS = 20000


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def reducer(hiplib):
    R = hiplib.CvoReducer(8, 32768)
    yield R
    R.close()


@pytest.fixture(scope="module")
def four():
    """groups of 1, 2, 8 and 64 members with sizes from SIZES -- empty members, wave edges and block edges -- on a noisy sheet, under poses that
    bring every moved coordinate into (0, 10): one 64 m voxel holds a whole group, and at 1e-5 m the cell coordinates stay below 2^20"""
    rng = np.random.default_rng(41)
    sizes = [[3000], [0, 65], [256, 1, 0, 63, 3000, 257, 64, 255], [SIZES[k % 8] for k in range(64)]]
    sizes[3][5] = 3000; sizes[3][40] = 3000
    assert sizes[3][63] > 0 and sizes[3][0] == 0 and set(n for g in sizes for n in g) == set(SIZES)
    groups, poses = [], []
    for g in sizes:
        assert sum(g) <= MAX_ROWS
        groups.append([fr.surface(rng, n, 0.01) for n in g])
        ps = []
        for _ in g:
            P = fr.rigid(rng, 0.1, 0.2); P[:2, 3] += np.float32(4.0); ps.append(P)
        poses.append(ps)
    return groups, poses


@pytest.fixture(scope="module")
def window():
    """ten overlapping windows of one sheet, each in a camera frame of its own"""
    members, poses = mr.sliding_windows(np.random.default_rng(42))
    assert min(x.shape[0] for x, f in members) > 1000
    return members, poses


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev(torch, members):
    return [(up(torch, x), up(torch, f), "points_first") for x, f in members]


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else t


def same(got, want, what="", keys=FUSED):
    assert got["n_out"] == want["n_out"], (what, got["n_out"], want["n_out"])
    for key in keys:
        g, w = host(got[key]), host(want[key])
        if key == "view_mask":
            g, w = g.view(np.uint64), w.view(np.uint64)                # (torch carries the 64 bits as int64)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, key)


def is_reading(maps, k, reading, what="", **flt):
    """map k's extract, every output, against the reading's; and its row counts"""
    got = maps.extract([k], want=WANT, **flt)[0]
    same(got, reading.extract(**flt), what, mr.OUTPUTS)
    rows, live = maps.rows([k])
    assert (int(rows[0]), int(live[0])) == (reading.rows, reading.live), what
    return got


def snapshot(maps, ks):
    rows, live = maps.rows(ks)
    return [{key: (host(v).copy() if hasattr(v, "cpu") else v) for key, v in e.items()} for e in maps.extract(ks, 0, 0, -2 ** 31, want=WANT)], rows.tolist(), live.tolist()


def unchanged(maps, ks, before):
    after = snapshot(maps, ks)
    assert after[1:] == before[1:]
    for a, b in zip(after[0], before[0]):
        same(a, b, "unchanged", mr.OUTPUTS)


# ---- 1. one call against fuse's bytes and order
@pytest.mark.parametrize("voxel", [0.05, 64.0, 1e-5], ids=["5cm", "one_cell", "own_cells"])
def test_one_call_is_fuse_in_bytes_and_order(hiplib, torch, reducer, four, voxel):
    groups, poses = four
    tens = [dev(torch, g) for g in groups]
    stamps = [list(range(len(g))) for g in groups]
    M = hiplib.CvoMaps(reducer, 4, MAX_ROWS, voxel)
    M.integrate([2, 0, 3, 1], tens, poses, stamps)                     # group g into map (2, 0, 3, 1)[g]
    for min_points, min_views in ((1, 1), (2, 2)):
        fused = reducer.fuse(tens, poses, voxel, "mean", min_points, min_views, want=FUSE_WANT)
        got = M.extract([2, 0, 3, 1], min_points, min_views, want=WANT)
        for g in range(4):
            same(got[g], fused[g], (voxel, g, "fuse"))
            same(got[g], fr.fuse_reading(groups[g], poses[g], voxel, "mean", min_points, min_views), (voxel, g, "reading"))
    for g, k in enumerate((2, 0, 3, 1)):
        R = mr.Map(MAX_ROWS, voxel); R.update(groups[g], poses[g], stamps[g])
        e = is_reading(M, k, R, (voxel, g))
        total = sum(x.shape[0] for x, f in groups[g])
        if voxel == 64.0:
            assert e["n_out"] == 1 and host(e["count"]).tolist() == [total] and (g != 3 or int(host(e["view_mask"]).view(np.uint64)[0]) >> 63 == 1)   # bit 63 is real
        if voxel == 1e-5:
            assert e["n_out"] == total                                 # as many cells as points
    assert M.info() == dict(max_maps=4, max_rows=MAX_ROWS, voxel=float(np.float32(voxel)), device_bytes=M.info()["device_bytes"]) and M.info()["device_bytes"] > 4 * MAX_ROWS * 208
    M.close()


# ---- 2. in pieces; 3. many maps with histories of their own
def test_pieces_give_the_bytes_of_one_call(hiplib, torch, reducer, four, window):
    M = hiplib.CvoMaps(reducer, 4, MAX_ROWS, 0.05)
    for members, poses in ((four[0][2], four[1][2]), (window[0][:8], window[1][:8])):
        tens = dev(torch, members)
        M.clear()
        M.integrate([0], [tens], [poses], [list(range(8))])
        for t in range(8):
            M.integrate([1], [tens[t:t + 1]], [poses[t:t + 1]], [[t]])
        M.integrate([2], [tens[:3]], [poses[:3]], [[0, 1, 2]]); M.integrate([2], [tens[3:]], [poses[3:]], [[3, 4, 5, 6, 7]])
        whole, single, split = M.extract([0, 1, 2], want=WANT)
        same(single, whole, "one per call", mr.OUTPUTS); same(split, whole, "3 + 5", mr.OUTPUTS)
        same(whole, reducer.fuse([tens], [poses], 0.05, want=FUSE_WANT)[0], "fuse")
        assert whole["n_out"] > 100 and M.rows([3])[0].tolist() == [0]
    M.close()


def test_eight_maps_with_histories_of_their_own_in_one_launch(hiplib, torch, reducer, window):
    members, poses = window
    members = members[:9] + [(np.zeros((0, 3), np.float32), np.zeros((0, 5), np.float32))]     # member 9 is empty
    tens = dev(torch, members)
    M = hiplib.CvoMaps(reducer, 8, MAX_ROWS, 0.05)
    R = [mr.Map(MAX_ROWS, 0.05) for _ in range(8)]
    # call -> {map: (member numbers, sign)}; map 7 stays untouched throughout, map 6 only ever gets the empty member
    calls = [{0: ([0], 1), 1: ([0, 1, 2], 1), 2: ([9, 3], 1), 3: ([5], 1), 6: ([9], 1)},
             {0: ([1], 1), 1: ([1], -1), 2: ([4, 9, 5], 1), 4: ([8, 7, 6], 1), 5: ([2], 1)},
             {0: ([0], -1), 2: ([3], -1), 3: ([5], -1), 4: ([7], -1), 5: ([2, 3], 1), 1: ([3], 1)},
             {3: ([6], 1), 5: ([2], -1), 0: ([2, 3, 4, 5], 1)},
             {0: ([6], 1), 1: ([6], 1), 2: ([6, 9], 1), 3: ([7], 1), 4: ([9, 0], 1), 5: ([1], 1), 6: ([9, 9], 1)}]     # seven of the eight maps in one launch
    for t, call in enumerate(calls):
        ks = list(call)
        groups = [[tens[m] for m in call[k][0]] for k in ks]
        ps = [[poses[min(m, 8)] for m in call[k][0]] for k in ks]
        stamps = [[m + 60 for m in call[k][0]] for k in ks]           # stamps 60 .. 69: bits 60 .. 63 and 0 .. 5
        for sign in (1, -1):                                           # (one call per sign: a call has one sign for all its maps)
            pick = [j for j, k in enumerate(ks) if call[k][1] == sign]
            if not pick:
                continue
            args = ([ks[j] for j in pick], [groups[j] for j in pick], [ps[j] for j in pick], [stamps[j] for j in pick])
            (M.integrate if sign > 0 else M.remove)(*args)
            for j in pick:
                R[ks[j]].update([members[m] for m in call[ks[j]][0]], ps[j], stamps[j], sign)
        for k in range(8):
            is_reading(M, k, R[k], (t, k))
        for k, e in enumerate(M.extract(None, 1, 2, want=WANT)):       # all eight maps by one extract
            same(e, R[k].extract(1, 2), (t, k, "all at once"), mr.OUTPUTS)
    assert R[7].rows == 0 and R[6].rows == 0 and R[3].rows > R[3].live > 0 and R[0].live > 500
    M.close()


# ---- 4. bad input; 5. layouts
def test_bad_floats_and_far_moves_belong_to_no_cell(hiplib, torch, reducer):
    rng = np.random.default_rng(43)
    x, f = fr.surface(rng, 600, 0.01)
    P = np.concatenate([x, f], axis=1)
    for j, val in enumerate([np.nan, np.inf, -np.inf, 32768.0, -40000.0]):    # one bad float in each of the 8 places
        for k in range(8):
            P[200 + 8 * j + k, k] = val
    x, f = np.ascontiguousarray(P[:, :3]), np.ascontiguousarray(P[:, 3:])
    past_2_15 = EYE.copy(); past_2_15[0, 3] = 32767.5
    past_2_20 = EYE.copy(); past_2_20[1, 3] = 10485.0                  # at voxel 0.01 cell y' >= 2^20 for y >= 0.76
    zero_row = EYE.copy(); zero_row[0, 0] = 0.0                        # 0 * 40000 = 0: the source float must be refused on its own
    members, poses = [(x, f)] * 4, [EYE, past_2_15, past_2_20, zero_row]
    tens = dev(torch, members)
    for voxel in (0.25, 0.01):
        M = hiplib.CvoMaps(reducer, 2, MAX_ROWS, voxel)
        R = mr.Map(MAX_ROWS, voxel); R.update(members, poses, [0, 1, 2, 3])
        M.integrate([1], [tens], [poses], [[0, 1, 2, 3]])
        e = is_reading(M, 1, R, voxel)
        assert int(host(e["count"]).sum()) < 4 * 600 - 40 and np.isfinite(host(e["xyz"])).all()
        same(e, reducer.fuse([tens], [poses], voxel, want=FUSE_WANT)[0], voxel)
        M.remove([1], [tens[1:3]], [poses[1:3]], [[1, 2]]); R.update(members[1:3], poses[1:3], [1, 2], -1)
        is_reading(M, 1, R, (voxel, "removed"))
        M.close()


def test_layouts_give_the_tight_copy_s_bytes(hiplib, torch, reducer, window):
    members, poses = window[0][:4], window[1][:4]
    rng = np.random.default_rng(2)
    tight = dev(torch, members)
    other = []
    for k, (x, f) in enumerate(members):
        n = x.shape[0]
        if k == 0:                                                     # float4 points (stride 16), channel-major features
            other.append((up(torch, np.concatenate([x, rng.normal(size=(n, 1)).astype(np.float32)], axis=1))[:, :3], up(torch, f.T), "channels_first"))
        elif k == 1:                                                   # columns 2 .. 4 of an (n, 8) tensor, features every other row of a (2 n, 5) one
            big = rng.normal(size=(n, 8)).astype(np.float32); big[:, 2:5] = x
            ff = rng.normal(size=(2 * n, 5)).astype(np.float32); ff[::2] = f
            other.append((up(torch, big)[:, 2:5], up(torch, ff)[::2], "points_first"))
        else:
            other.append((tight[k][0], up(torch, f.T), "channels_first"))
    M = hiplib.CvoMaps(reducer, 2, MAX_ROWS, 0.05)
    M.integrate([0, 1], [tight, other], [poses, poses], [[0, 1, 2, 3]] * 2)
    a, b = M.extract([0, 1], want=WANT)
    same(b, a, "layouts", mr.OUTPUTS); same(a, fr.fuse_reading(members, poses, 0.05), "reading")
    M.remove([0, 1], [other[1:2], tight[1:2]], [poses[1:2]] * 2, [[1], [1]])      # what went in one way comes out the other
    a, b = M.extract([0, 1], want=WANT)
    same(b, a, "layouts, removed", mr.OUTPUTS)
    M.close()


# ---- 6. removal
def test_a_window_of_four_slides_over_ten_members(hiplib, torch, reducer, window):
    members, poses = window
    tens = dev(torch, members)
    M = hiplib.CvoMaps(reducer, 1, MAX_ROWS, 0.05)
    R = mr.Map(MAX_ROWS, 0.05)
    for t in range(10):
        M.integrate([0], [[tens[t]]], [[poses[t]]], [[t]]); R.update([members[t]], [poses[t]], [t])
        if t >= 4:
            M.remove([0], [[tens[t - 4]]], [[poses[t - 4]]], [[t - 4]]); R.update([members[t - 4]], [poses[t - 4]], [t - 4], -1)
        lo = max(0, t - 3)
        e = is_reading(M, 0, R, t)
        fused = reducer.fuse([tens[lo:t + 1]], [poses[lo:t + 1]], 0.05, want=FUSE_WANT)[0]
        assert mr.row_set({k: host(v) for k, v in e.items()}) == mr.row_set({k: host(v) for k, v in fused.items()}), t
        masks = {host(e["xyz"])[r].tobytes(): int(host(e["view_mask"]).view(np.uint64)[r]) for r in range(e["n_out"])}
        fx, fm = host(fused["xyz"]), host(fused["view_mask"]).view(np.uint64)
        assert all(masks[fx[r].tobytes()] == int(fm[r]) << lo for r in range(fused["n_out"])), t     # the bits sit at the stamps
    assert R.rows > R.live                                              # dead rows were skipped by every extract above
    M.close()


def test_a_dead_row_is_revived_with_a_new_born(hiplib, torch, reducer, window):
    members, poses = window
    tens = dev(torch, members)
    M = hiplib.CvoMaps(reducer, 1, MAX_ROWS, 0.05)
    R = mr.Map(MAX_ROWS, 0.05)
    for sign, m, stamp in ((1, 0, 4), (1, 1, 5), (-1, 0, 4), (1, 0, 9)):
        (M.integrate if sign > 0 else M.remove)([0], [[tens[m]]], [[poses[m]]], [[stamp]]); R.update([members[m]], [poses[m]], [stamp], sign)
        e = is_reading(M, 0, R, (sign, m, stamp))
    born = host(e["born"])
    assert (born == 9).any() and (born == 4).any() and (born == 5).any()      # revived rows; rows member 1 kept alive; member 1's own
    M.close()


def test_refused_removals_leave_every_map_byte_identical(hiplib, torch, reducer, window):
    members, poses = window
    tens = dev(torch, members)
    M = hiplib.CvoMaps(reducer, 3, MAX_ROWS, 0.05)
    M.integrate([0, 1, 2], [[tens[0]], [tens[1]], [tens[0], tens[1]]], [[poses[0]], [poses[1]], poses[:2]], [[0], [1], [0, 1]])
    before = snapshot(M, [0, 1, 2])
    with pytest.raises(hiplib.CvoError, match=r"map 1 \(group 1\).*absent"):            # map 2's removal in the same call is fine: nothing of it may stay
        M.remove([2, 1], [[tens[0]], [tens[2]]], [[poses[0]], [poses[2]]], [[0], [2]])
    unchanged(M, [0, 1, 2], before)
    with pytest.raises(hiplib.CvoError, match=r"map 0 .*more members"):
        M.remove([1, 0], [[tens[1]], [tens[0], tens[0]]], [[poses[1]], [poses[0]] * 2], [[1], [0, 0]])
    unchanged(M, [0, 1, 2], before)
    M.remove([2], [[tens[0]]], [[poses[0]]], [[0]])                     # and the maps still work
    left = M.extract([2])[0]; fused = reducer.fuse([[tens[1]]], [[poses[1]]], 0.05, want=FUSE_WANT)[0]
    assert mr.row_set({k: host(v) for k, v in left.items()}) == mr.row_set({k: host(v) for k, v in fused.items()})
    M.close()


# ---- 7. capacity
def test_max_rows_exactly_enough_and_one_short(hiplib, torch, reducer, window):
    members, poses = window
    tens = dev(torch, members)
    first = fr.fuse_reading(members[:1], poses[:1], 0.05)["n_out"]
    need = fr.fuse_reading(members[:2], poses[:2], 0.05)["n_out"]
    assert need > first + 10
    for max_rows in (need, need - 1):
        M = hiplib.CvoMaps(reducer, 2, max_rows, 0.05)
        M.integrate([0, 1], [[tens[0]]] * 2, [[poses[0]]] * 2, [[0]] * 2)
        before = snapshot(M, [0, 1])
        if max_rows == need:
            M.integrate([0], [[tens[1]]], [[poses[1]]], [[1]])
            assert M.rows([0])[0].tolist() == [need]
            same(M.extract([0], want=FUSE_WANT)[0], fr.fuse_reading(members[:2], poses[:2], 0.05), "exact")
        else:
            with pytest.raises(hiplib.CvoError, match=rf"map 0 .*{first} rows.*{need - first} new cells.*max_rows {need - 1}"):
                M.integrate([1, 0], [[tens[0]], [tens[1]]], [[poses[0]], [poses[1]]], [[5], [1]])   # map 1's part is fine: it must not stay
            unchanged(M, [0, 1], before)
        M.close()
    M = hiplib.CvoMaps(reducer, 1, 1, 64.0)                             # max_rows = 1: one cell is the whole map
    near = EYE.copy(); near[:3, 3] = 10.0                              # every moved coordinate in (0, 64)
    far = near.copy(); far[0, 3] = 100.0
    M.integrate([0], [tens[:3]], [[near] * 3], [[0, 1, 2]])
    one = M.extract([0], want=FUSE_WANT)[0]
    same(one, fr.fuse_reading(members[:3], [near] * 3, 64.0), "one row"); assert one["n_out"] == 1
    with pytest.raises(hiplib.CvoError, match="max_rows 1"):
        M.integrate([0], [tens[:1]], [[far]], [[3]])
    same(M.extract([0], want=FUSE_WANT)[0], one, "one row still")
    M.close()


def test_the_count_bound(hiplib, torch):
    n = 1048575
    R = hiplib.CvoReducer(1, n)
    rng = np.random.default_rng(44)
    x = rng.uniform(0.5, 9.5, (n, 3)).astype(np.float32); f = rng.uniform(0, 255, (n, 5)).astype(np.float32)
    t = (up(torch, x), up(torch, f), "points_first")
    M = hiplib.CvoMaps(R, 1, 4, 64.0)
    for k in range(16):
        M.integrate([0], [[t]], [[EYE]], [[k]])
    e = M.extract([0], want=WANT)[0]
    keys, sums, counts, _ = mr.call_cells([(x, f)], [EYE], 64.0)
    assert counts.tolist() == [n] and host(e["count"]).tolist() == [16 * n] == [mr.MAX_COUNT - 15]
    mean = ((16 * sums).astype(np.float64) / (np.float64(16 * n) * 16777216.0)).astype(np.float32)
    assert np.concatenate([host(e["xyz"]), host(e["feat"])], axis=1).tobytes() == mean.tobytes()
    assert int(host(e["view_mask"])[0]) == 0xFFFF and host(e["last_stamp"]).tolist() == [15] and host(e["born"]).tolist() == [0]
    with pytest.raises(hiplib.CvoError, match="16777215"):
        M.integrate([0], [[t]], [[EYE]], [[16]])
    again = M.extract([0], want=WANT)[0]
    same(again, e, "refused", mr.OUTPUTS)
    M.integrate([0], [[(t[0][:15], t[1][:15], "points_first")]], [[EYE]], [[16]])     # exactly to the bound
    assert host(M.extract([0])[0]["count"]).tolist() == [mr.MAX_COUNT]
    assert R.L.cvo_reducer_destroy(R.h) == INVALID and b"still live" in R.L.cvo_last_error()   # live maps: the reducer stays
    M.close(); R.close()


# ---- 8. extract
class Raw:
    """one map's output arrays as byte tensors prefilled with 0xA5, each with 64 guard bytes behind its cap rows"""
    G = 64
    WIDTH = dict(xyz=12, feat=20, count=4, views=4, view_mask=8, last_stamp=4, born=4, row=4)

    def __init__(self, torch, cap):
        self.cap = cap
        self.t = {k: torch.full((w * cap + self.G,), 0xA5, dtype=torch.uint8, device="cuda") for k, w in self.WIDTH.items()}

    def record(self, api):
        return api.MapCloud(*[self.t[k].data_ptr() for k in self.WIDTH], self.cap, 0)

    def host(self, key, dtype, rows):
        return self.t[key].cpu().numpy()[:self.WIDTH[key] * rows].view(dtype)

    def guards_intact(self):
        return all((t.cpu().numpy()[self.WIDTH[k] * self.cap:] == 0xA5).all() for k, t in self.t.items())


def test_extract_filters_cap_guards_count_only_and_every_output(hiplib, torch, reducer, window):
    api = hiplib.api
    members, poses = window
    tens = dev(torch, members)
    M = hiplib.CvoMaps(reducer, 2, MAX_ROWS, 0.05)
    R = mr.Map(MAX_ROWS, 0.05)
    M.integrate([1], [tens[:6]], [poses[:6]], [[3, 4, 5, 6, 7, 8]]); R.update(members[:6], poses[:6], [3, 4, 5, 6, 7, 8])
    for flt in (dict(min_points=1, min_views=1), dict(min_points=3, min_views=1), dict(min_points=1, min_views=3), dict(min_points=0, min_views=0),
                dict(min_points=2, min_views=2, min_last_stamp=7), dict(min_last_stamp=9)):
        e = is_reading(M, 1, R, flt, **flt)
    assert e["n_out"] == 0 and is_reading(M, 1, R, "all")["n_out"] == R.rows
    a, b = M.extract([1, 0], [1, 5], [2, 0], [0, 0], want=WANT)        # a filter per map; map 0 is empty
    same(a, R.extract(1, 2), "per map", mr.OUTPUTS); assert b["n_out"] == 0
    full = R.extract(1, 2)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    ks = np.asarray([1], np.int32); flt = (api.MapFilter * 1)(api.MapFilter(1, 2, 0, 0))
    for cap in (full["n_out"] - 1, 257, 1, full["n_out"]):
        raw = Raw(torch, cap); n_out = np.zeros(1, np.int32)
        assert M.L.cvo_maps_extract(M.h, 1, ip(ks), flt, (api.MapCloud * 1)(raw.record(api)), ip(n_out), None) == 0
        torch.cuda.synchronize()
        rows = min(cap, full["n_out"])
        assert n_out.tolist() == [full["n_out"]] and raw.guards_intact(), cap            # the FULL count; no byte behind row cap - 1
        for key in mr.OUTPUTS:
            assert raw.host(key, full[key].dtype, rows).tobytes() == full[key][:rows].tobytes(), (cap, key)
    n_out = np.zeros(1, np.int32)
    assert M.L.cvo_maps_extract(M.h, 1, ip(ks), flt, (api.MapCloud * 1)(), ip(n_out), None) == 0 and n_out.tolist() == [full["n_out"]]   # count only
    assert M.extract([1], 1, 2, cap=0, want=())[0]["n_out"] == full["n_out"]
    with pytest.raises(hiplib.CvoError, match="more than cap 100"):
        M.extract([1], cap=100)
    M.check_extract([0, 1], 1, 1)
    bad = (api.MapCloud * 1)(api.MapCloud(None, None, None, None, None, None, None, None, 70000, 0))
    assert M.L.cvo_check_maps_extract(M.h, 1, ip(ks), flt, bad) == INVALID and b"cap 70000" in M.L.cvo_last_error()
    raw = Raw(torch, 10); rec = raw.record(api); rec.view_mask += 4
    assert M.L.cvo_check_maps_extract(M.h, 1, ip(ks), flt, (api.MapCloud * 1)(rec)) == INVALID and b"view_mask is not 8-byte aligned" in M.L.cvo_last_error()
    assert M.L.cvo_check_maps_extract(M.h, 2, ip(np.asarray([1, 1], np.int32)), (api.MapFilter * 2)(), (api.MapCloud * 2)()) == INVALID and b"twice" in M.L.cvo_last_error()
    M.close()


# ---- 9. compact
def test_compact_every_clause_drop_new_row_and_the_rebuilt_table(hiplib, torch, reducer, window):
    from cvo_slam_amd.voxels import carve_mask
    members, poses = window
    tens = dev(torch, members)
    M = hiplib.CvoMaps(reducer, 3, MAX_ROWS, 0.05)
    R = [mr.Map(MAX_ROWS, 0.05) for _ in range(3)]
    for k in range(3):
        for t in range(5):
            M.integrate([k], [[tens[t]]], [[poses[t]]], [[t]]); R[k].update([members[t]], [poses[t]], [t])
        M.remove([k], [[tens[0]]], [[poses[0]]], [[0]]); R[k].update([members[0]], [poses[0]], [0], -1)
    before = M.extract([0], want=WANT)[0]
    rows_out, new_row = M.compact([0], new_row=True)                   # the defaults drop the dead rows alone
    want_new = R[0].compact()
    assert rows_out.tolist() == [R[0].rows] and host(new_row[0]).tobytes() == want_new.tobytes() and (want_new == -1).any()
    after = is_reading(M, 0, R[0], "dead rows dropped")
    same(after, before, "extract, compact, extract", mr.OUTPUTS[:-1])
    assert np.array_equal(want_new[host(before["row"])], host(after["row"]))
    # every clause at once on map 1, with a drop mask; map 2 by ageing alone, in the same call
    e = R[1].extract()
    drop = np.zeros(R[1].rows, np.uint8); drop[e["row"][e["views"] >= 2][:7]] = 1
    mask = carve_mask(R[1].rows, up(torch, e["row"]), up(torch, np.flatnonzero(drop[e["row"]]).astype(np.int32)), up(torch, np.ones(int(drop.sum()), np.int32)))
    assert host(mask).tobytes() == drop.tobytes()
    rows_out, new_row = M.compact([1, 2], [1, 3], [2, 0], [3, -2 ** 31], drop=[mask, None], new_row=True)
    want1 = R[1].compact(1, 2, 3, drop); want2 = R[2].compact(3, 0, -2 ** 31)
    assert rows_out.tolist() == [R[1].rows, R[2].rows] and 0 < R[1].rows < e["n_out"] and 0 < R[2].rows < e["n_out"]
    assert host(new_row[0]).tobytes() == want1.tobytes() and host(new_row[1]).tobytes() == want2.tobytes()
    for k in (1, 2):
        is_reading(M, k, R[k], ("compacted", k))
    # integrate and remove after a compaction: the rebuilt table finds every cell, and new cells are born behind the survivors
    for k in range(3):
        M.integrate([k], [[tens[0], tens[5]]], [[poses[0], poses[5]]], [[10, 11]]); R[k].update([members[0], members[5]], [poses[0], poses[5]], [10, 11])
        # member 4 leaves: map 0's compaction dropped dead rows alone, so plain removal holds; maps 1 and 2 lost live rows of member 4's
        sign = -1 if k == 0 else -2
        M.remove([k], [[tens[4]]], [[poses[4]]], [[4]], present=k > 0); R[k].update([members[4]], [poses[4]], [4], sign)
        is_reading(M, k, R[k], ("after", k))
    M.compact(); [r.compact() for r in R]                               # all maps, twice over the two sides
    M.compact(); [r.compact() for r in R]
    for k in range(3):
        is_reading(M, k, R[k], ("twice", k))
    empty = hiplib.CvoMaps(reducer, 1, 10, 0.05)
    assert empty.compact().tolist() == [0] and empty.extract()[0]["n_out"] == 0
    empty.close(); M.close()


def test_the_loop_with_carving_and_probation_runs_past_the_window(hiplib, torch, reducer, window):
    """INTEGRATION.md's loop, two streams in every call: integrate keyframe t, remove keyframe t - K (what is still there), extract, and a
    compaction that drops LIVE rows -- a drop mask and one-view cells past their probation -- until every keyframe that lost rows has left"""
    members, poses = window
    tens = dev(torch, members)
    K = 3
    M = hiplib.CvoMaps(reducer, 2, MAX_ROWS, 0.05)
    R = [mr.Map(MAX_ROWS, 0.05) for _ in range(2)]
    shift = (0, 1)                                                     # stream s sees member t + shift[s]
    for t in range(9):
        new = [t + d for d in shift]
        M.integrate([0, 1], [[tens[m]] for m in new], [[poses[m]] for m in new], [[t], [t]])
        for s in range(2):
            R[s].update([members[new[s]]], [poses[new[s]]], [t])
        if t >= K:
            old = [t - K + d for d in shift]
            if t == K:                                                 # plain removal after those compactions: a carved cell is absent
                before = snapshot(M, [0, 1])
                with pytest.raises(hiplib.CvoError, match=r"map 0 .*absent"):
                    M.remove([0, 1], [[tens[m]] for m in old], [[poses[m]] for m in old], [[t - K], [t - K]])
                unchanged(M, [0, 1], before)
            M.remove([0, 1], [[tens[m]] for m in old], [[poses[m]] for m in old], [[t - K], [t - K]], present=True)
            for s in range(2):
                R[s].update([members[old[s]]], [poses[old[s]]], [t - K], -2)
        got = M.extract([0, 1], min_views=2, want=WANT)
        drops = []
        for s in range(2):
            e = R[s].extract(min_views=2)
            same(got[s], e, (t, s), mr.OUTPUTS)
            drop = np.zeros(R[s].rows, np.uint8); drop[e["row"][::7]] = 1
            drops.append(drop)
        dev_drops = [torch.zeros(R[s].rows, dtype=torch.uint8, device="cuda") for s in range(2)]
        for s in range(2):
            dev_drops[s][got[s]["row"][::7].long()] = 1                # from the extract's own row numbers, on the device
        rows_out = M.compact([0, 1], min_views=2, probation_from=t - 1, drop=dev_drops)
        for s in range(2):
            R[s].compact(min_views=2, probation_from=t - 1, drop=drops[s])
            is_reading(M, s, R[s], (t, s, "compacted"))
        assert rows_out.tolist() == [R[0].rows, R[1].rows]
    assert R[0].rows > 50
    # a group that is partly present in a row refuses, with the maps as they were
    before = snapshot(M, [0, 1])
    with pytest.raises(hiplib.CvoError, match="partly present"):
        M.remove([0], [[tens[8], tens[0]]], [[poses[8], poses[0]]], [[8, 0]], present=True)
    unchanged(M, [0, 1], before)
    M.close()


# ---- 10. frames
def test_frames_are_fuse_frames_bytes(hiplib, torch, reducer):
    rng = np.random.default_rng(45)
    cams = [pc.CAMERA, pc.CAMERA_B]
    for (w, h), steps in (((64, 64), (1, 16)), ((100, 70), (2,))):
        kf, poses, tens = [], [], []
        for m in range(4):
            bgr, dep = pc.image(w, h, "noise"), pc.depth(w, h, "holes" if m % 2 else "full")
            kf.append((bgr, dep)); poses.append(fr.rigid(rng, 0.05, 0.1))
            if m == 2:                                                 # BGRA with both pitches above the rows' bytes
                bgra = rng.integers(0, 256, (h, w + 3, 4), dtype=np.uint8); bgra[:, :w, :3] = bgr
                wide = rng.integers(0, 65536, (h, w + 5), dtype=np.uint16); wide[:, :w] = dep
                tens.append((up(torch, bgra)[:, :w, :3], up(torch, wide.view(np.int16))[:, :w]))
            else:
                tens.append((up(torch, bgr), up(torch, dep.view(np.int16))))
        ci = [0, 1, 0, 1]
        for step in steps:
            M = hiplib.CvoMaps(reducer, 2, MAX_ROWS, 0.1)
            M.integrate_frames([0], [tens], [poses], [[0, 1, 2, 3]], cams, cam_index=[ci], step=step)
            for t in range(4):
                M.integrate_frames([1], [[tens[t]]], [[poses[t]]], [[t]], cams, cam_index=[[ci[t]]], step=step)
            fused = reducer.fuse_frames([tens], [poses], cams, 0.1, cam_index=[ci], step=step, want=FUSE_WANT)[0]
            a, b = M.extract([0, 1], want=WANT)
            same(a, fused, (w, h, step)); same(b, a, (w, h, step, "pieces"), mr.OUTPUTS)
            dense = [frd.dense_reading(bgr, dep, cams[c], step) for (bgr, dep), c in zip(kf, ci)]
            R = mr.Map(MAX_ROWS, 0.1); R.update(dense, poses, [0, 1, 2, 3])
            is_reading(M, 0, R, (w, h, step))
            M.remove_frames([0], [tens[1:3]], [poses[1:3]], [[1, 2]], cams, cam_index=[ci[1:3]], step=step); R.update(dense[1:3], poses[1:3], [1, 2], -1)
            is_reading(M, 0, R, (w, h, step, "removed"))
            assert a["n_out"] > (0 if step == 16 else 100)
            M.check_integrate_frames([0], [tens], [poses], [[0, 1, 2, 3]], cams, cam_index=[ci], step=step)
            M.close()


# ---- 11. the stream rule; 12. coexistence; 13. reproducibility
def test_stream_orders_input_and_output(hiplib, torch, reducer, window):
    members, poses = window[0][:4], window[1][:4]
    want = fr.fuse_reading(members, poses, 0.05, 0, 1, 2)
    side = torch.cuda.Stream()
    pinned = [(torch.from_numpy(x).pin_memory(), torch.from_numpy(f).pin_memory()) for x, f in members]
    tens = [(torch.full(x.shape, 1000.0, dtype=torch.float32, device="cuda"), torch.zeros(f.shape, dtype=torch.float32, device="cuda"), "points_first") for x, f in members]
    a = torch.randn((4096, 4096), device="cuda")
    M = hiplib.CvoMaps(reducer, 1, MAX_ROWS, 0.05)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):                                             # work in front of the writes: without the edge in, the kernel would read the 1000s
            a = a @ a * 1e-3
        for (tx, tf, _), (hx, hf) in zip(tens, pinned):
            tx.copy_(hx, non_blocking=True); tf.copy_(hf, non_blocking=True)
    M.integrate([0], [tens], [poses], [[0, 1, 2, 3]], cloud_stream=side)
    for tx, tf, _ in tens:                                             # the members were read before the call returned
        tx.fill_(-3.0)
    got = M.extract([0], 1, 2, want=WANT, stream=side)[0]
    with torch.cuda.stream(side):                                      # a read queued on that stream behind the call, and an overwrite behind the read
        snap = {k: got[k].clone() for k in FUSED}
        for k in FUSED:
            got[k].zero_()
    side.synchronize()
    same(dict(snap, n_out=got["n_out"]), want)
    M.close()


def test_reduce_fuse_view_and_maps_interleaved_on_one_reducer(hiplib, torch, reducer, window):
    import voxel_reading as vr
    members, poses = window[0][:4], window[1][:4]
    tens = dev(torch, members)
    M = hiplib.CvoMaps(reducer, 2, MAX_ROWS, 0.05)
    R = mr.Map(MAX_ROWS, 0.05)
    scratch = reducer.scratch_bytes()
    cam = (5000.0, 60.0, 60.0, 32.0, 24.0)
    for t in range(4):
        M.integrate([1], [[tens[t]]], [[poses[t]]], [[t]]); R.update([members[t]], [poses[t]], [t])
        g = reducer.reduce([tens[t]], 0.05, "mean", 1, want=("count",))[0]
        w = vr.reduce_reading(members[t][0], members[t][1], 0.05, "mean", 1)
        assert g["n_out"] == w["n_out"] and host(g["xyz"]).tobytes() == w["xyz"].tobytes()
        same(reducer.fuse([tens[:t + 1]], [poses[:t + 1]], 0.05, want=FUSE_WANT)[0], fr.fuse_reading(members[:t + 1], poses[:t + 1], 0.05), t)
        e = is_reading(M, 1, R, t)
        v = reducer.view([(e["xyz"], e["feat"], "points_first")], [EYE], cam, (64, 48), cell=2, want=("source",))[0]
        assert 0 < v["n_out"] <= e["n_out"]
    assert reducer.scratch_bytes() == scratch
    M.close()


def test_the_same_history_twice_gives_identical_bytes(hiplib, torch, reducer, window):
    members, poses = window
    tens = dev(torch, members)
    runs = []
    for max_rows in (MAX_ROWS, 7000):                                  # another table size: another layout, which must not show
        M = hiplib.CvoMaps(reducer, 1, max_rows, 0.05)
        for t in range(6):
            M.integrate([0], [[tens[t]]], [[poses[t]]], [[t]])
            if t >= 2:
                M.remove([0], [[tens[t - 2]]], [[poses[t - 2]]], [[t - 2]])
        mid = M.extract([0], 0, 0, want=WANT)[0]
        M.compact([0], min_views=2, probation_from=5)
        M.integrate([0], [tens[6:8]], [poses[6:8]], [[6, 7]])
        runs.append(({k: host(v).copy() if hasattr(v, "cpu") else v for k, v in mid.items()}, {k: host(v).copy() if hasattr(v, "cpu") else v for k, v in M.extract([0], 0, 0, want=WANT)[0].items()}))
        M.close()
    R = mr.Map(MAX_ROWS, 0.05)                                          # the same history in the reading
    for t in range(6):
        R.update([members[t]], [poses[t]], [t])
        if t >= 2:
            R.update([members[t - 2]], [poses[t - 2]], [t - 2], -1)
    want = [R.extract(0, 0)]
    dropped = R.compact(min_views=2, probation_from=5)
    R.update(members[6:8], poses[6:8], [6, 7])
    want.append(R.extract(0, 0))
    assert (dropped == -1).any() and (dropped >= 0).any() and want[1]["n_out"] > 0     # the compaction dropped rows and kept some
    for stage in (0, 1):
        same(runs[1][stage], runs[0][stage], stage, mr.OUTPUTS)
        same(runs[0][stage], want[stage], (stage, "reading"), mr.OUTPUTS)


# ---- 14. end to end
def test_an_extracted_map_viewed_and_aligned_is_the_reading_s_rows(hiplib, torch):
    from cvo_slam_amd import synth
    frames, cam_poses = synth.make_sequence(0, 5)
    clouds = []
    for bgr, dep in frames:
        c = synth.dense_cloud(bgr, dep, synth.TUM1)
        pick = np.unique(np.linspace(0, c.n - 1, 5000).astype(np.int64))
        clouds.append((np.ascontiguousarray(c.xyz[pick]), np.ascontiguousarray(c.feat[:, pick].T)))
    poses = [(np.linalg.inv(cam_poses[3]) @ cam_poses[k]).astype(np.float32) for k in range(4)]   # keyframe k in the newest keyframe's frame
    Rd = hiplib.CvoReducer(2, 20000)
    M = hiplib.CvoMaps(Rd, 1, 20000, 0.04)
    R = mr.Map(20000, 0.04)
    tens = dev(torch, clouds[:4])
    for t in range(4):
        M.integrate([0], [[tens[t]]], [[poses[t]]], [[t]]); R.update([clouds[t]], [poses[t]], [t])
    got = M.extract([0], min_views=2, want=WANT)[0]
    want = R.extract(min_views=2)
    same(got, want, "extract", mr.OUTPUTS)
    cam = (synth.TUM1["depth_factor"], synth.TUM1["fx"], synth.TUM1["fy"], synth.TUM1["cx"], synth.TUM1["cy"])
    size = (frames[0][1].shape[1], frames[0][1].shape[0])
    seen = Rd.view([(got["xyz"], got["feat"], "points_first")], [EYE], cam, size, cell=8, want=("source",))[0]
    src = host(seen["source"])
    assert 0 < seen["n_out"] <= want["n_out"] and host(seen["xyz"]).tobytes() == want["xyz"][src].tobytes()   # (the identity move keeps the bits: no -0.0 here)
    moving = Rd.reduce([dev(torch, clouds[4:])[0]], 0.04, "mean", 1, want=())[0]
    B = hiplib.CvoBatch(1)
    B.set_pairs_clouds([(seen["xyz"], seen["feat"], "points_first"), (moving["xyz"], moving["feat"], "points_first")], [0], [1])
    B.align_async(1)
    res = B.wait(1)[0]
    Bh = hiplib.CvoBatch(1)
    Bh.set_pairs([(np.ascontiguousarray(want["xyz"][src]), np.ascontiguousarray(want["feat"][src].T), host(moving["xyz"]), np.ascontiguousarray(host(moving["feat"]).T))])
    ref = Bh.align(1)[0]
    assert res["status"] == 0 and ref["status"] == 0
    assert res["transform"].tobytes() == ref["transform"].tobytes() and res["ell"] == ref["ell"] and res["iter"] == ref["iter"]
    B.close(); Bh.close(); M.close(); Rd.close()
