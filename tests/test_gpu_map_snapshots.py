"""Saving and restoring resident maps (cvo_maps_snapshot / cvo_maps_restore, CvoMaps.snapshot / restore / grown, voxels.save_maps / load_maps)
against the reading of the definition (tests/map_snapshot_reading.py) and against the statement it rests on: a map IS its ordered rows, so a
restored twin returns the original's bytes from every later call.  Every comparison is exact, on bytes."""
import numpy as np
import pytest

import fuse_reading as fr
import map_reading as mr
import map_snapshot_reading as sr
import table_cases as tc
import view_reading as vw
import voxel_reading as vr
from test_gpu_map_views import SHEET_CAM
from test_gpu_maps import WANT as MAP_WANT
from test_gpu_view_clouds import up_depth

pytestmark = pytest.mark.gpu

EYE = np.eye(4, dtype=np.float32)
VOXEL = 0.05
GUARD = 0x5A
SIGNED = {"keys": np.int64, "sums": np.int64, "count": np.int32, "view_mask": np.int64, "last_stamp": np.int32, "born": np.int32}
UNSIGNED = {"keys": np.uint64, "sums": np.int64, "count": np.uint32, "view_mask": np.uint64, "last_stamp": np.int32, "born": np.int32}
BIG = 70001


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def reducer(hiplib):
    R = hiplib.CvoReducer(16, 32768)
    yield R
    R.close()


@pytest.fixture(scope="module")
def window():
    members, poses = mr.sliding_windows(np.random.default_rng(42))
    assert min(x.shape[0] for x, f in members) > 1000
    return members, poses


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev(torch, members):
    return [(up(torch, x), up(torch, f), "points_first") for x, f in members]


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def to_host(snap):
    """a snapshot's dict as numpy arrays in the header's types"""
    rows = int(snap.get("rows", len(snap["keys"])))
    return {k: np.ascontiguousarray(host(snap[k])[:rows]).view(UNSIGNED[k]) for k in sr.FIELDS}


def to_dev(torch, arrays):
    """numpy arrays in the header's types as a dict `restore` takes (torch's signed carriers)"""
    return {k: up(torch, np.ascontiguousarray(arrays[k]).view(SIGNED[k])) for k in sr.FIELDS} | dict(rows=int(len(arrays["keys"])))


def is_reading(M, k, R, what=""):
    got = to_host(M.snapshot([k])[0])
    want = sr.snapshot(R)
    for name in sr.FIELDS:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (what, name, got[name].shape, want[name].shape)
        assert got[name].tobytes() == want[name].tobytes(), (what, name)
    rows, live = M.rows([k])
    assert (int(rows[0]), int(live[0])) == (R.rows, R.live), what


def lattice(n, seed=0):
    """n points, one per cell of a slanted line of distinct cells, exact in float32 at tc.VOXEL"""
    k = np.arange(n, dtype=np.int64)
    cells = np.stack([k - 10, 2 * k - 7 + 3 * seed, -k - seed], axis=1)
    return tc.positions(cells), tc.features(n, 900 + seed + n)


def lattice_history(hiplib, torch, M, k, n):
    """map k of M and its reading after a history that ends with exactly n rows, dead and revived ones among them"""
    R = mr.Map(M.max_rows, tc.VOXEL)
    x, f = lattice(n, k)
    a = n // 2
    steps = [((x[:a], f[:a]), 0, 1), ((x[a // 2:], f[a // 2:]), 1, 1), ((x[:a], f[:a]), 0, -1), ((x[:a // 4], f[:a // 4]), 5, 1)]
    if n < 4:                                                          # a map of dead rows alone
        steps = [((x, f), 0, 1), ((x, f), 0, -1)]
    for cloud, stamp, sign in steps:
        if cloud[0].shape[0] == 0:
            continue
        (M.integrate if sign > 0 else M.remove)([k], [dev(torch, [cloud])], [[EYE]], [[stamp]])
        R.update([cloud], [EYE], [stamp], sign)
    assert R.rows == n
    return R


# ---- 1. snapshot against the reading
SIZES = (0, 1, 255, 256, 257, 3000, 64, 65)


@pytest.fixture(scope="module")
def eight(hiplib, torch, reducer):
    M = hiplib.CvoMaps(reducer, 8, 3000, tc.VOXEL)                     # (map 5 holds exactly max_rows rows)
    R = [lattice_history(hiplib, torch, M, k, n) for k, n in enumerate(SIZES)]
    assert [r.rows for r in R] == list(SIZES) and all(r.live < r.rows for r in R if r.rows >= 4) and R[1].rows == 1 and R[1].live == 0
    yield M, R
    M.close()


def test_eight_histories_in_one_call_are_the_reading_s_rows(hiplib, torch, eight):
    M, R = eight
    got = M.snapshot(None)
    assert len(got) == 8 and [g["rows"] for g in got] == list(SIZES)
    for k in range(8):
        assert sr.same_snapshot(to_host(got[k]), sr.snapshot(R[k])), k
        is_reading(M, k, R[k], k)
    order = [5, 0, 7, 2]                                               # a list in an order of its own
    for g, k in zip(M.snapshot(order), order):
        assert sr.same_snapshot(to_host(g), sr.snapshot(R[k])), k


def guarded(torch, M, rows, extra):
    """per map: arrays of rows + extra + 8 rows filled with GUARD bytes, and the dict that offers the first rows + extra of each"""
    whole, offered = [], []
    for n in rows:
        cap = int(n) + extra
        full = M.empty_snapshots([cap + 8])[0]
        for name in sr.FIELDS:
            full[name].view(torch.uint8).fill_(GUARD)
        whole.append(full)
        offered.append({name: full[name][:cap] for name in sr.FIELDS} | dict(rows=cap))
    return whole, offered


def untouched_behind(whole, rows):
    for full, n in zip(whole, rows):
        for name in sr.FIELDS:
            tail = host(full[name])[int(n):]
            assert (tail.view(np.uint8) == GUARD).all(), name


@pytest.mark.parametrize("extra", [0, 5])
def test_capacity_exact_and_larger_touch_no_byte_behind_the_rows(hiplib, torch, eight, extra):
    M, R = eight
    whole, offered = guarded(torch, M, SIZES, extra)
    M.check_snapshot(None, offered)
    out = M.snapshot_into(None, offered)
    assert out.dtype == np.int32 and out.tolist() == list(SIZES)
    untouched_behind(whole, SIZES)
    for k in range(8):
        assert sr.same_snapshot(to_host(dict(offered[k], rows=SIZES[k])), sr.snapshot(R[k])), k


def test_capacity_one_short_is_refused_with_every_output_untouched(hiplib, torch, eight):
    M, R = eight
    whole, offered = guarded(torch, M, SIZES, 0)
    offered[2] = {name: whole[2][name][:SIZES[2] - 1] for name in sr.FIELDS} | dict(rows=SIZES[2] - 1)
    for call in (M.check_snapshot, M.snapshot_into):
        with pytest.raises(hiplib.CvoError, match=r"map 2: dst rows 254 .* below the map's 255 rows"):
            call(None, offered)
    untouched_behind(whole, [0] * 8)


# ---- 2. the statement: a restored twin goes on like the original
def history(hiplib, torch, M, k, tens, members, poses):
    R = mr.Map(M.max_rows, VOXEL)
    for t in range(5):
        M.integrate([k], [[tens[t]]], [[poses[t]]], [[t]]); R.update([members[t]], [poses[t]], [t])
    for t in (0, 1):
        M.remove([k], [[tens[t]]], [[poses[t]]], [[t]]); R.update([members[t]], [poses[t]], [t], -1)
    assert 0 < R.live < R.rows
    return R


def test_a_restored_twin_returns_the_original_s_bytes_from_every_later_call(hiplib, torch, reducer, window):
    members, poses = window
    tens = dev(torch, members)
    A = hiplib.CvoMaps(reducer, 2, 20000, VOXEL)
    R = history(hiplib, torch, A, 0, tens, members, poses)
    S = A.snapshot([0])
    reducer2 = hiplib.CvoReducer(4, 32768)
    B = hiplib.CvoMaps(reducer, 1, R.rows + 4000, VOXEL)               # another max_rows: another table size
    C = hiplib.CvoMaps(reducer2, 3, 20000, VOXEL)                      # another reducer
    A.restore([1], S); B.restore([0], S); C.restore([2], S)
    where = [(A, 0), (A, 1), (B, 0), (C, 2)]
    for M, k in where:
        is_reading(M, k, R, ("restored", k))
    dead = [r for r in range(R.rows) if R.count[r] == 0]
    rows_before = R.rows

    def every(call, keys):
        """the call on the original and on each twin: every named output equal to the original's, byte for byte"""
        outs = [call(M, k) for M, k in where]
        for o in outs[1:]:
            for key in keys:
                a, b = outs[0][key], o[key]
                if hasattr(a, "cpu") or isinstance(a, np.ndarray):
                    a, b = host(a), host(b)
                    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key
                else:
                    assert a == b, key
        return outs[0]

    def update(M, k):
        M.integrate([k], [[tens[5], tens[0]]], [[poses[5], poses[0]]], [[5, 40]])
        M.remove([k], [[tens[2]]], [[poses[2]]], [[2]], present=True)
        return {}
    every(update, ())
    R.update([members[5], members[0]], [poses[5], poses[0]], [5, 40]); R.update([members[2]], [poses[2]], [2], -2)
    assert any(R.count[r] > 0 for r in dead) and R.rows > rows_before  # a dead row revived, new rows born
    for M, k in where:
        is_reading(M, k, R, ("updated", k))
    for flt in (dict(min_views=0, min_last_stamp=-2 ** 31), dict(min_points=3), dict(min_views=2), dict(min_last_stamp=5)):
        e = every(lambda M, k: M.extract([k], want=MAP_WANT, **flt)[0], mr.OUTPUTS + ("n_out",))
        assert 0 < e["n_out"] <= R.rows
    E = R.extract()
    obs = up_depth(torch, vw.shifted_rendering((E["xyz"], E["feat"]), EYE, SHEET_CAM, (64, 48)))
    keys = ("xyz", "feat", "source", "pixel", "map", "depth", "index", "relation", "carve", "n_out")
    views = []

    def view(M, k):
        # (the depth image lives on the first reducer's device: the same GPU)
        v = M.view([k], [EYE], SHEET_CAM, (64, 48), 2, "surface", 0.05, observed=[obs], want=("source", "pixel", "relation", "map", "depth", "index"), carve=True)[0]
        views.append(v)
        return v
    v = every(view, keys)
    assert v["n_out"] > 100 and 0 < int(host(v["carve"]).sum()) < v["n_out"]
    world = fr.moved_concat([members[6]], [poses[6]])
    cloud = dev(torch, [(np.ascontiguousarray(world[0]), np.ascontiguousarray(world[1]))])
    for reach in (0, 1):
        p = every(lambda M, k: M.probe([k], cloud, [EYE], reach=reach, want=("dist2", "count", "views", "last_stamp"), hit=True)[0],
                  ("row", "dist2", "count", "views", "last_stamp", "hit"))
        assert p["counts"][0] > 100 and p["counts"].sum() == world[0].shape[0]
    drops = iter(views)
    c = every(lambda M, k: dict(zip(("rows", "new_row"), (lambda o: (o[0].tolist(), o[1][0]))(M.compact([k], drop=[next(drops)["carve"]], new_row=True)))), ("rows", "new_row"))
    new_row = R.compact(drop=host(v["carve"]))
    assert c["rows"] == [R.rows] and host(c["new_row"]).tobytes() == new_row.tobytes()
    first = to_host(A.snapshot([0])[0])
    for M, k in where:
        is_reading(M, k, R, ("compacted", k))
        assert sr.same_snapshot(to_host(M.snapshot([k])[0]), first)
    for M in (A, B, C):
        M.close()
    reducer2.close()


# ---- 3. states no integration gives cheaply
def rows_of_cells(cells, seed, dead=()):
    """a supported state with one row per integer cell: (arrays in the header's types, xyz: a point inside each cell)"""
    rng = np.random.default_rng(seed)
    n = cells.shape[0]
    xyz = tc.positions(cells)
    ok, key = tc.keys_of(xyz)
    assert ok.all() and np.unique(key).shape[0] == n
    count = rng.integers(1, 6, n).astype(np.uint32)
    count[list(dead)] = 0
    P = np.concatenate([xyz, rng.uniform(0, 255, (n, 5)).astype(np.float32)], axis=1)
    sums = np.rint(P.astype(np.float64) * 16777216.0).astype(np.int64) * count.astype(np.int64)[:, None]
    mask = rng.integers(1, 2 ** 62, n).astype(np.uint64); mask[list(dead)] = 0
    last = rng.integers(0, 50, n).astype(np.int32)
    arrays = dict(keys=key.astype(np.uint64), sums=sums, count=count, view_mask=mask, last_stamp=last, born=(last // 2).astype(np.int32))
    return arrays, xyz


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(77)
    cells = np.unique(rng.integers(-4000, 4001, (BIG + 2000, 3)), axis=0)
    cells = cells[rng.permutation(cells.shape[0])[:BIG]]
    assert cells.shape[0] == BIG
    arrays, xyz = rows_of_cells(cells, 78, dead=(7, 66000))
    assert sr.refusal_bits(arrays) == 0
    return arrays, xyz


def finds_every_row(torch, M, k, arrays, xyz, what=""):
    """a probe at reach 0 with one point inside each row's cell: row r for a live row, -4 (present, filtered) for a dead one"""
    n = xyz.shape[0]
    if n == 0:
        return
    p = M.probe([k], dev(torch, [(xyz, np.zeros((n, 5), np.float32))]), [EYE], reach=0, min_views=0, min_last_stamp=-2 ** 31, want=("count",), hit=True)[0]
    alive = arrays["count"] >= 1
    want = np.where(alive, np.arange(n), -4).astype(np.int32)
    assert host(p["row"]).tobytes() == want.tobytes(), what
    assert host(p["count"]).tobytes() == np.where(alive, arrays["count"], 0).astype(np.int32).tobytes(), what
    assert host(p["hit"]).tobytes() == alive.astype(np.uint8).tobytes() and p["counts"].tolist() == [int(alive.sum()), 0, int(n - alive.sum()), 0], what


def test_rows_exactly_max_rows_past_65536_straight_from_arrays(hiplib, torch, reducer, big):
    arrays, xyz = big
    M = hiplib.CvoMaps(reducer, 1, BIG, tc.VOXEL)
    M.restore([0], to_dev(torch, arrays))
    rows, live = M.rows([0])
    assert (int(rows[0]), int(live[0])) == (BIG, BIG - 2)
    assert sr.same_snapshot(to_host(M.snapshot([0])[0]), arrays)
    finds_every_row(torch, M, 0, arrays, xyz, "big")
    S = hiplib.CvoMaps(reducer, 1, BIG - 1, tc.VOXEL)
    with pytest.raises(hiplib.CvoError, match=f"src rows {BIG} is outside 0 .. max_rows {BIG - 1}"):
        S.restore([0], to_dev(torch, arrays))
    S.close(); M.close()


@pytest.mark.parametrize("make,n", [(tc.last_slot, 64), (tc.last_slot, 257), (tc.staircase, 257), (tc.staircase, 64)])
def test_clustered_keys_with_a_dead_row_among_them(hiplib, torch, reducer, make, n):
    case = make(n)                                                     # homes for a table of 2 n slots: max_rows = n
    arrays, xyz = rows_of_cells(case["cells"], 500 + n, dead=(3, n - 2))
    assert np.array_equal(tc.home_slot(arrays["keys"], 2 * n), case["homes"])
    M = hiplib.CvoMaps(reducer, 2, n, tc.VOXEL)
    M.restore([1], to_dev(torch, arrays))
    finds_every_row(torch, M, 1, arrays, xyz, case["name"])
    R = sr.restore(arrays, n, tc.VOXEL)
    cloud = (np.ascontiguousarray(xyz[:8]), tc.features(8, 1))         # adds to rows 0 .. 7 and revives the dead row 3
    M.integrate([1], [dev(torch, [cloud])], [[EYE]], [[60]]); R.update([cloud], [EYE], [60])
    assert R.rows == n and R.count[3] == 1 and R.born[3] == 60
    is_reading(M, 1, R, case["name"])
    M.close()


# ---- 4. refusals
def small_states(seed):
    """five different supported states of a few hundred rows, each with dead rows"""
    out = []
    for k in range(5):
        n = 300 + 17 * k
        i = np.arange(n, dtype=np.int64)
        cells = np.stack([i + seed, 3 * i - 50 * k, 7 * k - i], axis=1)
        out.append(rows_of_cells(cells, 10 * seed + k, dead=(0, 64 + k, n - 1)))
    return out


def test_every_refusal_names_map_and_bits_and_leaves_every_listed_map_as_it_was(hiplib, torch, reducer, big):
    A = hiplib.CvoMaps(reducer, 5, BIG, tc.VOXEL)
    T = hiplib.CvoMaps(reducer, 5, 5000, tc.VOXEL)                     # the untouched twin: never sees a refused restore
    old = small_states(1)
    for M in (A, T):
        M.restore(None, [to_dev(torch, a) for a, _ in old])
    offer = small_states(2)                                            # what the refused calls would put in: other rows than the maps hold
    order = [4, 0, 2, 1, 3]                                            # the offending map is the third of the call's five

    def spoil(field, row, value, col=None, base=None):
        a = {k: v.copy() for k, v in (offer[2][0] if base is None else base).items()}
        if col is None:
            a[field][row] = value
        else:
            a[field][row, col] = value
        return a

    good = offer[2][0]
    two = spoil("last_stamp", 200, -1); two["keys"][11] = two["keys"][10]
    far = spoil("keys", 66005, big[0]["keys"][5], base=big[0])
    cases = [("bad key", sr.BAD_KEY, spoil("keys", 100, np.uint64(1 << 63) | good["keys"][100])),
             ("empty mark", sr.BAD_KEY, spoil("keys", 299, np.uint64(2 ** 64 - 1))),
             ("count", sr.BAD_COUNT, spoil("count", 5, np.uint32(mr.MAX_COUNT + 1))),
             ("stamp", sr.BAD_STAMP, spoil("born", 257, -3)),
             ("sum", sr.BAD_SUM, spoil("sums", 0, -1, col=7)),                          # (row 0 is dead: its bound is 0)
             ("sum of a live row", sr.BAD_SUM, spoil("sums", 9, int(good["count"][9]) * sr.SUM_BOUND + 1, col=2)),
             ("duplicate one row apart", sr.DUPLICATE, spoil("keys", 256, good["keys"][255])),
             ("duplicate 66 000 rows apart", sr.DUPLICATE, far),
             ("two kinds", sr.BAD_STAMP | sr.DUPLICATE, two)]
    extra = lattice(40, 3)
    stamp = 50
    for name, bits, bad in cases:
        assert sr.refusal_bits(bad) == bits, name
        before = [to_host(s) for s in A.snapshot(None)]
        snaps = [to_dev(torch, bad if k == 2 else offer[k][0]) for k in order]
        A.check_restore(order, snaps)                                  # the host finds nothing wrong: the rows are tested on the device
        with pytest.raises(hiplib.CvoError, match=rf"map 2 \(entry 2\): the rows are refused, bits {bits}:"):
            A.restore(order, snaps)
        rows, live = A.rows(None)
        for k, (s, (a, xyz)) in enumerate(zip(A.snapshot(None), old)):
            assert sr.same_snapshot(to_host(s), before[k]), (name, k)
            assert (int(rows[k]), int(live[k])) == (len(before[k]["keys"]), int((before[k]["count"] >= 1).sum())), (name, k)
            finds_every_row(torch, A, k, a, xyz, (name, k))             # the table really was built again, dead rows' keys included
        # the next integration behaves as on the untouched twin: old rows, a dead row revived, new rows born
        cloud = (np.concatenate([old[1][1][:3], extra[0]]), np.concatenate([tc.features(3, 5), extra[1]]))
        for M in (A, T):
            M.integrate([1, 3], [dev(torch, [cloud]), dev(torch, [extra])], [[EYE], [EYE]], [[stamp], [stamp]])
        stamp += 1
        for a, t in zip(A.snapshot(None), T.snapshot(None)):
            assert sr.same_snapshot(to_host(a), to_host(t)), name
        old = [(to_host(s), None) for s in A.snapshot(None)]
        old = [(a, xyz_of(a)) for a, _ in old]
    A.restore(order, [to_dev(torch, offer[k][0]) for k in order])      # and the same call without the spoiled row goes through
    for k in range(5):
        assert sr.same_snapshot(to_host(A.snapshot([k])[0]), offer[k][0])
        finds_every_row(torch, A, k, *offer[k], ("accepted", k))
    A.close(); T.close()


def xyz_of(arrays):
    """a point inside the cell of each row's key, at tc.VOXEL"""
    k = arrays["keys"].astype(np.uint64)
    cells = np.stack([((k >> np.uint64(s)) & np.uint64(0x1FFFFF)).astype(np.int64) - 2 ** 20 for s in (42, 21, 0)], axis=1)
    return tc.positions(cells)


def test_the_host_refuses_rows_above_max_rows_a_wrong_voxel_and_bad_arrays(hiplib, torch, reducer):
    M = hiplib.CvoMaps(reducer, 2, 300, tc.VOXEL)
    arrays, xyz = small_states(3)[0]
    assert len(arrays["keys"]) == 300
    M.restore([0], to_dev(torch, arrays))
    before = to_host(M.snapshot([0])[0])
    more, _ = rows_of_cells(np.stack([np.arange(301), np.arange(301), np.arange(301)], axis=1), 4)
    for call in (M.check_restore, M.restore):
        with pytest.raises(hiplib.CvoError, match="map 0: src rows 301 is outside 0 .. max_rows 300"):
            call([0], [to_dev(torch, more)])
        with pytest.raises(hiplib.CvoError, match="voxel .* has not the bits of the object's voxel"):
            call([0], [to_dev(torch, arrays)], voxel=np.nextafter(np.float32(tc.VOXEL), np.float32(1)))
        with pytest.raises(ValueError, match="map 0 appears twice"):
            call([0, 0], [to_dev(torch, arrays)] * 2)
        with pytest.raises(ValueError, match="keys has 300 rows, below rows 301"):
            call([0], [dict(to_dev(torch, arrays), rows=301)])
    M.restore([1], [dict(rows=0)])                                     # rows == 0 with no arrays: an empty map
    M.restore([0], [to_dev(torch, {k: v[:0] for k, v in arrays.items()})]); M.restore([0], to_dev(torch, arrays))
    assert M.rows([1])[0].tolist() == [0] and sr.same_snapshot(to_host(M.snapshot([0])[0]), before)
    finds_every_row(torch, M, 0, arrays, xyz, "after an empty restore")
    M.close()


# ---- 5. the python helpers
def test_grown_is_the_remedy_for_a_full_map(hiplib, torch, reducer):
    n = 500
    x, f = lattice(n + 10, 1)
    M = hiplib.CvoMaps(reducer, 2, n, tc.VOXEL)
    R = mr.Map(n + 100, tc.VOXEL)
    first, rest = (x[:n], f[:n]), (x[n - 5:], f[n - 5:])
    M.integrate([1], [dev(torch, [first])], [[EYE]], [[0]]); R.update([first], [EYE], [0])
    assert M.rows([1])[0].tolist() == [n]
    with pytest.raises(hiplib.CvoError, match="above max_rows 500"):
        M.integrate([1], [dev(torch, [rest])], [[EYE]], [[1]])
    G = M.grown(n + 100)
    assert G.info()["max_rows"] == n + 100 and G.info()["max_maps"] == 2 and G.reducer is M.reducer
    G.integrate([1], [dev(torch, [rest])], [[EYE]], [[1]]); R.update([rest], [EYE], [1])
    assert R.rows == n + 10
    is_reading(G, 1, R, "grown")
    is_reading(G, 0, mr.Map(n + 100, tc.VOXEL), "grown, empty")
    assert M.rows([1])[0].tolist() == [n]                              # the old object stays as it was
    M.close(); G.close()


def test_save_and_load_round_trip_through_a_file(hiplib, torch, reducer, eight, tmp_path):
    from cvo_slam_amd.voxels import load_maps, save_maps
    M, R = eight
    snaps = M.snapshot(None)
    path = tmp_path / "maps.npz"
    save_maps(path, snaps, M.voxel)
    loaded, voxel = load_maps(path, reducer.device)
    assert np.float32(voxel).tobytes() == np.float32(M.voxel).tobytes() and len(loaded) == 8
    on_host, _ = load_maps(path)
    N = hiplib.CvoMaps(reducer, 8, 4000, tc.VOXEL)
    N.restore(None, loaded, voxel=voxel)
    for k in range(8):
        assert sr.same_snapshot(to_host(loaded[k]), sr.snapshot(R[k])) and sr.same_snapshot(on_host[k], sr.snapshot(R[k])), k
        assert on_host[k]["keys"].dtype == np.uint64 and on_host[k]["count"].dtype == np.uint32
        is_reading(N, k, R[k], ("loaded", k))
    N.close()


# ---- 6. streams and interleaving
def test_the_stream_rule_orders_snapshots_and_restores(hiplib, torch, reducer, window):
    members, poses = window[0][:3], window[1][:3]
    R = mr.Map(20000, VOXEL); R.update(members, poses, [0, 1, 2])
    side = torch.cuda.Stream()
    pinned = [(torch.from_numpy(x).pin_memory(), torch.from_numpy(f).pin_memory()) for x, f in members]
    tens = [(torch.full(x.shape, 1000.0, dtype=torch.float32, device="cuda"), torch.zeros(f.shape, dtype=torch.float32, device="cuda"), "points_first") for x, f in members]
    a = torch.randn((4096, 4096), device="cuda")
    M = hiplib.CvoMaps(reducer, 2, 20000, VOXEL)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):                                             # work in front of the writes
            a = a @ a * 1e-3
        for (tx, tf, _), (hx, hf) in zip(tens, pinned):
            tx.copy_(hx, non_blocking=True); tf.copy_(hf, non_blocking=True)
    M.integrate([0], [tens], [poses], [[0, 1, 2]], cloud_stream=side)
    snap = M.snapshot([0], stream=side)                                # queued behind the integration: it sees it
    M.restore([1], snap, stream=side)                                  # behind the snapshot of the same arrays: ordered by the stream
    with torch.cuda.stream(side):
        kept = {k: snap[0][k].clone() for k in sr.FIELDS}
        for k in sr.FIELDS:
            snap[0][k].zero_()                                         # an overwrite behind the restore's read
    again = M.snapshot([1], stream=side)
    side.synchronize()
    assert sr.same_snapshot(to_host(kept), sr.snapshot(R)) and sr.same_snapshot(to_host(again[0]), sr.snapshot(R))
    is_reading(M, 0, R, "original"); is_reading(M, 1, R, "twin")
    M.close()


def test_reduce_fuse_view_updates_probes_snapshots_and_restores_interleaved(hiplib, torch, reducer, window):
    members, poses = window[0][:4], window[1][:4]
    tens = dev(torch, members)
    M = hiplib.CvoMaps(reducer, 3, 20000, VOXEL)
    R = mr.Map(20000, VOXEL)
    scratch = reducer.scratch_bytes()
    side = torch.cuda.Stream()
    for t in range(4):
        M.integrate([1], [[tens[t]]], [[poses[t]]], [[t]]); R.update([members[t]], [poses[t]], [t])
        g = reducer.reduce([tens[t]], VOXEL, "mean", 1, want=("count",))[0]
        w = vr.reduce_reading(members[t][0], members[t][1], VOXEL, "mean", 1)
        assert g["n_out"] == w["n_out"] and host(g["xyz"]).tobytes() == w["xyz"].tobytes()
        snap = M.snapshot([1], stream=side)                            # no host wait ...
        f = reducer.fuse([tens[:t + 1]], [poses[:t + 1]], VOXEL, want=("count",))[0]   # ... and the next call on the reducer writes its table
        assert f["n_out"] == fr.fuse_reading(members[:t + 1], poses[:t + 1], VOXEL)["n_out"]
        p = M.probe([1], [tens[t]], [poses[t]], counts=False, cloud_stream=side)[0]
        M.restore([2 if t % 2 else 0], snap, stream=side)
        v = M.view([2 if t % 2 else 0], [EYE], SHEET_CAM, (64, 48), 2, want=("source",))[0]
        assert v["n_out"] > 50
        side.synchronize()
        assert (host(p["row"]) >= 0).all()
        is_reading(M, 2 if t % 2 else 0, R, t); is_reading(M, 1, R, t)
        if t >= 1:
            M.remove([0 if t % 2 else 2], [[tens[0]]], [[poses[0]]], [[0]])   # the other twin, one step behind, goes its own way
    assert reducer.scratch_bytes() == scratch
    M.close()
