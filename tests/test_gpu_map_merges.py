"""Merging resident maps (cvo_maps_merge, CvoMaps.merge / check_merge / coarser) against the reading of the definition
(tests/map_merge_reading.py on map_reading.Map): every byte of a destination's snapshot and its row counts, after merges into empty and
populated maps at levels 0, 1, 2 and 4, under the filter, at the cell edges, at the row and count bounds, and through every later call."""
import numpy as np
import pytest

import fuse_reading as fr
import map_merge_reading as gr
import map_reading as mr
import map_snapshot_reading as sr
import table_cases as tc
from test_gpu_map_snapshots import dev, host, is_reading, lattice, lattice_history, to_dev, to_host
from test_gpu_map_views import SHEET_CAM
from test_gpu_maps import WANT as MAP_WANT, same

pytestmark = pytest.mark.gpu

EYE = np.eye(4, dtype=np.float32)
VOXEL = np.float32(0.05)
SIZES = (0, 1, 63, 64, 65, 255, 256, 257)
LEVELS = (0, 1, 2, 4)
TOP = (1 << 20) - 1


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
def scene():
    return mr.sliding_windows(np.random.default_rng(5), members=10, n=3000)


def at_level(voxel, level):
    return np.float32(np.ldexp(np.float32(voxel), level))


def restored(hiplib, torch, reducer, R, max_maps=1, k=0, max_rows=None):
    """a device object whose map k is the reading R's rows"""
    M = hiplib.CvoMaps(reducer, max_maps, R.max_rows if max_rows is None else max_rows, float(R.voxel))
    M.restore([k], to_dev(torch, sr.snapshot(R)))
    return M


def all_snapshots(M):
    return [to_host(s) for s in M.snapshot(None)]


def unchanged(M, before):
    return all(sr.same_snapshot(a, b) for a, b in zip(all_snapshots(M), before))


@pytest.fixture(scope="module")
def sources(hiplib, torch, reducer):
    S = hiplib.CvoMaps(reducer, 8, 300, tc.VOXEL)
    R = [lattice_history(hiplib, torch, S, k, n) for k, n in enumerate(SIZES)]
    assert [r.rows for r in R] == list(SIZES) and all(0 < r.live < r.rows for r in R if r.rows >= 4)   # dead and revived rows in each
    yield S, R
    S.close()


# ---- 1. sizes and the shape of a call
@pytest.mark.parametrize("level", LEVELS)
def test_eight_merges_a_call_into_empty_and_populated_maps(hiplib, torch, reducer, sources, level):
    S, RS = sources
    voxel = at_level(tc.VOXEL, level)
    D = hiplib.CvoMaps(reducer, 9, 700, float(voxel))
    RD = [mr.Map(700, voxel) for _ in range(9)]
    for k, keep in ((3, False), (7, False), (5, True)):                  # destinations that hold rows already: all dead (3, 7) or half dead (5)
        x, f = lattice(257, k)
        for cloud, sign in (((x[:100], f[:100]), 1), ((x[:100 if not keep else 50], f[:100 if not keep else 50]), -1)):
            (D.integrate if sign > 0 else D.remove)([k], [dev(torch, [cloud])], [[EYE]], [[9]]); RD[k].update([cloud], [EYE], [9], sign)
        assert RD[k].rows > 0 and RD[k].live == (RD[k].rows - sum(1 for c in RD[k].count if c == 0)) and (RD[k].live == 0) == (not keep)
    before = to_host(S.snapshot([7])[0])
    dead_before = {k: [r for r in range(RD[k].rows) if RD[k].count[r] == 0] for k in (3, 5, 7)}
    pairs = [(0, 7), (1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (6, 6), (7, 7)]   # source 7 goes into two destinations
    D.check_merge([d for d, s in pairs], S, [s for d, s in pairs], level=level)
    D.merge([d for d, s in pairs], S, [s for d, s in pairs], level=level)
    for d, s in pairs:
        gr.merge(RD[d], RS[s], level)
    for k in (3, 5, 7):
        assert any(RD[k].count[r] > 0 for r in dead_before[k]), k       # an incoming cell revived a dead destination row
    for k in range(9):
        is_reading(D, k, RD[k], ("first", level, k))
    D.merge([8], S, [0], level=level)                                    # a source without rows: nothing changes
    D.merge([0, 1, 2, 3, 4, 5, 6, 7], S, [1, 2, 3, 4, 5, 6, 7, 0], level=level)   # everything again, into populated maps
    for d, s in zip(range(8), [1, 2, 3, 4, 5, 6, 7, 0]):
        gr.merge(RD[d], RS[s], level)
    for k in range(9):
        is_reading(D, k, RD[k], ("second", level, k))
    for k in range(8):
        is_reading(S, k, RS[k], ("source", k))                           # the sources are only read
    assert sr.same_snapshot(to_host(S.snapshot([7])[0]), before)
    D.close()


@pytest.mark.parametrize("level", LEVELS)
def test_3000_rows_with_dead_and_revived_rows(hiplib, torch, reducer, level):
    S = hiplib.CvoMaps(reducer, 1, 3000, tc.VOXEL)
    R = lattice_history(hiplib, torch, S, 0, 3000)
    assert R.rows == 3000 and 0 < R.live < 3000
    D = S.coarser(level)
    want = gr.coarser(R, level)
    assert (want.rows < 3000) == (level >= 2) and want.rows > 256        # (the lattice's y cell is 2 k - 7: distinct cells up to level 1; more than one block of call-cells at every level)
    is_reading(D, 0, want, level)
    D.close(); S.close()


# ---- 2. the filter
def test_the_filter_keeps_drops_and_never_passes_a_dead_row(hiplib, torch, reducer, scene):
    members, poses = scene
    R = gr.window_history(mr.Map(4000, VOXEL), members, poses, 4)
    S = restored(hiplib, torch, reducer, R)
    flt = dict(min_views=2, min_last_stamp=8)
    keep = gr.kept(R, False, 1, **flt)
    dead = [r for r in range(R.rows) if R.count[r] == 0]
    dropped = [r for r in range(R.rows) if R.count[r] >= 1 and r not in set(keep)]
    assert len(keep) > 100 and len(dropped) > 100 and len(dead) > 100 and not set(keep) & set(dead)
    assert any(bin(R.mask[r]).count("1") < 2 for r in dropped) and any(R.last[r] < 8 for r in dropped)
    for level in (0, 1):
        D = hiplib.CvoMaps(reducer, 2, 4000, float(at_level(VOXEL, level)))
        D.merge([1, 0], S, [0, 0], level=level, all_rows=[False, True], min_points=1, min_views=[2, 0], min_last_stamp=[8, 0])
        is_reading(D, 1, gr.merge(mr.Map(4000, at_level(VOXEL, level)), R, level, all_rows=False, **flt), ("filtered", level))
        is_reading(D, 0, gr.coarser(R, level, 4000), ("all rows", level))
        D.close()
    S.close()


# ---- 3. cell edges
def rows_at(cells, seed, dead=()):
    """a supported state with one row per given cell (cells past +-2^15 / voxel hold no valid point: the sums are small numbers of their own)"""
    rng = np.random.default_rng(seed)
    n = len(cells)
    count = rng.integers(1, 6, n).astype(np.uint32); count[list(dead)] = 0
    sums = rng.integers(-2 ** 30, 2 ** 30, (n, 8)).astype(np.int64) * count.astype(np.int64)[:, None]
    mask = rng.integers(1, 2 ** 62, n).astype(np.uint64); mask[list(dead)] = 0
    last = rng.integers(0, 50, n).astype(np.int32)
    return dict(keys=np.asarray([gr.key_of(c) for c in cells], np.uint64), sums=sums, count=count, view_mask=mask, last_stamp=last, born=(last // 2).astype(np.int32))


@pytest.mark.parametrize("level", LEVELS)
def test_cells_at_the_edges_and_negative_cells(hiplib, torch, reducer, level):
    cells = [(TOP, TOP, TOP), (-TOP, -TOP, -TOP), (TOP, -TOP, 0), (-1, -1, -1), (-2, -2, -2), (-1, 0, -2), (0, 0, 0), (1, 1, 1), (-TOP + 1, TOP - 1, -3),
             (TOP - 1, TOP, TOP), (-16, -17, 15), (-32, 31, -33)]
    arrays = rows_at(cells, 11, dead=(4, 9))
    assert sr.refusal_bits(arrays) == 0
    R = sr.restore(arrays, 64, tc.VOXEL)
    S = restored(hiplib, torch, reducer, R)
    D = S.coarser(level, max_rows=12)
    want = gr.coarser(R, level, 12)
    assert {(TOP >> level,) * 3, ((-TOP) >> level,) * 3, (-1, -1, -1)} <= {gr.cell_of(k) for k in want.key}
    assert (want.rows < 12) == (level > 0)
    is_reading(D, 0, want, level)
    D.close(); S.close()


# ---- 4. against history twins on the device
@pytest.mark.parametrize("level", [1, 2, 4])
def test_a_coarse_merge_is_the_twin_with_the_same_history_but_for_born(hiplib, torch, reducer, scene, level):
    members, poses = scene
    tens = dev(torch, members)
    both = [hiplib.CvoMaps(reducer, 1, 4000, float(at_level(VOXEL, k))) for k in (0, level)]
    for m in range(10):
        for M in both:
            M.integrate([0], [[tens[m]]], [[poses[m]]], [[m]])
            if m >= 4:
                M.remove([0], [[tens[m - 4]]], [[poses[m - 4]]], [[m - 4]])
    fine, twin = both
    R = gr.window_history(mr.Map(4000, VOXEL), members, poses, 4)
    is_reading(fine, 0, R, "fine")
    D = fine.coarser(level)
    assert D.voxel == float(at_level(VOXEL, level)) and D.max_rows == 4000 and D.reducer is reducer
    is_reading(D, 0, gr.coarser(R, level), ("merged", level))
    got, want = to_host(D.snapshot([0])[0]), to_host(twin.snapshot([0])[0])
    assert len(got["keys"]) > 10 and (got["count"] == 0).any()
    for name in sr.FIELDS:
        if name != "born":
            assert got[name].tobytes() == want[name].tobytes(), name
    assert (got["born"] >= want["born"])[got["count"] >= 1].all()
    assert D.rows([0])[1].tolist() == twin.rows([0])[1].tolist()
    for M in (fine, twin, D):
        M.close()


def test_a_level_0_union_of_a_fork_is_the_one_map(hiplib, torch, reducer, scene):
    members, poses = scene
    tens = dev(torch, members)
    A = hiplib.CvoMaps(reducer, 3, 4000, float(VOXEL))
    whole = mr.Map(4000, VOXEL)
    for m in range(10):
        A.integrate([0 if m < 5 else 1], [[tens[m]]], [[poses[m]]], [[m]]); whole.update([members[m]], [poses[m]], [m])
    A.restore([2], A.snapshot([0]))                                      # the fork
    A.merge([2], A, [1])                                                 # source and destination in one object
    is_reading(A, 2, whole, "union")
    with pytest.raises(ValueError, match="map 2 is both a source and a destination"):
        A.merge([2, 0], A, [1, 2])
    is_reading(A, 2, whole, "after the refusal")
    A.close()


# ---- 5. later calls on a merged map
def test_later_calls_on_a_merged_map_are_those_on_a_restored_twin(hiplib, torch, reducer, scene):
    from test_gpu_view_clouds import up_depth
    import view_reading as vw
    members, poses = scene
    tens = dev(torch, members)
    R0 = gr.window_history(mr.Map(4000, VOXEL), members, poses, 4, upto=8)
    S = restored(hiplib, torch, reducer, R0)
    D = S.coarser(1)
    R = gr.coarser(R0, 1)
    reducer2 = hiplib.CvoReducer(2, 32768)
    T = restored(hiplib, torch, reducer2, R)
    where = [(D, 0), (T, 0)]

    def every(call, keys):
        outs = [call(M, k) for M, k in where]
        for key in keys:
            a, b = outs[0][key], outs[1][key]
            if hasattr(a, "cpu") or isinstance(a, np.ndarray):
                a, b = host(a), host(b)
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key
            else:
                assert a == b, key
        return outs[0]

    def update(M, k):
        M.integrate([k], [[tens[8], tens[0]]], [[poses[8], poses[0]]], [[8, 40]])
        M.remove([k], [[tens[6]]], [[poses[6]]], [[6]], present=True)
        return {}
    dead = [r for r in range(R.rows) if R.count[r] == 0]
    every(update, ())
    R.update([members[8], members[0]], [poses[8], poses[0]], [8, 40]); R.update([members[6]], [poses[6]], [6], -2)
    assert dead and any(R.count[r] > 0 for r in dead)
    for M, k in where:
        is_reading(M, k, R, "updated")
    for flt in (dict(min_views=0, min_last_stamp=-2 ** 31), dict(min_points=3), dict(min_views=2), dict(min_last_stamp=7)):
        e = every(lambda M, k: M.extract([k], want=MAP_WANT, **flt)[0], mr.OUTPUTS + ("n_out",))
        assert 0 < e["n_out"] <= R.rows
    E = R.extract()
    obs = up_depth(torch, vw.shifted_rendering((E["xyz"], E["feat"]), EYE, SHEET_CAM, (64, 48)))
    views = []

    def view(M, k):
        v = M.view([k], [EYE], SHEET_CAM, (64, 48), 2, "surface", 0.05, observed=[obs], want=("source", "pixel", "relation", "map", "depth", "index"), carve=True)[0]
        views.append(v)
        return v
    v = every(view, ("xyz", "feat", "source", "pixel", "map", "depth", "index", "relation", "carve", "n_out"))
    assert v["n_out"] > 50
    world = fr.moved_concat([members[9]], [poses[9]])
    cloud = dev(torch, [(np.ascontiguousarray(world[0]), np.ascontiguousarray(world[1]))])
    for reach in (0, 1):
        p = every(lambda M, k: M.probe([k], cloud, [EYE], reach=reach, want=("dist2", "count", "views", "last_stamp"), hit=True)[0],
                  ("row", "dist2", "count", "views", "last_stamp", "hit"))
        assert p["counts"][0] > 100
    drops = iter(views)
    c = every(lambda M, k: dict(zip(("rows", "new_row"), (lambda o: (o[0].tolist(), o[1][0]))(M.compact([k], drop=[next(drops)["carve"]], new_row=True)))), ("rows", "new_row"))
    R.compact(drop=host(v["carve"]))
    assert c["rows"] == [R.rows]
    for M, k in where:
        is_reading(M, k, R, "compacted")
    for M in (S, D, T):
        M.close()
    reducer2.close()


# ---- 6. row and count bounds; every refusal leaves every map of both objects as it was
def test_max_rows_exact_and_one_short(hiplib, torch, reducer, sources):
    S, RS = sources
    voxel = at_level(tc.VOXEL, 1)
    want = gr.coarser(RS[7], 1)
    src_before = all_snapshots(S)
    x, f = lattice(65, 4)
    far = (np.ascontiguousarray(x + np.float32(4096.0)), f)              # rows of its own, far from every source cell
    own = mr.Map(1000, voxel); own.update([far], [EYE], [0])
    assert own.rows > 10 and not set(own.key) & set(want.key)
    for short in (0, 1):
        D = hiplib.CvoMaps(reducer, 3, own.rows + want.rows - short, float(voxel))
        D.integrate([1], [dev(torch, [far])], [[EYE]], [[0]])
        before = all_snapshots(D)
        if short:
            with pytest.raises(hiplib.CvoError, match=rf"map 1 \(merge 1\): its {own.rows} rows and the merge's {want.rows} new cells are above max_rows {D.max_rows}"):
                D.merge([0, 1], S, [3, 7], level=1)
            assert unchanged(D, before) and unchanged(S, src_before)     # map 0's merge was not written either
            assert D.rows(None)[0].tolist() == [0, own.rows, 0]
        else:
            D.merge([0, 1], S, [3, 7], level=1)
            R1 = mr.Map(D.max_rows, voxel); R1.update([far], [EYE], [0])
            is_reading(D, 1, gr.merge(R1, RS[7], 1), "exact")
            assert D.rows([1])[0].tolist() == [D.max_rows]
            is_reading(D, 0, gr.coarser(RS[3], 1, D.max_rows), "beside it")
        D.close()


def full_rows(cells):
    n = len(cells)
    return dict(keys=np.asarray([gr.key_of(c) for c in cells], np.uint64), sums=np.ones((n, 8), np.int64), count=np.full(n, mr.MAX_COUNT, np.uint32),
                view_mask=np.ones(n, np.uint64), last_stamp=np.zeros(n, np.int32), born=np.zeros(n, np.int32))


def test_the_count_bound_and_the_wrap(hiplib, torch, reducer):
    pair = full_rows([(0, 0, 0), (1, 0, 0), (-7, 2, 2)])                 # two children of 16777215 each, and a cell of its own ...
    pair["last_stamp"][2] = 5                                            # ... which min_last_stamp = 5 keeps alone
    many = full_rows([(j % 16, (j // 16) % 16, 16 + j // 256) for j in range(300)])   # 300 siblings of one level-4 cell: 300 x 16777215 > 2^32
    assert 300 * mr.MAX_COUNT > 2 ** 32 > (300 * mr.MAX_COUNT) % 2 ** 32 and len({gr.shifted(int(k), 4) for k in many["keys"]}) == 1
    S = hiplib.CvoMaps(reducer, 2, 300, tc.VOXEL)
    S.restore([0, 1], [to_dev(torch, pair), to_dev(torch, many)])
    RS = [sr.restore(pair, 300, tc.VOXEL), sr.restore(many, 300, tc.VOXEL)]
    src_before = all_snapshots(S)
    for level, src, ok in ((0, 0, True), (1, 0, False), (4, 0, False), (0, 1, True), (1, 1, False), (4, 1, False)):
        D = hiplib.CvoMaps(reducer, 2, 400, float(at_level(tc.VOXEL, level)))
        x, f = lattice(20, 1)
        D.integrate([0], [dev(torch, [(x, f)])], [[EYE]], [[3]])
        before = all_snapshots(D)
        if ok:
            D.merge([1], S, [src], level=level)
            is_reading(D, 1, gr.coarser(RS[src], level, 400), (level, src))
            with pytest.raises(hiplib.CvoError, match=r"map 1 \(merge 0\): the merge would take a cell's count above 16777215"):
                D.merge([1], S, [src], level=level)                      # once more: present rows at the bound
            is_reading(D, 1, gr.coarser(RS[src], level, 400), (level, src, "refused"))
        else:
            with pytest.raises(mr.Refused):
                gr.coarser(RS[src], level, 400)
            with pytest.raises(hiplib.CvoError, match=r"map 1 \(merge 1\): the merge would take a cell's count above 16777215"):
                _two(D, S, src, level)
            assert unchanged(D, before)
        assert unchanged(S, src_before)
        D.close()
    S.close()


def _two(D, S, src, level):
    """a call whose SECOND merge breaks the count bound: map 1 takes the source whole; map 0, which holds a lattice of its own, takes the one
    row of source map 0 that min_last_stamp = 5 keeps -- a merge that would be written if the call were not refused as a whole"""
    D.merge([0, 1], S, [0, src], level=level, all_rows=[False, True], min_last_stamp=[5, 0])


# ---- 7. other objects, the stream rule, other calls in between
def test_a_source_on_a_second_reducer_and_the_stream_rule(hiplib, torch, reducer, sources):
    S, RS = sources
    reducer2 = hiplib.CvoReducer(4, 1024)
    D = hiplib.CvoMaps(reducer2, 2, 500, float(at_level(tc.VOXEL, 2)))
    st = torch.cuda.Stream()
    D.merge([1], S, [7], level=2, stream=st)                             # (the source's writes are long done)
    st.synchronize()
    is_reading(D, 1, gr.coarser(RS[7], 2, 500), "second reducer")
    D.merge([0, 1], S, [6, 5], level=2, stream=st.cuda_stream)
    want = gr.merge(gr.coarser(RS[7], 2, 500), RS[5], 2)
    is_reading(D, 1, want, "again")
    is_reading(D, 0, gr.coarser(RS[6], 2, 500), "beside")
    D.close()
    small = hiplib.CvoReducer(2, 256)
    E = hiplib.CvoMaps(small, 1, 500, float(tc.VOXEL))
    E.merge([0], S, [6], level=0)                                        # 256 rows: exactly a region's points
    is_reading(E, 0, gr.coarser(RS[6], 0, 500), "256 rows on 256 points")
    before = all_snapshots(E)
    for call in (E.check_merge, E.merge):
        with pytest.raises(hiplib.CvoError, match=r"merge 0: source map 7 has 257 rows, above the 256 \(max_points\)"):
            call([0], S, [7], level=0)
    assert unchanged(E, before)
    E.close(); small.close(); reducer2.close()


def test_merges_between_every_other_kind_of_call_on_one_reducer(hiplib, torch, reducer, sources, scene):
    S, RS = sources
    members, poses = scene
    tens = dev(torch, members)
    D = hiplib.CvoMaps(reducer, 2, 2000, float(at_level(tc.VOXEL, 1)))
    other = hiplib.CvoMaps(reducer, 1, 4000, float(VOXEL))
    RO = mr.Map(4000, VOXEL)
    first = reducer.reduce([tens[0]], 0.05, "mean", 1, want=())[0]
    D.merge([0], S, [7], level=1)
    other.integrate([0], [[tens[1]]], [[poses[1]]], [[1]]); RO.update([members[1]], [poses[1]], [1])
    fused = reducer.fuse([[tens[0], tens[1]]], [[poses[0], poses[1]]], 0.05)[0]
    D.merge([1, 0], S, [5, 6], level=1)
    e = D.extract([0], min_views=0, want=MAP_WANT)[0]
    snap = other.snapshot([0])
    D.merge([1], S, [7], level=1)
    other.restore([0], snap)
    p = D.probe([1], [tens[2]], [poses[2]], reach=1)[0]
    D.compact([0])
    D.merge([0], S, [4], level=1)
    again = reducer.reduce([tens[0]], 0.05, "mean", 1, want=())[0]
    R0 = gr.merge(gr.coarser(RS[7], 1, 2000), RS[6], 1)
    same(e, R0.extract(min_views=0), "extract between merges", mr.OUTPUTS)
    R0.compact(); gr.merge(R0, RS[4], 1)
    is_reading(D, 0, R0, "map 0"); is_reading(D, 1, gr.merge(gr.coarser(RS[5], 1, 2000), RS[7], 1), "map 1"); is_reading(other, 0, RO, "other")
    assert host(first["xyz"]).tobytes() == host(again["xyz"]).tobytes() and fused["n_out"] > 0 and p["counts"].sum() == members[2][0].shape[0]
    D.close(); other.close()


# ---- 8. every refusal the host makes
def test_host_refusals_launch_nothing(hiplib, torch, reducer, sources):
    S, RS = sources
    from cvo_slam_amd import api
    D = hiplib.CvoMaps(reducer, 4, 600, float(at_level(tc.VOXEL, 1)))
    D.merge([3], S, [7], level=1)
    before, src_before = all_snapshots(D), all_snapshots(S)
    half = hiplib.CvoMaps(reducer, 1, 10, 0.2)                           # neither the source's voxel nor twice it
    L = D.L

    entry = [None]                                                     # the entry point under test: the check alone, then the call

    def raw(dst, recs, src, level, n=None):
        arr = (api.MapMerge * max(1, len(recs)))(*[api.MapMerge(d, s, a, 0, api.MapFilter(1, v, 0, 0)) for d, s, a, v in recs])
        fn, more = entry[0]
        api._check(fn(dst, len(recs) if n is None else n, arr, src, level, *more))
    ok = [(0, 1, 1, 0)]
    cases = [("null maps object", lambda: raw(None, ok, S.h, 1)), ("null maps object", lambda: raw(D.h, ok, None, 1)),
             ("count 0 is outside 1 .. the destination's max_maps 4", lambda: raw(D.h, ok, S.h, 1, n=0)), ("count 5 is outside", lambda: raw(D.h, ok * 5, S.h, 1)),
             ("level -1 is outside 0 .. 4", lambda: raw(D.h, ok, S.h, -1)), ("level 5 is outside 0 .. 4", lambda: raw(D.h, ok, S.h, 5)),
             ("has not the bits of the source's voxel", lambda: raw(D.h, ok, S.h, 0)), ("has not the bits of the source's voxel", lambda: raw(D.h, ok, S.h, 2)),
             ("has not the bits of the source's voxel", lambda: raw(half.h, ok, S.h, 0)), ("has not the bits of the source's voxel", lambda: raw(half.h, ok, S.h, 1)),
             ("merge 0: dst_map 4 is outside 0 .. 3", lambda: raw(D.h, [(4, 1, 1, 0)], S.h, 1)), ("merge 0: dst_map -1", lambda: raw(D.h, [(-1, 1, 1, 0)], S.h, 1)),
             ("merge 1: src_map 8 is outside 0 .. 7", lambda: raw(D.h, ok + [(1, 8, 1, 0)], S.h, 1)), ("merge 0: src_map -1", lambda: raw(D.h, [(0, -1, 1, 0)], S.h, 1)),
             ("merge 2: destination map 0 appears twice", lambda: raw(D.h, [(0, 1, 1, 0), (1, 1, 1, 0), (0, 2, 1, 0)], S.h, 1)),
             ("merge 0: all_rows 2 is neither 0 nor 1", lambda: raw(D.h, [(0, 1, 2, 0)], S.h, 1)), ("merge 0: min_views 65", lambda: raw(D.h, [(0, 1, 0, 65)], S.h, 1)),
             ("merge 1: map 5 is both a source and a destination", lambda: raw(S.h, [(5, 1, 1, 0), (2, 5, 1, 0)], S.h, 0)),
             ("merge 0: map 1 is both a source and a destination", lambda: raw(S.h, [(1, 1, 1, 0)], S.h, 0))]
    for entry[0] in ((L.cvo_check_maps_merge, ()), (L.cvo_maps_merge, (None,))):
        for match, call in cases:
            with pytest.raises(hiplib.CvoError, match=match):
                call()
    for match, kw in [("level 5", dict(level=5)), ("level 1.5", dict(level=1.5)), ("2 destination maps but 1 source maps", dict(dst_maps=[0, 1])),
                      ("source map 8", dict(src_maps=[8])), ("map 0 appears twice", dict(dst_maps=[0, 0], src_maps=[1, 2])), ("min_views 65", dict(min_views=65)),
                      ("one per merge", dict(all_rows=[True, False]))]:
        args = dict(dict(dst_maps=[0], src=S, src_maps=[1], level=1), **kw)
        for call in (D.merge, D.check_merge):
            with pytest.raises(ValueError, match=match):
                call(**args)
    with pytest.raises(ValueError, match="both a source and a destination"):
        S.merge([0, 1], S, [1, 2])
    with pytest.raises(ValueError, match="level 7"):
        S.coarser(7)
    assert unchanged(D, before) and unchanged(S, src_before)
    D.close(); half.close()


# ---- 9. alignment
def test_a_coarse_map_extracted_and_aligned_is_the_reading_s_rows(hiplib, torch):
    from cvo_slam_amd import synth
    frames, cam_poses = synth.make_sequence(0, 5)
    clouds = []
    for bgr, dep in frames:
        c = synth.dense_cloud(bgr, dep, synth.TUM1)
        pick = np.unique(np.linspace(0, c.n - 1, 5000).astype(np.int64))
        clouds.append((np.ascontiguousarray(c.xyz[pick]), np.ascontiguousarray(c.feat[:, pick].T)))
    poses = [(np.linalg.inv(cam_poses[3]) @ cam_poses[k]).astype(np.float32) for k in range(4)]
    Rd = hiplib.CvoReducer(2, 20000)
    M = hiplib.CvoMaps(Rd, 1, 20000, 0.02)
    R = mr.Map(20000, 0.02)
    tens = dev(torch, clouds[:4])
    for t in range(4):
        M.integrate([0], [[tens[t]]], [[poses[t]]], [[t]]); R.update([clouds[t]], [poses[t]], [t])
    coarse = M.coarser(1)
    got = coarse.extract([0], min_views=2, want=MAP_WANT)[0]
    want = gr.coarser(R, 1).extract(min_views=2)
    assert 100 < want["n_out"] < R.extract(min_views=2)["n_out"]
    same(got, want, "coarse extract", mr.OUTPUTS)
    moving = Rd.reduce([dev(torch, clouds[4:])[0]], 0.04, "mean", 1, want=())[0]
    B = hiplib.CvoBatch(1)
    B.set_pairs_clouds([(got["xyz"], got["feat"], "points_first"), (moving["xyz"], moving["feat"], "points_first")], [0], [1])
    B.align_async(1)
    res = B.wait(1)[0]
    Bh = hiplib.CvoBatch(1)
    Bh.set_pairs([(np.ascontiguousarray(want["xyz"]), np.ascontiguousarray(want["feat"].T), host(moving["xyz"]), np.ascontiguousarray(host(moving["feat"]).T))])
    ref = Bh.align(1)[0]
    assert res["status"] == 0 and ref["status"] == 0
    assert res["transform"].tobytes() == ref["transform"].tobytes() and res["ell"] == ref["ell"] and res["iter"] == ref["iter"]
    coarse.close(); M.close(); Rd.close()
