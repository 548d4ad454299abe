"""The voxel-grid kernels' shared table and lane runs (cvo_voxel_table.hpp) on the engineered clouds of tests/table_cases.py: chains as long as
the cloud, inserts that step from the table's last slot to slot 0, finds deep in a chain, lookups of absent keys that walk a whole chain,
compactions that take rows out of a chain's middle, and prescribed lane runs.  The numpy mirror of the hash that places those clouds is held to
the device's own function first (cvo_selftest_voxel_slots); then every case goes through reduce, count, fuse and the resident maps and is
compared with the readings byte for byte (tests/voxel_reading.py, tests/fuse_reading.py, tests/map_reading.py)."""
import numpy as np
import pytest

import fuse_reading as fr
import map_reading as mr
import table_cases as tc
import voxel_reading as vr

pytestmark = pytest.mark.gpu

REDUCED = ("xyz", "feat", "count", "source", "map")
FUSED = REDUCED + ("views", "view_mask")
MAP_WANT = ("count", "views", "view_mask", "last_stamp", "born", "row")
SLOTS = (2, 6, 128, 130, 514, 2097150)
MAX_POINTS = 400


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def reducer(hiplib):
    R = hiplib.CvoReducer(32, MAX_POINTS)
    yield R
    R.close()


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev(torch, members):
    return [(up(torch, x), up(torch, f), "points_first") for x, f in members]


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else t


def same(got, want, what, keys):
    assert got["n_out"] == want["n_out"], (what, got["n_out"], want["n_out"])
    for key in keys:
        g, w = host(got[key]), host(want[key])
        if key == "view_mask":
            g, w = g.view(np.uint64), w.view(np.uint64)                # (torch carries the 64 bits as int64)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, key)


# ---- 1. the mirror against the device
def corner_points(voxel):
    """positions at the last cells either way and one beyond, -0.0, exact multiples of the voxel and their neighbours, NaN, inf, 2^15"""
    v = np.float32(voxel)
    down = lambda a: np.nextafter(np.float32(a), np.float32(-np.inf)); upw = lambda a: np.nextafter(np.float32(a), np.float32(np.inf))
    far = np.float32(1048575.0) * v                                    # cell 2^20 - 1 where it is below 2^15
    vals = [0.0, -0.0, v, -v, down(-v), upw(-v), down(v), 2 * v, -2 * v, 3 * v, 7 * v, -7 * v, far, -far, upw(far), down(-far), np.float32(1048576.0) * v,
            -np.float32(1048576.0) * v, down(np.float32(1048576.0) * v), np.float32(1048575.5) * v, np.nan, np.inf, -np.inf, 32768.0, -32768.0, down(32768.0),
            upw(-32768.0), 40000.0, down(0.0), upw(0.0)]
    vals = np.array(vals, np.float32)
    x = np.full((3 * vals.shape[0] + vals.shape[0], 3), 0.3, np.float32) * v
    for axis in range(3):
        x[axis * vals.shape[0]:(axis + 1) * vals.shape[0], axis] = vals
    x[3 * vals.shape[0]:] = vals[:, None]                               # all three coordinates at once
    return np.ascontiguousarray(x)


def test_the_mirror_is_the_device_s_function(hiplib):
    api = hiplib.api
    rng = np.random.default_rng(61)
    clouds = [(rng.uniform(-4.0, 4.0, (100000, 3)).astype(np.float32), 0.05)]
    clouds += [(corner_points(v), v) for v in (2.0 ** -6, 0.05, 1.0, tc.VOXEL)]
    clouds += [(rng.uniform(-20000.0, 20000.0, (2000, 3)).astype(np.float32), 2.0 ** -6)]       # cells up to the 2^20 bound, many past it
    for x, voxel in clouds:
        ok, key = tc.keys_of(x, voxel)
        for slots in SLOTS:
            valid, dkey, dslot = api.selftest_voxel_slots(x, voxel, slots)
            assert np.array_equal(valid, ok), (voxel, slots)
            assert np.array_equal(dkey[ok], key[ok].astype(np.uint64)) and (dkey[~ok] == 0).all(), (voxel, slots)
            assert np.array_equal(dslot[ok].astype(np.int64), tc.home_slot(key[ok], slots)) and (dslot[~ok] == 0).all(), (voxel, slots)
    ok, key = tc.keys_of(clouds[1][0], 2.0 ** -6)
    assert ok.any() and (~ok).any() and (key[ok] >> 42).max() == 2 ** 21 - 1 and (key[ok] >> 42).min() == 1       # cells 2^20 - 1 and -(2^20 - 1) are there
    ok, _ = tc.keys_of(clouds[-1][0], 2.0 ** -6)
    assert 100 < ok.sum() < 1900


def test_every_engineered_point_reports_the_home_it_was_built_for(hiplib):
    api = hiplib.api
    for case in tc.all_cases():
        ok, key = tc.keys_of(case["xyz"])
        valid, dkey, dslot = api.selftest_voxel_slots(case["xyz"], tc.VOXEL, case["slots"])
        assert np.array_equal(valid, ok) and np.array_equal(dkey[ok], key[ok].astype(np.uint64)), case["name"]
        c = case["cells"] + (1 << 20)
        assert np.array_equal(dkey[ok].astype(np.int64), ((c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2])[ok]), case["name"]
        if case["homes"] is not None:
            assert ok.all() and np.array_equal(dslot.astype(np.int64), case["homes"]), case["name"]


# ---- 2. every case against the readings
def test_reduce_and_count_every_case_in_one_call(hiplib, torch, reducer):
    cases = tc.all_cases()
    assert len(cases) == 16 and len({c["xyz"].shape[0] for c in cases}) == 6          # clouds of different sizes side by side (grid.y)
    clouds = dev(torch, [(c["xyz"], c["feat"]) for c in cases])
    for mode in ("mean", "central"):
        for min_points in (1, 2):
            got = reducer.reduce(clouds, tc.VOXEL, mode, min_points, want=("count", "source", "map"))
            for c, g in zip(cases, got):
                same(g, vr.reduce_reading(c["xyz"], c["feat"], tc.VOXEL, mode, min_points), (c["name"], mode, min_points), REDUCED)
    sizes = [tc.VOXEL, 2 * tc.VOXEL, tc.VOXEL / 2, 64.0]
    for min_points in (1, 2):
        counts = reducer.count_voxels(clouds, sizes, min_points)
        want = np.array([[vr.count_reading(c["xyz"], c["feat"], v, min_points) for v in sizes] for c in cases])
        assert np.array_equal(counts, want), min_points
    for c, row in zip(cases, reducer.count_voxels(clouds, sizes, 1)):
        if c["homes"] is not None:                                     # a chain of as many cells as the case has
            assert row[0] == len({tuple(q) for q in c["cells"].tolist()}), c["name"]


@pytest.mark.parametrize("mode", ["mean", "central"])
def test_fuse_every_case_split_over_members(hiplib, torch, reducer, mode):
    cases = tc.all_cases()
    groups, poses = [], []
    for parts in (2, 3):
        for c in cases:
            members, ps = tc.split(c, parts)
            groups.append(members); poses.append(ps)
    assert len(groups) == 32 and all(sum(x.shape[0] for x, f in g) <= MAX_POINTS for g in groups)
    tens = [dev(torch, g) for g in groups]
    shared = 0
    for min_points, min_views in ((1, 1), (1, 2), (2, 1)):
        got = reducer.fuse(tens, poses, tc.VOXEL, mode, min_points, min_views, want=("count", "source", "map", "views", "view_mask"))
        for k, (g, ps) in enumerate(zip(groups, poses)):
            want = fr.fuse_reading(g, ps, tc.VOXEL, mode, min_points, min_views)
            same(got[k], want, (cases[k % 16]["name"], k // 16 + 2, mode, min_points, min_views), FUSED)
            assert np.array_equal(got[k]["offsets"], want["offsets"])
            shared += int(min_views == 2 and want["n_out"] > 0)
    assert shared >= 8                                                 # cells that collide in the table are shared between members


# ---- 3. the same cases in resident maps
def chain_drop(reading, slots):
    """a drop mask that takes every other row out of the map's chains, in chain order: the rows' keys are inserted one after the other into a
    table of `slots` slots, every chain is walked from its first slot, and rows 1, 3, 5, ... of the walk go"""
    keys = np.asarray(reading.key, np.int64)
    s = tc.simulate(keys, np.ones(keys.shape[0], bool), slots)
    row_at = {int(slot): r for r, slot in enumerate(s["slot"].tolist())}
    occupied = s["table"] >= 0
    starts = [q for q in np.flatnonzero(occupied).tolist() if not occupied[q - 1]]          # (q - 1 == -1: the last slot)
    drop = np.zeros(keys.shape[0], bool)
    longest = 0
    for q in starts:
        chain = tc.chain_order(s["table"], q)
        longest = max(longest, len(chain))
        drop[[row_at[t] for t in chain[1::2]]] = True
    return drop, longest


def history(hiplib, torch, reducer, max_rows, first, second, absent, chain_slots=None):
    """one map's life on engineered clouds, held to the reading at every step; returns the last extract (host arrays).  chain_slots: the table
    size whose chains the drop mask is taken from (the map's own by default)"""
    clouds = {name: (c["xyz"], c["feat"]) for name, c in (("first", first), ("second", second), ("absent", absent)) if c is not None}
    tens = {name: dev(torch, [c])[0] for name, c in clouds.items()}
    EYE = np.eye(4, dtype=np.float32)
    M = hiplib.CvoMaps(reducer, 2, max_rows, tc.VOXEL)
    R = mr.Map(max_rows, tc.VOXEL)

    def check(what, **flt):
        got = M.extract([1], want=MAP_WANT, **flt)[0]
        same(got, R.extract(**flt), (max_rows, what), mr.OUTPUTS)
        rows, live = M.rows([1])
        assert (int(rows[0]), int(live[0])) == (R.rows, R.live), (max_rows, what)
        assert M.rows([0])[0].tolist() == [0]                          # the other map stays empty throughout
        return {k: (host(v).copy() if hasattr(v, "cpu") else v) for k, v in got.items()}

    def update(name, stamp, sign=1):
        (M.integrate if sign > 0 else M.remove)([1], [[tens[name]]], [[EYE]], [[stamp]], **({} if sign > -2 else dict(present=True)))
        R.update([clouds[name]], [EYE], [stamp], sign)

    update("first", 0)
    check("first")
    if second is not None:
        update("second", 1)
        check("second")
    # cells that are not in the map but whose probes start inside its chain: a lookup walks the chain to an empty slot
    before = check("before the refusals", min_points=0, min_views=0, min_last_stamp=-2 ** 31)
    with pytest.raises(hiplib.CvoError, match="absent"):
        M.remove([1], [[tens["absent"]]], [[EYE]], [[0]])
    with pytest.raises(mr.Refused):
        R.update([clouds["absent"]], [EYE], [0], -1)
    after = check("after the refusal", min_points=0, min_views=0, min_last_stamp=-2 ** 31)
    assert all(np.asarray(before[k]).tobytes() == np.asarray(after[k]).tobytes() for k in mr.OUTPUTS)
    update("absent", 0, -2)                                            # "remove what is still there" skips them
    after = check("after the skipped removal", min_points=0, min_views=0, min_last_stamp=-2 ** 31)
    assert all(np.asarray(before[k]).tobytes() == np.asarray(after[k]).tobytes() for k in mr.OUTPUTS)
    # every other row of the chain goes: the rows behind a dropped one must still be found
    drop, longest = chain_drop(R, 2 * max_rows if chain_slots is None else chain_slots)
    assert drop.sum() >= R.rows // 2 - 2
    n_new, new_row = M.compact([1], drop=[up(torch, drop.astype(np.uint8))], new_row=True)
    want_new = R.compact(drop=drop.tolist())
    assert n_new.tolist() == [R.rows] and host(new_row[0]).tobytes() == want_new.tobytes()
    check("compacted")
    update("first", 2)                                                 # the survivors are found and added to; the dropped cells are born again behind them
    check("first again")
    if second is not None:
        update("second", 1, -2)                                        # survivors of the second cloud go; its dropped cells are skipped
        check("second removed")
    update("first", 0, -2)                                             # the survivors lose their first visit; the cells born again have no such bit
    check("first's first visit removed")
    n_new, new_row = M.compact([1], new_row=True)                      # the dead rows alone
    want_new = R.compact()
    assert n_new.tolist() == [R.rows] and host(new_row[0]).tobytes() == want_new.tobytes()
    last = check("at the end")
    assert last["n_out"] == R.rows > 0
    M.close()
    return last, longest


def test_maps_on_a_half_full_table_and_on_other_table_sizes(hiplib, torch, reducer):
    n = 257
    # a. max_rows exactly the cell count: the table is exactly half full, one chain from its last slot through slot 0
    full = tc.last_slot(n)
    absent = tc.last_slot(16, slots=2 * n, avoid=full["cells"])
    a, longest = history(hiplib, torch, reducer, n, full, None, absent)
    assert longest == n
    # b. a larger map: a chain from its last slot, then a second cloud whose cells home at the start of that chain, and absent cells that do too
    big = 600
    first = tc.last_slot(n, slots=2 * big)
    second = tc.last_slot(64, slots=2 * big, avoid=first["cells"])
    gone = tc.last_slot(16, slots=2 * big, avoid=np.concatenate([first["cells"], second["cells"]]))
    b, longest = history(hiplib, torch, reducer, big, first, second, gone)
    assert longest == n + 64
    # c. the same clouds in maps of other sizes: another table, the same bytes
    for case_args, chain_slots, want, sizes in (((full, None, absent), 2 * n, a, (big, 300)), ((first, second, gone), 2 * big, b, (1000, n + 64 + 1))):
        for max_rows in sizes:
            got, _ = history(hiplib, torch, reducer, max_rows, *case_args, chain_slots=chain_slots)     # (the same rows dropped as in the first map)
            assert got["n_out"] == want["n_out"] and all(np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes() for k in mr.OUTPUTS), max_rows
