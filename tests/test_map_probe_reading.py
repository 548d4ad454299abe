"""The reading of a map probe (tests/map_probe_reading.py) against what the definition implies, and the conditions on the shared scene that keep
every class of outcome populated.  No GPU."""
import numpy as np
import pytest

import map_probe_reading as mp
import map_reading as mr
import map_view_reading as mv

LOOSEST = mv.FILTERS[0]
TWO_VIEWS = mv.filter_of(1, 2, -2 ** 31)
EYE = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def scene():
    S = mv.scene("small")
    steps, M = mv.history(S["windows"])
    members, poses = S["windows"]
    return dict(M=M, members=members, poses=poses, steps=steps)


def d2_to_rows(moved, means):
    """(points, rows) f32: the definition's d2 of every point to every row mean"""
    d = moved[:, None, :] - means[None, :, :]
    return ((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]).astype(np.float32)


def cells_of_keys(key):
    k = np.asarray(key, np.int64)
    return np.stack([(k >> 42) & 0x1FFFFF, (k >> 21) & 0x1FFFFF, k & 0x1FFFFF], axis=1) - (1 << 20)


def test_a_member_the_map_holds_is_found_whole(scene):
    M = scene["M"]
    for m in (0, 2, 3, 4):                                             # the members the history left in the map
        got = mp.probe_reading(M, LOOSEST, scene["members"][m], scene["poses"][m], 0)
        assert got["valid"].all() and (got["row"] >= 0).all() and got["counts"].tolist() == [got["row"].shape[0], 0, 0, 0]
        own = np.asarray([M.index[int(k)] for k in ((got["cell"][:, 0] + (1 << 20)) << 42 | (got["cell"][:, 1] + (1 << 20)) << 21 | (got["cell"][:, 2] + (1 << 20))).tolist()])
        assert np.array_equal(got["row"], own)
        assert (got["dist2"] < 3 * mv.VOXEL ** 2).all() and (got["count"] >= 1).all() and (got["views"] >= 1).all()


@pytest.mark.parametrize("flt", [LOOSEST, TWO_VIEWS, mv.FILTERS[4]])
def test_reach_1_is_the_brute_force_nearest_where_that_lies_in_the_27_cells(scene, flt):
    M = scene["M"]
    E = M.extract(**flt)
    rows_cell = cells_of_keys(E["key"])
    got = mp.probe_reading(M, flt, scene["members"][5], scene["poses"][5], 1)
    ok = got["valid"]
    d2 = d2_to_rows(got["moved"][ok], E["xyz"])
    rank = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | E["row"].astype(np.uint64)[None, :]
    near = rank.argmin(axis=1)                                         # the nearest kept row of the whole map, ties to the lowest row
    inside = (np.abs(rows_cell[near] - got["cell"][ok]) <= 1).all(axis=1)
    assert inside.sum() >= 500
    assert np.array_equal(got["row"][ok][inside], E["row"][near[inside]])
    assert got["dist2"][ok][inside].tobytes() == d2[np.arange(near.shape[0]), near][inside].tobytes()
    # and where it lies outside, the winner is the nearest among the rows of the 27 cells, or there is none
    in27 = (np.abs(rows_cell[None, :, :] - got["cell"][ok][:, None, :]) <= 1).all(axis=2)
    masked = np.where(in27, rank, np.iinfo(np.uint64).max)
    pick = masked.argmin(axis=1)
    has = in27.any(axis=1)
    assert np.array_equal(got["row"][ok][has], E["row"][pick[has]]) and (got["row"][ok][~has] < 0).all()


@pytest.mark.parametrize("reach", [0, 1])
@pytest.mark.parametrize("flt", list(mv.FILTERS) + [TWO_VIEWS])
def test_hit_counts_and_the_row_less_outputs(scene, reach, flt):
    M = scene["M"]
    for m in (1, 5):
        got = mp.probe_reading(M, flt, scene["members"][m], scene["poses"][m], reach)
        n = scene["members"][m][0].shape[0]
        assert got["counts"].sum() == n and got["row"].shape == (n,)
        want = np.zeros(M.rows, np.uint8); want[np.unique(got["row"][got["row"] >= 0])] = 1
        assert np.array_equal(got["hit"], want) and got["hit"].shape == (M.rows,)
        none = got["row"] < 0
        assert (got["dist2"][none].view(np.uint32) == mp.INF_BITS).all() and np.isfinite(got["dist2"][~none]).all()
        assert not got["count"][none].any() and not got["views"][none].any() and not got["last_stamp"][none].any()
        kept = set(M.extract(**flt)["row"].tolist())
        assert set(got["row"][~none].tolist()) <= kept


def test_invalid_points_and_an_empty_member(scene):
    M = scene["M"]
    x, f = (a.copy() for a in scene["members"][5])
    x[3, 1] = np.nan; x[10, 0] = np.inf; x[11, 2] = 40000.0; f[20, 4] = 32768.0; f[21, 0] = -np.inf
    far = EYE.copy(); far[0, 3] = 32767.0                              # moves every x' past 2^15
    for reach in (0, 1):
        got = mp.probe_reading(M, LOOSEST, (x, f), scene["poses"][5], reach)
        assert (got["row"][[3, 10, 11, 20, 21]] == mp.INVALID).all() and got["counts"][3] == 5
        gone = mp.probe_reading(M, LOOSEST, scene["members"][5], far @ scene["poses"][5], reach)
        assert gone["counts"][3] + gone["counts"][1] == gone["row"].shape[0] and gone["counts"][3] > 0
        none = mp.probe_reading(M, LOOSEST, (np.zeros((0, 3), np.float32), np.zeros((0, 5), np.float32)), EYE, reach)
        assert none["counts"].tolist() == [0, 0, 0, 0] and none["row"].shape == (0,) and not none["hit"].any()
        empty = mp.probe_reading(mr.Map(10, mv.VOXEL), LOOSEST, scene["members"][5], scene["poses"][5], reach)
        assert empty["counts"][1] == empty["row"].shape[0] and empty["hit"].shape == (0,)


def test_scene_conditions(scene):
    """every class of outcome has its points on the shared scene: a later change of the scene cannot empty one"""
    M = scene["M"]
    assert M.rows > M.live > 1000
    five = scene["members"][5], scene["poses"][5]
    r0 = mp.probe_reading(M, LOOSEST, *five, 0); r1 = mp.probe_reading(M, LOOSEST, *five, 1)
    assert r0["counts"][0] >= 100 and r0["counts"][1] >= 100
    own = r0["row"]                                                    # at the loosest filter: the own cell's row where it has a live one
    other = (r1["row"] >= 0) & (r1["row"] != own)
    assert (other & (own >= 0)).sum() >= 100                          # winners in another cell than the point's own, though that has a row
    assert ((r1["row"] >= 0) & (own < 0)).sum() >= 50                 # found at reach 1, missed at reach 0
    one = mp.probe_reading(M, LOOSEST, scene["members"][1], scene["poses"][1], 0)
    assert one["counts"][2] >= 100                                     # the removed member's dead rows
    for reach in (0, 1):
        two = mp.probe_reading(M, TWO_VIEWS, *five, reach)
        assert (two["counts"][:3] >= 100).all(), (reach, two["counts"])


def tie_maps():
    """voxel 0.5; two lone rows with means 0.75 and 1.25 along x, integrated in either order; a point at x = 1.0 has d2 = 0.0625 to both"""
    f = np.full((1, 5), 7.0, np.float32)
    a = (np.array([[0.75, 0.25, 0.25]], np.float32), f); b = (np.array([[1.25, 0.25, 0.25]], np.float32), f)
    maps = []
    for first, second in ((a, b), (b, a)):
        M = mr.Map(8, 0.5)
        M.update([first], [EYE], [0]); M.update([second], [EYE], [1])
        maps.append(M)
    return maps, (np.array([[1.0, 0.25, 0.25]], np.float32), f)


def test_the_exact_tie_goes_to_the_lower_row():
    (ab, ba), point = tie_maps()
    for M, x_of_row_0 in ((ab, 0.75), (ba, 1.25)):
        E = M.extract(**LOOSEST)
        assert E["xyz"][0, 0] == np.float32(x_of_row_0) and M.rows == 2
        got = mp.probe_reading(M, LOOSEST, point, EYE, 1)
        assert got["row"].tolist() == [0] and got["dist2"].tolist() == [0.0625]
        own = mp.probe_reading(M, LOOSEST, point, EYE, 0)
        assert E["xyz"][own["row"][0], 0] == np.float32(1.25) and own["dist2"].tolist() == [0.0625]   # reach 0: the own cell, [1.0, 1.5)


def test_the_rim_of_the_grid():
    """voxel 2^-5: cells 2^20 - 1 and -(2^20 - 1) hold rows; their outer neighbours do not exist and are skipped"""
    voxel = 2.0 ** -5
    hi = np.float32((2 ** 20 - 1) * voxel + voxel / 2); lo = np.float32(-(2 ** 20 - 1) * voxel + voxel / 2)
    f = np.zeros((2, 5), np.float32)
    pts = (np.array([[hi, hi, hi], [lo, lo, lo]], np.float32), f)
    M = mr.Map(8, voxel)
    M.update([pts], [EYE], [0])
    assert M.rows == 2
    for reach in (0, 1):
        got = mp.probe_reading(M, LOOSEST, pts, EYE, reach)
        assert got["row"].tolist() == [0, 1] and got["dist2"].tolist() == [0.0, 0.0] and (np.abs(got["cell"]) == 2 ** 20 - 1).all()
    inner = (pts[0] - np.float32(voxel) * np.sign(pts[0])).astype(np.float32)    # one cell inward: found at reach 1 only
    assert mp.probe_reading(M, LOOSEST, (inner, f), EYE, 0)["row"].tolist() == [-1, -1]
    assert mp.probe_reading(M, LOOSEST, (inner, f), EYE, 1)["row"].tolist() == [0, 1]
