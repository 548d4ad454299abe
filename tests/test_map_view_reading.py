"""tests/map_view_reading.py holds the definition of a view of a resident map (cvo_hip.h, "Viewing maps"); this file holds the reading to what it
must agree with -- the view of a fusion's MEAN rows, carve_mask -- and to the scene conditions without which the GPU comparisons of
tests/test_gpu_map_views.py would be about nothing.  No GPU."""
import numpy as np
import pytest

import fuse_reading as fr
import map_reading as mr
import map_view_reading as mv
import view_reading as vw

EYE = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def small():
    return mv.scene("small")


@pytest.fixture(scope="module")
def aged(small):
    return mv.history(small["windows"])[1]


@pytest.mark.parametrize("min_views", [1, 2])
@pytest.mark.parametrize("mode,slack,cell", [(vw.FRONT, 0.0, 1), (vw.SURFACE, 0.05, 3)])
def test_a_one_call_map_is_the_view_of_fuse_s_mean_rows(small, min_views, mode, slack, cell):
    members, poses = small["windows"][0][:4], small["windows"][1][:4]
    M = mr.Map(20000, mv.VOXEL); M.update(members, poses, [0, 1, 2, 3])
    F = fr.fuse_reading(members, poses, mv.VOXEL, fr.MEAN, 1, min_views)
    p = vw.params(*small["size"], cell=cell, mode=mode, slack=slack)
    pose = small["poses"][0]
    got = mv.map_view_reading(M, mv.filter_of(1, min_views), pose, small["camera"], p)
    want = vw.view_reading((F["xyz"], F["feat"]), pose, small["camera"], p)
    assert got["n_out"] == want["n_out"] > 100
    for key in ("xyz", "feat", "pixel", "depth"):
        assert got[key].tobytes() == want[key].tobytes(), key
    row = got["E"]["row"]                                               # the fusion's rows are the kept map rows, in order
    assert got["source"].tolist() == row[want["source"]].tolist()
    assert (got["map"][row] == want["map"]).all() and (np.delete(got["map"], row) == mv.FILTERED).all()
    if min_views == 1:
        assert row.tolist() == list(range(M.rows)) and got["index"].tobytes() == want["index"].tobytes()


def test_dead_and_filtered_rows_are_minus_four_and_never_the_front(small, aged):
    M = aged
    dead = np.flatnonzero(np.asarray(M.count) == 0)
    assert dead.size > 10 and dead.max() < M.rows - 1 and dead.min() > 0 < (np.asarray(M.count)[dead.min() - 1])   # dead rows between live ones
    p = vw.params(*small["size"], cell=2)
    for k, flt in enumerate(mv.FILTERS):
        got = mv.map_view_reading(M, flt, small["poses"][1], small["camera"], p)
        kept = np.zeros(M.rows, bool); kept[got["E"]["row"]] = True
        assert (got["map"][~kept] == mv.FILTERED).all() and (got["map"][kept] != mv.FILTERED).all() and not kept[dead].any()
        fronts = got["index"][got["index"] >= 0]
        assert kept[fronts].all() and kept[got["source"]].all() and fronts.size > 50, k
        assert (got["map"][got["source"]] == np.arange(got["n_out"])).all()
        if k in mv.CLAUSE_OF:                                           # the clause alone takes fronts away
            assert 0 < (~kept).sum() and mv.fronts_lost_to(M, flt, mv.CLAUSE_OF[k], small["poses"][1], small["camera"], p) > 0, k


def test_carve_is_carve_mask_of_the_extract_and_its_view(small, aged):
    from cvo_slam_amd.voxels import carve_mask
    M = aged
    flt = mv.filter_of(1, 1, 0)
    E = M.extract(**flt)
    pose = small["poses"][2]
    obs = vw.shifted_rendering((E["xyz"], E["feat"]), pose, small["camera"], small["size"])
    for mode, cell in ((vw.FRONT, 1), (vw.SURFACE, 2)):
        p = vw.params(*small["size"], cell=cell, mode=mode, slack=0.05)
        got = mv.map_view_reading(M, flt, pose, small["camera"], p, obs)
        V = got["V"]
        assert got["carve"].tobytes() == carve_mask(M.rows, E["row"], V["source"], V["relation"]).tobytes()
        assert got["carve"].sum() == got["relation_counts"][1] > 0 and (got["relation_counts"] > 0).all()


def test_the_scenes_of_the_gpu_tests_have_what_they_are_there_for(small, aged):
    """a hidden share and points out of view in the lattice maps and the map with a history; filtered rows; and past the cap"""
    cam, size = small["camera"], small["size"]
    p = vw.params(*size, **vw.SHARES_AT)
    M = mr.Map(20000, mv.VOXEL); M.update([small["lattice"][3000]], [EYE], [0])
    assert M.rows == 3000                                               # a row per point
    for Mk, flt in ((M, mv.filter_of(1, 1, 0)), (aged, mv.FILTERS[4])):
        m = mv.map_view_reading(Mk, flt, small["poses"][0], cam, p)["map"]
        hidden, outside, visible = (m == -1).sum(), (m == -2).sum(), (m >= 0).sum()
        assert hidden > 0.1 * (hidden + visible) and outside > 0.05 * m.shape[0] and visible > 100
    assert (mv.map_view_reading(aged, mv.FILTERS[4], small["poses"][0], cam, p)["map"] == mv.FILTERED).sum() > 100


def test_past_the_cap_the_view_has_rows_where_an_extract_has_none():
    members, poses = mv.past_the_cap()
    M = mr.Map(mv.PAST_MAX_ROWS, mv.PAST_VOXEL); M.update(members, poses, [0, 1, 2])
    E = M.extract(1, 1, 0)
    assert E["n_out"] > 65535 and -(-(-(-M.rows // 256)) // 256) == 2     # the block counts are scanned at two blocks per thread
    for cell in (1, 2):
        for mode in (vw.FRONT, vw.SURFACE):
            got = mv.map_view_reading(M, mv.filter_of(1, 1, 0), mv.PAST_POSE, mv.PAST_CAMERA, vw.params(*mv.PAST_SIZE, cell=cell, mode=mode, slack=0.05), E=E)
            assert 10000 < got["n_out"] <= 65535 and got["source"].max() > 65536, (cell, mode, got["n_out"])
