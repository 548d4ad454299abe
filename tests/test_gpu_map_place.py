"""One resident map through every reader on both of its sides: after an integration, after a compaction (the rows move to the other side) and
after a restore of an earlier snapshot into the same map (they move back, with another row count), extract, view, probe and snapshot are each held
to the reading of the same map_reading.Map, byte for byte.  A reader that was handed the wrong side of the rows, or a stale row count, fails here."""
import numpy as np
import pytest

import fuse_reading as fr
import map_probe_reading as mp
import map_reading as mr
import map_snapshot_reading as sr
import map_view_reading as mv
import view_reading as vw
from test_gpu_map_probes import KEYS as PROBE_KEYS, WANT as PROBE_WANT, same as same_probe
from test_gpu_map_snapshots import dev, is_reading
from test_gpu_map_views import KEYS as VIEW_KEYS, SHEET_CAM, WANT as VIEW_WANT, same as same_view
from test_gpu_maps import WANT as MAP_WANT, same as same_extract

pytestmark = pytest.mark.gpu

EYE = np.eye(4, dtype=np.float32)
MAX_ROWS, VOXEL = 320, 0.12                                            # two 256-row blocks, the second partial; a table of 640 slots
FILTER = mv.filter_of(2, 3, 1)                                         # three values of their own: a reader that swaps two fields reads other rows
SIZE = (64, 48)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def scene():
    """six windows of a 1500-point sheet (map_reading.sliding_windows), and the probe's member: the first 500 points of the last window, which
    no map takes in, in the maps' frame, the last 50 of them 5 m behind the sheet (absent at either reach)"""
    members, poses = mr.sliding_windows(np.random.default_rng(7), members=6, n=1500)
    world = fr.moved_concat([members[5]], [poses[5]])
    probe = (np.ascontiguousarray(world[0][:500]), np.ascontiguousarray(world[1][:500]))
    probe[0][450:, 2] += np.float32(5.0)
    assert probe[0].shape == (500, 3) and np.isfinite(probe[0]).all()
    return members, poses, probe


def readings_of(R, probe):
    """the four readings of map R, with the moment's conditions: the filter drops a row and keeps a row; both probes find, miss and meet a
    filtered row"""
    E = R.extract(**FILTER)
    assert 0 < E["n_out"] < R.rows
    V = mv.map_view_reading(R, FILTER, EYE, SHEET_CAM, vw.params(*SIZE, 1, vw.FRONT, 0.0), E=E)
    assert 0 < V["n_out"] <= E["n_out"]
    P = [mp.probe_reading(R, FILTER, probe, EYE, reach) for reach in (0, 1)]
    for p in P:
        assert (p["counts"][:3] >= 1).all() and p["counts"].sum() == 500, p["counts"]
    return E, V, P


def every_reader(torch, M, R, probe, what):
    E, V, P = readings_of(R, probe)                                    # (numpy alone: before any call)
    same_extract(M.extract([0], want=MAP_WANT, **FILTER)[0], E, what, mr.OUTPUTS)
    same_view(M.view([0], [EYE], SHEET_CAM, SIZE, 1, "front", 0.0, want=VIEW_WANT, **FILTER)[0], V, what, VIEW_KEYS)
    cloud = dev(torch, [probe])
    for reach in (0, 1):
        same_probe(M.probe([0], cloud, [EYE], reach=reach, want=PROBE_WANT, hit=True, **FILTER)[0], P[reach], (what, reach), PROBE_KEYS)
    is_reading(M, 0, R, what)


def test_one_map_through_every_reader_on_both_sides(hiplib, torch):
    members, poses, probe = scene()
    tens = dev(torch, members)
    reducer = hiplib.CvoReducer(4, 4096)
    M = hiplib.CvoMaps(reducer, 1, MAX_ROWS, VOXEL)
    R = mr.Map(MAX_ROWS, VOXEL)
    # the earlier state, kept for the third moment
    M.integrate([0], [tens[:3]], [poses[:3]], [[0, 1, 2]]); R.update(members[:3], poses[:3], [0, 1, 2])
    early_rows = R.rows
    early = sr.snapshot(R)
    kept = M.snapshot([0])[0]
    assert sr.same_snapshot(kept, early) and 256 < early_rows < MAX_ROWS
    # 1. integrate: about 300 rows, the table more than 40 % full, some rows dead
    for t in (3, 4):
        M.integrate([0], [[tens[t]]], [[poses[t]]], [[t]]); R.update([members[t]], [poses[t]], [t])
    M.remove([0], [[tens[0]]], [[poses[0]]], [[0]]); R.update([members[0]], [poses[0]], [0], -1)
    assert 290 <= R.rows <= MAX_ROWS and R.rows > 0.4 * 2 * MAX_ROWS and 0 < R.live < R.rows
    every_reader(torch, M, R, probe, "integrated")
    # 2. compact: every third row dropped, and the dead ones; the rows are on the other side now
    before = R.rows
    drop = (np.arange(before) % 3 == 0).astype(np.uint8)
    rows_out = M.compact([0], drop=[torch.from_numpy(drop).cuda()])
    R.compact(drop=drop)
    assert np.asarray(rows_out).tolist() == [R.rows] and 0.5 * before < R.rows <= 0.7 * before and R.live == R.rows
    every_reader(torch, M, R, probe, "compacted")
    # 3. restore the earlier snapshot into the same map: back on the first side, with another row count
    M.restore([0], [kept])
    R = sr.restore(early, MAX_ROWS, VOXEL)
    assert R.rows == early_rows
    every_reader(torch, M, R, probe, "restored")
    M.close(); reducer.close()
