"""The voxel-grid passes past 65 536 points and rows: reduce, count, fuse, frames read in place, views and resident maps at the sizes at which
an index passes 2^16 and the block-count scan (offsets_pass of cvo_voxel_table.hpp) gives a thread more than one block -- per = ceil(nb / 256)
from 1 (65 536 points, the last thread owns the last block) through 2 (65 537: thread 128 owns one block, the threads behind it none), 3 and 5
(a 640 x 480 frame) to 16 (1 048 575 points, every thread full).  Every comparison is byte for byte against the readings the smaller tests use
(tests/voxel_reading.py, fuse_reading.py, frame_reading.py, view_reading.py, map_reading.py).

Each test first asserts from the reading that its shape is the one it is there for: nb, per, and -- where every cell counts (min_points 1,
min_views 1, the fine voxel) -- that every 256-point block holds at least one head and that the blocks' counts are not all equal.  (With
min_points 2 or min_views 2 heads are few and a block may have none; there the counts must still differ.)

Random clouds are uniform(-4, 4) positions and uniform(0, 255) features with a fixed seed.  The large reducers are created inside their tests
and closed there: CvoReducer(2, 1048575) is 805 MB of scratch."""
import ctypes as C

import numpy as np
import pytest

import frame_reading as frd
import fuse_reading as fr
import map_reading as mr
import view_reading as vw
import voxel_reading as vr

pytestmark = pytest.mark.gpu

CAP = 65535
FINE, COARSE = 0.05, 0.25                                             # many cells: rows past CAP at the larger sizes; 32^3 cells: every row compared
REDUCED = ("xyz", "feat", "count", "source", "map")
FUSED = REDUCED + ("views", "view_mask")
MAP_WANT = ("count", "views", "view_mask", "last_stamp", "born", "row")
CAMERA_VGA = (5000.0, 525.0, 525.0, 319.5, 239.5)
EYE = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


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


def random_cloud(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-4.0, 4.0, (n, 3)).astype(np.float32), rng.uniform(0.0, 255.0, (n, 5)).astype(np.float32)


def block_heads(map_):
    """the heads of every 256-point block, from a reading's map: a head is the lowest point of a row"""
    m = np.asarray(map_); n = m.shape[0]
    idx = np.flatnonzero(m >= 0)
    _, first = np.unique(m[idx], return_index=True)
    return np.bincount(idx[first] // 256, minlength=-(-n // 256))


def shape_is(counts, nb, per, every_block=True):
    """the blocks' counts are a shape that drives offsets_pass as stated"""
    assert counts.shape[0] == nb and -(-nb // 256) == per, (counts.shape[0], nb, per)
    assert len(np.unique(counts)) > 1
    if every_block:
        assert (counts > 0).all()


# ---- reduce and count
SIZES = {"edge": (65536, 65537), "large": (131073, 1048575)}
SHAPES = {65536: (256, 1), 65537: (257, 2), 131073: (513, 3), 1048575: (4096, 16)}


@pytest.mark.parametrize("mode", [0, 1], ids=["mean", "central"])
@pytest.mark.parametrize("call", ["edge", "large"])
def test_reduce_past_65536_points(hiplib, torch, call, mode):
    from test_gpu_reduce_clouds import Raw, raw_reduce
    api = hiplib.api
    sizes = SIZES[call]
    clouds = [random_cloud(n, 70 + k) for k, n in enumerate(sizes)]
    assert -(-256 // 1) == 256 and -(-257 // 2) == 129 and -(-4096 // 16) == 256           # owning threads: per 1 all 256 (the last owns block 255), per 2 threads 0 .. 128, per 16 all
    R = hiplib.CvoReducer(2, max(sizes))
    try:
        tens = dev(torch, clouds)
        descs = [api.device_cloud(*t, max_n=api.REDUCE_MAX_POINTS) for t in tens]
        for min_points in (1, 2):
            want = [vr.reduce_reading(x, f, FINE, mode, min_points) for x, f in clouds]
            for n, w in zip(sizes, want):
                shape_is(block_heads(w["map"]), *SHAPES[n], every_block=min_points == 1)
            if call == "large":
                assert want[1]["n_out"] > CAP and (min_points == 2 or want[0]["n_out"] > CAP)                   # rows, and map[], past the cap
                assert all(w["map"].max() == w["n_out"] - 1 for w in want)
            else:
                assert min_points == 2 or all(60000 < w["n_out"] <= CAP for w in want)
            raws = [Raw(torch, CAP, n) for n in sizes]
            torch.cuda.synchronize()
            rc, n_out = raw_reduce(hiplib, R, descs, [r.record(api) for r in raws], FINE, mode, min_points)
            assert rc == 0, api.load_library().cvo_last_error()
            for r, w, n in zip(raws, want, sizes):
                rows = min(CAP, w["n_out"])                              # exactly so many rows are written
                assert n_out[sizes.index(n)] == w["n_out"], (n, min_points)
                for key, dt, width in (("xyz", np.float32, 3), ("feat", np.float32, 5), ("count", np.int32, 1), ("source", np.int32, 1)):
                    got = r.host(key, dt)
                    assert got[:rows * width].tobytes() == w[key][:rows].tobytes(), (n, min_points, key)
                    assert (got[rows * width:].view(np.uint8) == 0xA5).all(), (n, min_points, key, "behind the rows")
                assert r.host("map", np.int32).tobytes() == w["map"].tobytes(), (n, min_points)
                assert r.guards_intact(), (n, min_points)
            del raws
        # the coarser voxel: every row below the cap, every row compared
        got = R.reduce(tens, COARSE, mode, 1, want=("count", "source", "map"))
        for g, (x, f), n in zip(got, clouds, sizes):
            w = vr.reduce_reading(x, f, COARSE, mode, 1)
            assert 20000 < w["n_out"] < CAP and len(np.unique(block_heads(w["map"]))) > 1
            same(g, w, (n, "coarse"), REDUCED)
    finally:
        R.close()


def test_count_voxels_on_1048575_points(hiplib, torch):
    n = 1048575
    x, f = random_cloud(n, 71)                                         # (the large call's second cloud)
    sizes = [0.05, 0.1, 0.25, 1.0]
    R = hiplib.CvoReducer(1, n)
    try:
        t = dev(torch, [(x, f)])
        for min_points in (1, 2):
            want = [vr.count_reading(x, f, v, min_points) for v in sizes]
            assert want[0] > 10 * CAP > want[2] and len(set(want)) == 4 or min_points == 2
            assert R.count_voxels(t, sizes, min_points).tolist() == [want], min_points
    finally:
        R.close()


# ---- fuse
def fuse_groups():
    """one group of three members of 30001, 29999 and 30003 points (354 blocks, no member a multiple of 256), one of 64 members of 1100"""
    rng = np.random.default_rng(72)
    groups, poses = [], []
    for sizes in ((30001, 29999, 30003), (1100,) * 64):
        groups.append([random_cloud(n, int(rng.integers(1 << 30))) for n in sizes])
        poses.append([fr.rigid(rng, 0.1, 0.2) for _ in sizes])
    return groups, poses


@pytest.mark.parametrize("mode", ["mean", "central"])
def test_fuse_past_65536_points(hiplib, torch, mode):
    groups, poses = fuse_groups()
    voxel = 0.2                                                        # 40^3 cells: rows below the cap, cells shared between members
    assert [sum(-(-x.shape[0] // 256) for x, f in g) for g in groups] == [354, 320] and all(x.shape[0] % 256 for g in groups for x, f in g)
    R = hiplib.CvoReducer(2, 98304)
    try:
        tens = [dev(torch, g) for g in groups]
        for min_views in (1, 2):
            got = R.fuse(tens, poses, voxel, mode, 1, min_views, want=("count", "source", "map", "views", "view_mask"))
            for k, (g, ps) in enumerate(zip(groups, poses)):
                want = fr.fuse_reading(g, ps, voxel, mode, 1, min_views)
                # a group's blocks are its members' blocks one after the other: a head's block from its member and its index in it
                heads = np.zeros((354, 320)[k], np.int64)
                idx = np.flatnonzero(want["map"] >= 0)
                _, first = np.unique(want["map"][idx], return_index=True)
                lowest = idx[first]
                member = np.searchsorted(want["offsets"], lowest, side="right") - 1
                first_block = np.concatenate([[0], np.cumsum([-(-x.shape[0] // 256) for x, f in g])])[:-1]
                np.add.at(heads, first_block[member] + (lowest - want["offsets"][member]) // 256, 1)
                shape_is(heads, (354, 320)[k], 2, every_block=min_views == 1)
                assert 20000 < want["n_out"] <= CAP or min_views == 2
                assert min_views == 1 or 1000 < want["n_out"]
                same(got[k], want, (k, mode, min_views), FUSED)
    finally:
        R.close()


# ---- frames
def slab_frame(w, h, seed):
    """a colour image and a depth image: a tilted plane in pieces -- runs of 1 .. 40 pixels, each piece pushed to a depth of its own within
    +- 0.5 m -- with holes: neighbouring pixels of a piece share cells (lane runs), and every block of 256 pixels meets cells no block before it has"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    plane = 9000.0 + 20.0 * xs * (640.0 / max(w, 640)) + 35.0 * ys * (480.0 / max(h, 480))
    lengths = rng.integers(1, 41, w * h)
    piece = np.repeat(np.arange(lengths.shape[0]), lengths)[:w * h]
    push = rng.uniform(-2500.0, 2500.0, lengths.shape[0])[piece].reshape(h, w)
    depth = np.clip(plane + push, 1000, 60000).astype(np.uint16)
    depth[rng.uniform(size=(h, w)) < 0.03] = 0                         # single missing pixels, inside runs
    depth[h // 3:h // 3 + 9, w // 4:w // 4 + 40] = 0                   # a blind tile
    bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return bgr, depth


def up_frame(torch, bgr, dep):
    return (up(torch, bgr), up(torch, dep.view(np.int16)))             # (torch has no uint16 arithmetic; device_image reinterprets int16)


FRAME_SHAPES = [("257x256", 257, 256, 1, 257, 2), ("vga", 640, 480, 1, 1200, 5), ("vga_s2", 640, 480, 2, 300, 2)]
FRAME_VOXEL = 0.1


@pytest.mark.parametrize("name,w,h,step,nb,per", FRAME_SHAPES, ids=[s[0] for s in FRAME_SHAPES])
def test_frames_past_65536_pixels(hiplib, torch, name, w, h, step, nb, per):
    window = [slab_frame(w, h, 73 + k) for k in range(3)]
    poses = [EYE] + [fr.rigid(np.random.default_rng(80 + k), 0.05, 0.1) for k in range(2)]
    dense = [frd.dense_reading(b, d, CAMERA_VGA, step) for b, d in window]
    n = dense[0][0].shape[0]
    assert n == -(-w // step) * -(-h // step) and -(-n // 256) == nb and n > 65536
    R = hiplib.CvoReducer(2, 3 * n)
    try:
        frames = [up_frame(torch, b, d) for b, d in window]
        for mode in ("mean", "central"):
            for min_points in (1, 2):
                want = [vr.reduce_reading(x, f, FRAME_VOXEL, mode, min_points) for x, f in dense[:2]]
                for q in want:
                    shape_is(block_heads(q["map"]), nb, per, every_block=min_points == 1)
                    assert 2000 < q["n_out"] <= CAP
                got = R.reduce_frames(frames[:2], CAMERA_VGA, FRAME_VOXEL, step=step, mode=mode, min_points=min_points, want=("count", "source", "map"))
                for k in range(2):
                    same(got[k], want[k], (name, mode, min_points, k), REDUCED)
        sizes = [0.05, FRAME_VOXEL, 0.25, 1.0]
        for min_points in (1, 2):
            want = np.array([[vr.count_reading(x, f, v, min_points) for v in sizes] for x, f in dense[:2]])
            assert np.array_equal(R.count_frame_voxels(frames[:2], CAMERA_VGA, sizes, step=step, min_points=min_points), want), min_points
            assert want.min() > 0 and (name != "vga" or min_points == 2 or want[0, 0] > CAP)       # (counted past the cap)
        for mode, min_views in (("mean", 1), ("central", 2)):
            want = fr.fuse_reading(dense, poses, FRAME_VOXEL, mode, 1, min_views)
            assert 2000 < want["n_out"] <= CAP and (want["views"] == 3).any() and -(-3 * nb // 256) >= per
            got = R.fuse_frames([frames], [poses], CAMERA_VGA, FRAME_VOXEL, step=step, mode=mode, min_views=min_views,
                                want=("count", "source", "map", "views", "view_mask"))[0]
            same(got, want, (name, mode, min_views, "window"), FUSED)
    finally:
        R.close()


# ---- view
def test_view_of_70000_points(hiplib, torch):
    size, camera = (320, 240), (1000.0, 290.0, 288.0, 158.7, 119.2)
    rng = np.random.default_rng(74)
    n = 70000
    cloud = vw.two_walls(rng, n, camera, size)
    pose = fr.rigid(rng, 0.03, 0.05)
    observed = vw.shifted_rendering(cloud, pose, camera, size)
    R = hiplib.CvoReducer(1, 76800)                                    # the z-cells of a 320 x 240 image at cell 1
    try:
        t = dev(torch, [cloud])
        obs = up(torch, observed.view(np.int16))
        keys = ("xyz", "feat", "source", "pixel", "map", "depth", "index", "relation")
        for cell in (1, 2):
            for mode, slack in (("front", 0.0), ("surface", 0.0), ("surface", 0.05)):
                p = vw.params(size[0], size[1], cell, dict(front=vw.FRONT, surface=vw.SURFACE)[mode], slack)
                want = vw.view_reading(cloud, pose, camera, p, observed)
                visible = np.bincount(np.flatnonzero(want["map"] >= 0) // 256, minlength=274)
                shape_is(visible, 274, 2)
                assert 10000 < want["n_out"] <= CAP and (cell == 2 or want["depth"].size == 76800 > 65536)
                got = R.view(t, [pose], camera, size, cell, mode, slack, observed=[obs], want=keys[2:])[0]
                same(got, want, (cell, mode, slack), keys)
                assert np.array_equal(got["relation_counts"], want["relation_counts"])
    finally:
        R.close()


# ---- maps
def test_maps_past_65536_rows(hiplib, torch):
    from test_gpu_maps import Raw
    api = hiplib.api
    voxel, max_rows = 0.145, 80000                                     # about 168 000 cells in the box: 90 003 points fill some 70 000 of them
    rng = np.random.default_rng(75)
    one = [random_cloud(n, 90 + k) for k, n in enumerate((30001, 29999, 30003))]
    two = [random_cloud(8000, 93)]
    three = (np.array([[0.3, 0.3, 0.3], [1.3, 0.3, 0.3], [2.3, 0.3, 0.3]], np.float32), np.full((3, 5), 7.0, np.float32))      # three cells of their own
    poses_one = [fr.rigid(rng, 0.05, 0.1) for _ in one]; poses_two = [fr.rigid(rng, 0.05, 0.1)]
    red = hiplib.CvoReducer(2, 98304)
    M = hiplib.CvoMaps(red, 2, max_rows, voxel)
    R = [mr.Map(max_rows, voxel), mr.Map(max_rows, voxel)]
    try:
        t_one, t_two, t_three = dev(torch, one), dev(torch, two), dev(torch, [three])

        def check(what, ks=(0, 1), **flt):
            for k, got in zip(ks, M.extract(list(ks), want=MAP_WANT, **flt)):
                same(got, R[k].extract(**flt), (what, k), mr.OUTPUTS)
            rows, live = M.rows(list(ks))
            assert [(int(a), int(b)) for a, b in zip(rows, live)] == [(R[k].rows, R[k].live) for k in ks], what

        def check_past_the_cap(what):
            """map 0's extract when the filter keeps more than the cap: the full count, exactly cap rows, guards intact"""
            full = R[0].extract()
            assert full["n_out"] > CAP
            raw = Raw(torch, CAP); n_out = np.zeros(1, np.int32)
            ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
            torch.cuda.synchronize()
            assert M.L.cvo_maps_extract(M.h, 1, ip(np.asarray([0], np.int32)), (api.MapFilter * 1)(api.MapFilter(1, 1, 0, 0)), (api.MapCloud * 1)(raw.record(api)),
                                        ip(n_out), None) == 0
            torch.cuda.synchronize()
            assert n_out.tolist() == [full["n_out"]] and raw.guards_intact(), what
            for key in mr.OUTPUTS:
                assert raw.host(key, full[key].dtype, CAP).tobytes() == full[key][:CAP].tobytes(), (what, key)

        # the first call alone has more than 65 536 cells: lookup and the births' offsets at per 2, births above row 65 536
        keys, _, _, _ = mr.call_cells(one, poses_one, voxel)
        assert CAP + 1 < keys.shape[0] <= 75000 and -(-(-(-keys.shape[0] // 256)) // 256) == 2        # per = ceil(ceil(cells / 256) / 256)
        M.integrate([0, 1], [t_one, t_three], [poses_one, [EYE]], [[0, 1, 2], [0]])
        R[0].update(one, poses_one, [0, 1, 2]); R[1].update([three], [EYE], [0])
        assert R[0].rows == keys.shape[0] and R[1].rows == 3
        check("first", min_views=2)
        check_past_the_cap("first")
        # a second, overlapping group: old rows found and births appended behind row 65 536
        before = R[0].rows
        M.integrate([0], [t_two], [poses_two], [[3]]); R[0].update(two, poses_two, [3])
        assert before + 2000 < R[0].rows <= max_rows and sum(1 for m in R[0].mask[CAP + 1:before] if m & 8) > 100      # old rows above 65 536 were added to
        check("second", min_views=2)
        assert 1000 < R[0].extract(min_views=2)["n_out"] <= CAP
        check_past_the_cap("second")
        # the first group goes; then every other row, in the same call as the map of three rows, whose table the large map's grid clears
        M.remove([0], [t_one], [poses_one], [[0, 1, 2]]); R[0].update(one, poses_one, [0, 1, 2], -1)
        assert R[0].rows > CAP + 1 and 2000 < R[0].live <= 8000
        check("removed", ks=(0,))
        drops = [np.arange(R[0].rows) % 2 == 1, np.array([True, False, False])]
        n_new, new_row = M.compact([0, 1], drop=[up(torch, d.astype(np.uint8)) for d in drops], new_row=True)
        want_new = [R[k].compact(drop=drops[k].tolist()) for k in (0, 1)]
        assert n_new.tolist() == [R[0].rows, R[1].rows] and R[1].rows == 2 and 1000 < R[0].rows < 4000
        for k in (0, 1):
            assert host(new_row[k]).tobytes() == want_new[k].tobytes(), k
        check("compacted")
        # both maps again: the survivors are found, what was dropped is born again behind them -- in map 0 past row 65 536 once more
        M.integrate([1, 0], [t_three, t_one], [[EYE], poses_one], [[5], [4, 5, 6]])
        R[1].update([three], [EYE], [5]); R[0].update(one, poses_one, [4, 5, 6])
        assert R[1].rows == 3 and R[0].rows > CAP + 1
        check("again", min_views=2)
        check("again, map 1", ks=(1,), min_points=0, min_views=0)
        check_past_the_cap("again")
    finally:
        M.close(); red.close()
