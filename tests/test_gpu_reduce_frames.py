"""Reducing and fusing RGB-D frames in place (cvo_hip.h, "Reducing frames": cvo_frames_to_device_clouds, cvo_reduce_device_frames,
cvo_count_frame_voxels, cvo_fuse_device_frames) against the numpy readings: tests/frame_reading.py gives a frame's dense cloud, and
tests/voxel_reading.py / tests/fuse_reading.py reduce and fuse it.  Every comparison is exact, on bytes.  The shapes are the smallest at which
each edge exists: 64 x 64 (4096 points, exactly 16 blocks), 67 x 65 (odd, a partial last block), 97 x 70 at step 2 (49 x 35), 100 x 70 at step 3
(the last sub-grid column is pixel 99, the last row 69, where dy must be 0), 64 x 64 at step 16 (16 points: less than a wave)."""
import ctypes as C

import numpy as np
import pytest

import frame_reading as frd
import fuse_reading as fur
import pcd_cases as pc
import voxel_reading as vr

pytestmark = pytest.mark.gpu

INVALID = 4
WANT = ("count", "source", "map")
KEYS = ("xyz", "feat", "count", "source", "map")
FUSE_WANT = ("count", "source", "map", "views", "view_mask")
ONE_CELL_CAMERA = (5000.0, 95.3, 96.1, -1.0, -1.0)                    # every X and Y positive: a 64 m voxel holds the whole frame
VOXELS = [0.05, 0.5, 64.0, 1e-5]
MAX_POINTS = 16384


def plane_depth(w, h):
    """a smooth tilted plane: long runs of neighbouring pixels in one cell"""
    ys, xs = np.mgrid[0:h, 0:w]
    return (9000 + 20 * xs + 35 * ys).astype(np.uint16)


#            name        w    h  step  image family, arg   depth
FRAMES = [("64x64",      64,  64, 1,  ("noise", None),  lambda w, h: pc.depth(w, h, "holes")),
          ("67x65",      67,  65, 1,  ("white", None),  lambda w, h: pc.depth(w, h, "blind_tile")),
          ("97x70s2",    97,  70, 2,  ("noise", None),  lambda w, h: pc.depth(w, h, "full")),
          ("100x70s3",  100,  70, 3,  ("smooth", 40),   lambda w, h: pc.depth(w, h, "holes")),
          ("64x64s16",   64,  64, 16, ("checker", 3),   lambda w, h: pc.depth(w, h, "full")),
          ("plane",      67,  65, 1,  ("noise", None),  plane_depth)]
IDS = [f[0] for f in FRAMES]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def reducer(hiplib):
    R = hiplib.CvoReducer(8, MAX_POINTS)
    yield R
    R.close()


@pytest.fixture(scope="module")
def frames():
    """{name: (bgr, depth, step, dense reading (xyz, feat) under pc.CAMERA)}: computed once, never changed"""
    out = {}
    for name, w, h, step, (family, arg), depth in FRAMES:
        bgr, dep = pc.image(w, h, family, arg), depth(w, h)
        out[name] = (bgr, dep, step, frd.dense_reading(bgr, dep, pc.CAMERA, step))
    return out


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def up16(torch, dep):
    return up(torch, dep.view(np.int16))                               # (torch has no uint16 arithmetic; device_image reinterprets int16)


def tight(torch, bgr, dep):
    return (up(torch, bgr), up16(torch, dep))


def four_descriptors(torch, bgr, dep):
    """the same frame four ways: tight BGR; BGRA with both pitches above the rows' bytes; R, G, B bytes with swap_rb; a crop of a larger tensor
    (3 rows down, 5 pixels in).  ([(bgr, depth)], [swap_rb])"""
    h, w = dep.shape
    rng = np.random.default_rng(3)
    bgra = rng.integers(0, 256, (h, w + 3, 4), dtype=np.uint8); bgra[:, :w, :3] = bgr
    wide = rng.integers(0, 65536, (h, w + 5), dtype=np.uint16); wide[:, :w] = dep
    big = rng.integers(0, 256, (h + 7, w + 9, 3), dtype=np.uint8); big[3:3 + h, 5:5 + w] = bgr
    bigd = rng.integers(0, 65536, (h + 7, w + 9), dtype=np.uint16); bigd[3:3 + h, 5:5 + w] = dep
    tb, td = up(torch, bgra), up16(torch, wide)
    cb, cd = up(torch, big), up16(torch, bigd)
    return ([tight(torch, bgr, dep), (tb[:, :w, :3], td[:, :w]), (up(torch, bgr[:, :, ::-1]), up16(torch, dep)), (cb[3:3 + h, 5:5 + w], cd[3:3 + h, 5:5 + w])],
            [False, False, True, False])


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else t


def same(got, want, what="", keys=KEYS):
    assert got["n_out"] == want["n_out"], (what, got["n_out"], want["n_out"])
    for key in keys:
        g = host(got[key]); w = want[key]
        if key == "view_mask":
            g = g.view(np.uint64)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.shape, w.shape)
        np.testing.assert_array_equal(g.view(np.uint8), w.view(np.uint8), err_msg=str((what, key)))


# ---- a. the dense cloud itself, through every descriptor kind
@pytest.mark.parametrize("name", IDS)
def test_dense_frames_is_the_reading(hiplib, torch, reducer, frames, name):
    bgr, dep, step, (xyz, feat) = frames[name]
    descs, swap = four_descriptors(torch, bgr, dep)
    assert [hiplib.api.device_image(*d)[0].pixel_bytes for d in descs] == [3, 4, 3, 3]
    assert hiplib.api.device_image(*descs[1])[0].depth_pitch > 2 * dep.shape[1] and hiplib.api.device_image(*descs[3])[0].bgr_pitch == 3 * (dep.shape[1] + 9)
    got = reducer.dense_frames(descs, pc.CAMERA, step=step, swap_rb=swap)
    assert len(got) == 4
    for k, (x, f) in enumerate(got):
        assert x.shape == xyz.shape and f.shape == feat.shape
        np.testing.assert_array_equal(host(x).view(np.uint32), xyz.view(np.uint32), err_msg=str((name, k)))     # (bits: NaN rows included)
        np.testing.assert_array_equal(host(f).view(np.uint32), feat.view(np.uint32), err_msg=str((name, k)))
    if name == "100x70s3":                                             # the last sub-grid column is pixel 99, the last row is row 69: no dy there
        ws, hs, x, y = frd.sub_grid(100, 70, 3)
        assert x.max() == 99 and y.max() == 69 and (feat[y == 69, 3:] == 0).all() and (feat[y == 66, 4] != 0).any()
    # two cameras in one call
    two = reducer.dense_frames([descs[0], descs[0]], [pc.CAMERA_B, pc.CAMERA], cam_index=[1, 0], step=step)
    xb, fb = frd.dense_reading(bgr, dep, pc.CAMERA_B, step)
    np.testing.assert_array_equal(host(two[0][0]).view(np.uint32), xyz.view(np.uint32))
    np.testing.assert_array_equal(host(two[1][0]).view(np.uint32), xb.view(np.uint32))
    np.testing.assert_array_equal(host(two[1][1]).view(np.uint32), fb.view(np.uint32))


# ---- b. the generator's cloud of a frame is a row subset of its dense cloud
@pytest.mark.parametrize("size,family,arg", [((64, 64), "noise", None), ((67, 65), "smooth", 40), ((100, 70), "white", None)], ids=["64x64", "67x65", "100x70"])
def test_the_generated_cloud_is_rows_of_the_dense_cloud(hiplib, torch, reducer, size, family, arg):
    w, h = size
    bgr, dep = pc.image(w, h, family, arg), pc.depth(w, h, "holes")
    g = hiplib.Cvo()
    g.set_num_want(600)
    g.set_pcd_images(bgr, dep, pc.CAMERA)
    xyz, feat = g.get_cloud(hiplib.api.SLOT_FIXED)
    px = g.get_selected_points(hiplib.api.SLOT_FIXED)
    g.close()
    assert xyz.shape[0] == px.shape[0] >= 8
    dx, df = reducer.dense_frames([tight(torch, bgr, dep)], pc.CAMERA)[0]
    rows = frd.rows_of_pixels(w, h, 1, px)
    np.testing.assert_array_equal(host(dx)[rows].view(np.uint32), xyz.view(np.uint32))
    np.testing.assert_array_equal(host(df)[rows].view(np.uint32), np.ascontiguousarray(feat.T).view(np.uint32))


# ---- c. reduction
@pytest.mark.parametrize("name", IDS)
def test_reduce_frames_is_the_reading_and_the_reduction_of_the_dense_cloud(hiplib, torch, reducer, frames, name):
    bgr, dep, step, (xyz, feat) = frames[name]
    descs, swap = four_descriptors(torch, bgr, dep)
    dense = reducer.dense_frames(descs[:1], pc.CAMERA, step=step)
    clouds = [(dense[0][0], dense[0][1], "points_first")]
    for voxel in VOXELS:
        for mode in ("mean", "central"):
            for min_points in (1, 2):
                want = vr.reduce_reading(xyz, feat, voxel, mode, min_points)
                got = reducer.reduce_frames(descs, pc.CAMERA, voxel, step=step, mode=mode, min_points=min_points, want=WANT, swap_rb=swap)
                for k in range(4):
                    same(got[k], want, (name, voxel, mode, min_points, k))
                same(reducer.reduce(clouds, voxel, mode, min_points, want=WANT)[0], want, (name, voxel, mode, min_points, "dense"))
    valid = int(np.isfinite(xyz[:, 2]).sum())
    assert vr.reduce_reading(xyz, feat, 1e-5, "mean", 1)["n_out"] == valid > 0                       # own cells: as many rows as valid points
    x1, f1 = frd.dense_reading(bgr, dep, ONE_CELL_CAMERA, step)
    want = vr.reduce_reading(x1, f1, 64.0, "mean", 1)
    assert want["n_out"] == 1 and want["count"].tolist() == [valid]                                  # one cell: every lane's atomics on one row
    for mode in ("mean", "central"):
        same(reducer.reduce_frames(descs[:1], ONE_CELL_CAMERA, 64.0, step=step, mode=mode, want=WANT)[0], vr.reduce_reading(x1, f1, 64.0, mode, 1), (name, "one cell", mode))


class Raw:
    """one frame's or group's output arrays as byte tensors prefilled with 0xA5, each with 64 guard bytes behind its extent"""
    G = 64

    def __init__(self, torch, cap, n_in, arrays=("xyz", "feat", "count", "source", "map"), fused=False):
        self.cap = cap; self.fused = fused
        self.sizes = dict(xyz=12 * cap, feat=20 * cap, count=4 * cap, source=4 * cap, map=4 * n_in, views=4 * cap, view_mask=8 * cap)
        self.t = {k: torch.full((self.sizes[k] + self.G,), 0xA5, dtype=torch.uint8, device="cuda") for k in arrays}

    def record(self, api):
        p = lambda k: self.t[k].data_ptr() if k in self.t else None
        if self.fused:
            return api.FusedCloud(p("xyz"), p("feat"), p("count"), p("source"), p("map"), p("views"), p("view_mask"), self.cap, 0)
        return api.ReducedCloud(p("xyz"), p("feat"), p("count"), p("source"), p("map"), self.cap, 0)

    def host(self, key, dtype):
        return self.t[key].cpu().numpy()[:self.sizes[key]].view(dtype)

    def guards_intact(self):
        return all((t.cpu().numpy()[self.sizes[k]:] == 0xA5).all() for k, t in self.t.items())

    def untouched(self):
        return all((t.cpu().numpy() == 0xA5).all() for t in self.t.values())


def lead(api, R, images, w, h, step, cams=(pc.CAMERA,), cam_index=None):
    """the leading arguments of a frame call, and what must stay alive"""
    arr = (api.DeviceImage * max(1, len(images)))(*images)
    cam = (api.Camera * len(cams))(*[api.Camera(*c) for c in cams])
    ci = None if cam_index is None else np.asarray(cam_index, np.int32)
    return [R.h, len(images), arr, w, h, step, cam, None if ci is None else ci.ctypes.data_as(C.POINTER(C.c_int))], (arr, cam, ci)


def raw_reduce(api, R, args, recs, voxel=0.05, mode=0, min_points=1):
    out = (api.ReducedCloud * len(recs))(*recs)
    prm = api.ReduceParams(voxel, mode, min_points, 0)
    n_out = np.full(len(recs), -7, np.int32)
    return R.L.cvo_reduce_device_frames(*args, C.byref(prm), out, n_out.ctypes.data_as(C.POINTER(C.c_int)), None), n_out


@pytest.mark.parametrize("mode", [0, 1])
def test_cap_below_the_row_count_and_count_only(hiplib, torch, reducer, frames, mode):
    api = hiplib.api
    names = ["67x65", "100x70s3"]
    for name, cap in zip(names, (100, 7)):
        bgr, dep, step, (xyz, feat) = frames[name]
        t = tight(torch, bgr, dep)
        d, w, h = api.device_image(*t)
        want = vr.reduce_reading(xyz, feat, 0.05, mode, 1)
        assert want["n_out"] > cap
        raw = Raw(torch, cap, xyz.shape[0])
        torch.cuda.synchronize()
        args, keep = lead(api, reducer, [d], w, h, step)
        rc, n_out = raw_reduce(api, reducer, args, [raw.record(api)], 0.05, mode)
        assert rc == 0, api.load_library().cvo_last_error()
        assert n_out[0] == want["n_out"]                                # the full row count
        for key, dt in (("xyz", np.float32), ("feat", np.float32), ("count", np.int32), ("source", np.int32)):
            np.testing.assert_array_equal(raw.host(key, dt), want[key][:cap].reshape(-1), err_msg=key)
        np.testing.assert_array_equal(raw.host("map", np.int32), want["map"])                        # full row numbers
        assert raw.guards_intact()
        with pytest.raises(hiplib.CvoError, match=f"cap {cap}"):
            reducer.reduce_frames([t], pc.CAMERA, 0.05, step=step, mode=mode, cap=cap)
        rc, n_out = raw_reduce(api, reducer, args, [api.ReducedCloud(None, None, None, None, None, 0, 0)], 0.05, mode)
        assert rc == 0 and n_out.tolist() == [want["n_out"]]           # cap = 0 with every array NULL counts only
        counted = reducer.reduce_frames([t], pc.CAMERA, 0.05, step=step, mode=mode, cap=0, want=())[0]
        assert counted["n_out"] == want["n_out"] and counted["xyz"].shape[0] == 0


def test_frames_without_a_valid_point_write_nothing(hiplib, torch, reducer):
    api = hiplib.api
    bgr = pc.image(64, 64, "noise")
    zeros = np.zeros((64, 64), np.uint16); far = np.full((64, 64), 65535, np.uint16)
    unit = (1.0, 95.3, 96.1, 33.7, 31.2)                                # scaling_factor 1: z = 65535 >= 2^15, an invalid point
    x, f = frd.dense_reading(bgr, far, unit)
    assert (x[:, 2] == 65535.0).all() and vr.reduce_reading(x, f, 0.05)["n_out"] == 0
    for dep, cam in ((zeros, pc.CAMERA), (far, unit)):
        t = tight(torch, bgr, dep)                                      # (kept: the descriptor holds pointers, not tensors)
        d, w, h = api.device_image(*t)
        for mode in (0, 1):
            raw = Raw(torch, 300, 4096, arrays=("xyz", "feat", "count", "source"))
            torch.cuda.synchronize()
            args, keep = lead(api, reducer, [d], w, h, 1, [cam])
            rc, n_out = raw_reduce(api, reducer, args, [raw.record(api)], 0.05, mode)
            torch.cuda.synchronize()
            assert rc == 0 and n_out.tolist() == [0] and raw.untouched()
        got = reducer.reduce_frames([t], cam, 0.05, want=WANT)[0]
        assert got["n_out"] == 0 and (host(got["map"]) == -1).all()
        assert reducer.count_frame_voxels([t], cam, [0.05, 1.0]).tolist() == [[0, 0]]
    dx, df = reducer.dense_frames([tight(torch, bgr, zeros)], pc.CAMERA)[0]
    assert (host(dx).view(np.uint32) == 0x7FC00000).all() and np.array_equal(host(df)[:, :3], bgr.reshape(-1, 3).astype(np.float32))


# ---- d. counting
@pytest.mark.parametrize("min_points", [1, 2])
def test_count_frame_voxels_is_n_out_at_each_size(hiplib, torch, reducer, frames, min_points):
    from cvo_slam_amd.voxels import frame_voxel_for_budget, voxel_ladder
    sizes = voxel_ladder(0.005, 3.0, 16)
    for name in ("67x65", "97x70s2", "plane", "64x64s16"):
        bgr, dep, step, (xyz, feat) = frames[name]
        t = tight(torch, bgr, dep)
        counts = reducer.count_frame_voxels([t, t], [pc.CAMERA, pc.CAMERA_B], sizes, cam_index=[0, 1], step=step, min_points=min_points)
        assert counts.shape == (2, 16) and counts.dtype == np.int32
        xb, fb = frd.dense_reading(bgr, dep, pc.CAMERA_B, step)
        want = np.array([[vr.count_reading(x, f, v, min_points) for v in sizes] for x, f in ((xyz, feat), (xb, fb))])
        np.testing.assert_array_equal(counts, want)
        dense = reducer.dense_frames([t], pc.CAMERA, step=step)[0]
        np.testing.assert_array_equal(reducer.count_voxels([(dense[0], dense[1], "points_first")], sizes, min_points)[0], counts[0])
        for j in (0, 5, 10, 15):
            got = reducer.reduce_frames([t, t], [pc.CAMERA, pc.CAMERA_B], float(sizes[j]), cam_index=[0, 1], step=step, min_points=min_points, want=())
            assert [g["n_out"] for g in got] == counts[:, j].tolist()
        if min_points == 1 and name != "64x64s16":
            v = frame_voxel_for_budget(reducer, t, pc.CAMERA, 300, 0.005, 3.0, step=step)
            j = int(np.flatnonzero(sizes == np.float32(v))[0])
            assert want[0, j] <= 300 and (j == 0 or want[0, j - 1] > 300)
            assert len(np.unique(want[0])) >= 6                        # (the ladder really spans the range)


# ---- e. fusion
@pytest.fixture(scope="module")
def keyframes():
    """64 frames of 64 x 64 at step 4 (256 points each): one scene's image and depth shifted a little from frame to frame, member 1 without any
    depth; a pose each.  [(bgr, depth)], [pose], [dense reading]"""
    rng = np.random.default_rng(5)
    bgr0, dep0 = pc.image(100, 70, "noise"), plane_depth(100, 70)
    dep0[rng.random(dep0.shape) < 0.1] = 0
    out, poses, dense = [], [], []
    for m in range(64):
        ox, oy = m % 8, (m // 8) % 6
        bgr, dep = np.ascontiguousarray(bgr0[oy:oy + 64, ox:ox + 64]), np.ascontiguousarray(dep0[oy:oy + 64, ox:ox + 64])
        if m == 1:
            dep = np.zeros_like(dep)
        P = fur.rigid(rng, 0.05, 0.1)
        out.append((bgr, dep)); poses.append(P); dense.append(frd.dense_reading(bgr, dep, pc.CAMERA_B if m % 2 else pc.CAMERA, 4))
    return out, poses, dense


@pytest.mark.parametrize("mode", ["mean", "central"])
def test_fuse_frames_is_the_fusion_of_the_dense_clouds(hiplib, torch, reducer, keyframes, mode):
    kf, poses, dense = keyframes
    tens = [tight(torch, b, d) for b, d in kf]
    cams = [pc.CAMERA, pc.CAMERA_B]
    groups = [list(range(0, 1)), list(range(0, 2)), list(range(0, 4)), list(range(0, 64))]     # 1, 2, 4 and 64 members; member 1 has no depth
    ci = [[m % 2 for m in g] for g in groups]
    for voxel, min_points, min_views in ((0.1, 1, 1), (0.1, 1, 2), (0.3, 2, 2), (64.0, 1, 1), (1e-4, 1, 1)):
        got = reducer.fuse_frames([[tens[m] for m in g] for g in groups], [[poses[m] for m in g] for g in groups], cams, voxel, cam_index=ci, step=4,
                                  mode=mode, min_points=min_points, min_views=min_views, want=FUSE_WANT)
        for k, g in enumerate(groups):
            want = fur.fuse_reading([dense[m] for m in g], [poses[m] for m in g], voxel, mode, min_points, min_views)
            same(got[k], want, (mode, voxel, min_points, min_views, len(g)), KEYS + ("views", "view_mask"))
            assert got[k]["offsets"].tolist() == [256 * j for j in range(len(g))]
            if len(g) >= 2:
                assert not (want["view_mask"] & np.uint64(2)).any()    # the member without depth keeps bit 1, and never sets it
            if len(g) == 4 and voxel == 0.1:
                assert want["n_out"] > 0 and (want["views"] >= min_views).all()
                if min_views == 1:                                     # (its successors keep bits 2 and 3)
                    assert (want["view_mask"] & np.uint64(4)).any() and (want["view_mask"] & np.uint64(8)).any()
    # the same through fuse on the dense clouds
    g = groups[2]
    dd = reducer.dense_frames([tens[m] for m in g], cams, cam_index=ci[2], step=4)
    a = reducer.fuse([[(x, f, "points_first") for x, f in dd]], [[poses[m] for m in g]], 0.1, mode, 1, 2, want=FUSE_WANT)[0]
    b = reducer.fuse_frames([[tens[m] for m in g]], [[poses[m] for m in g]], cams, 0.1, cam_index=[ci[2]], step=4, mode=mode, min_views=2, want=FUSE_WANT)[0]
    assert a["n_out"] == b["n_out"] and all(torch.equal(a[k], b[k]) for k in KEYS + ("views", "view_mask"))
    counted = reducer.fuse_frames([[tens[m] for m in g]], [[poses[m] for m in g]], cams, 0.1, cam_index=[ci[2]], step=4, mode=mode, min_views=2, cap=0, want=())[0]
    assert counted["n_out"] == a["n_out"]


# ---- f. refusals
def test_refusals_change_nothing(hiplib, torch, reducer, frames):
    api = hiplib.api
    L = api.load_library(); ip = C.POINTER(C.c_int)
    bgr, dep, step, (xyz, feat) = frames["64x64"]
    t = tight(torch, bgr, dep)
    good, w, h = api.device_image(*t)
    big = tight(torch, pc.image(185, 114, "noise"), pc.depth(185, 114))                # 21090 points: above max_points at step 1, below at step 2
    bigd, bw, bh = api.device_image(*big)
    hostmem = np.zeros((64, 64, 3), np.uint8)                          # pageable host memory
    img = lambda **kw: api.DeviceImage(**(dict(bgr8=good.bgr8, depth16=good.depth16, bgr_pitch=good.bgr_pitch, depth_pitch=good.depth_pitch,
                                                pixel_bytes=3, swap_rb=0) | kw))
    raws = [Raw(torch, 300, 4096) for _ in range(9)]
    recs = [r.record(api) for r in raws]
    torch.cuda.synchronize()
    nan, inf = float("nan"), float("inf")
    cam = lambda **kw: tuple((dict(zip(("s", "fx", "fy", "cx", "cy"), pc.CAMERA)) | kw).values())
    #         what                  images            w   h   step  cameras           cam_index
    cases = [("step 0",             [good],           w,  h,  0,    [pc.CAMERA],      None),
             ("step 17",            [good],           w,  h,  17,   [pc.CAMERA],      None),
             ("count > max_clouds", [good] * 9,       w,  h,  1,    [pc.CAMERA],      None),
             ("count 0",            [],               w,  h,  1,    [pc.CAMERA],      None),
             ("n > max_points",     [bigd],           bw, bh, 1,    [pc.CAMERA],      None),
             ("negative cam_index", [good, good],     w,  h,  1,    [pc.CAMERA],      [0, -1]),
             ("scaling_factor 0",   [good],           w,  h,  1,    [cam(s=0.0)],     None),
             ("fx 0",               [good],           w,  h,  1,    [cam(fx=0.0)],    None),
             ("fy 0",               [good, good],     w,  h,  1,    [pc.CAMERA, cam(fy=-0.0)], [0, 1]),
             ("fx NaN",             [good],           w,  h,  1,    [cam(fx=nan)],    None),
             ("cx inf",             [good],           w,  h,  1,    [cam(cx=inf)],    None),
             ("cy NaN",             [good],           w,  h,  1,    [cam(cy=nan)],    None),
             ("scaling_factor inf", [good],           w,  h,  1,    [cam(s=inf)],     None),
             ("null bgr8",          [img(bgr8=None)], w,  h,  1,    [pc.CAMERA],      None),
             ("pixel_bytes 5",      [img(pixel_bytes=5)], w, h, 1,  [pc.CAMERA],      None),
             ("swap_rb 2",          [img(swap_rb=2)], w,  h,  1,    [pc.CAMERA],      None),
             ("bgr_pitch short",    [img(bgr_pitch=100)], w, h, 1,  [pc.CAMERA],      None),
             ("depth16 odd",        [img(depth16=good.depth16 + 1)], w, h, 1, [pc.CAMERA], None),
             ("pageable bgr8",      [good, img(bgr8=hostmem.ctypes.data)], w, h, 1, [pc.CAMERA], None),
             ("width 63",           [good],           63, h,  1,    [pc.CAMERA],      None)]
    vs = np.array([0.05], np.float32)
    for what, images, cw, ch, cstep, cams, ci in cases:
        args, keep = lead(api, reducer, images, cw, ch, cstep, cams, ci)
        n = max(1, len(images))
        assert L.cvo_check_device_frames(*args) == INVALID, what
        assert L.cvo_last_error(), what
        rc, n_out = raw_reduce(api, reducer, args, recs[:n])
        assert rc == INVALID and (n_out == -7).all(), what
        counts = np.full(n, -7, np.int32)
        assert L.cvo_count_frame_voxels(*args, 1, vs.ctypes.data_as(C.POINTER(C.c_float)), 1, counts.ctypes.data_as(ip), None) == INVALID, what
        assert (counts == -7).all(), what
        dst = (api.FrameCloud * n)(*[api.FrameCloud(r.t["xyz"].data_ptr(), r.t["map"].data_ptr()) for r in raws[:n]])
        assert L.cvo_frames_to_device_clouds(*args, dst, None) == INVALID, what
        torch.cuda.synchronize()
        assert all(r.untouched() for r in raws), what
    args, keep = lead(api, reducer, [good, good], w, h, 1, [pc.CAMERA, cam(fy=0.0)], [0, 1])
    assert L.cvo_check_device_frames(*args) == INVALID and b"frame 1" in L.cvo_last_error() and b"fy" in L.cvo_last_error()
    # the reduction's own rules, and the dense cloud's dst
    args, keep = lead(api, reducer, [good], w, h, 1)
    assert L.cvo_check_device_frames(*args) == 0
    reducer.check_frames([t], pc.CAMERA)
    with pytest.raises(hiplib.CvoError, match="max_points"):
        reducer.check_frames([big], pc.CAMERA)
    reducer.check_frames([big], pc.CAMERA, step=2)
    for what, kw in (("voxel 0", dict(voxel=0.0)), ("voxel NaN", dict(voxel=nan)), ("mode 2", dict(mode=2)), ("min_points 0", dict(min_points=0))):
        rc, n_out = raw_reduce(api, reducer, args, recs[:1], **kw)
        assert rc == INVALID and (n_out == -7).all(), what
    host_map = np.full(4096, 0x5A5A5A5A, np.int32)                      # a map in pageable host memory
    rc, n_out = raw_reduce(api, reducer, args, [api.ReducedCloud(recs[0].xyz, recs[0].feat, None, None, host_map.ctypes.data, 300, 0)])
    assert rc == INVALID and b"map" in L.cvo_last_error() and (host_map == 0x5A5A5A5A).all() and (n_out == -7).all()
    rc, n_out = raw_reduce(api, reducer, args, [api.ReducedCloud(None, recs[0].feat, None, None, None, 300, 0)])
    assert rc == INVALID
    for k, bad in ((17, [0.1] * 17), (0, []), (2, [0.1, 0.0])):
        v = np.array(bad + [0.0], np.float32); counts = np.full(max(1, k), -7, np.int32)
        assert L.cvo_count_frame_voxels(*args, k, v.ctypes.data_as(C.POINTER(C.c_float)), 1, counts.ctypes.data_as(ip), None) == INVALID
        assert (counts == -7).all()
    dst = (api.FrameCloud * 1)(api.FrameCloud(raws[0].t["xyz"].data_ptr(), None))
    assert L.cvo_frames_to_device_clouds(*args, dst, None) == INVALID
    host_xyz = np.full(3 * 4096, 7.0, np.float32)                       # a dense cloud's positions in pageable host memory
    dst = (api.FrameCloud * 1)(api.FrameCloud(host_xyz.ctypes.data, raws[0].t["feat"].data_ptr()))
    assert L.cvo_frames_to_device_clouds(*args, dst, None) == INVALID and b"dst xyz" in L.cvo_last_error() and (host_xyz == 7.0).all()
    dst = (api.FrameCloud * 1)(api.FrameCloud(raws[0].t["xyz"].data_ptr() + 2, raws[0].t["feat"].data_ptr()))
    assert L.cvo_frames_to_device_clouds(*args, dst, None) == INVALID and b"aligned" in L.cvo_last_error()
    torch.cuda.synchronize()
    assert all(r.untouched() for r in raws)
    # the fusion's limits
    eye = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    bad_pose = (C.c_float * 12)(1, 0, 0, nan, 0, 1, 0, 0, 0, 0, 1, 0)
    fraws = [Raw(torch, 300, MAX_POINTS, arrays=("xyz", "feat", "count", "source", "map", "views", "view_mask"), fused=True) for _ in range(2)]
    frecs = [r.record(api) for r in fraws]
    torch.cuda.synchronize()
    member = lambda image=good, pose=eye, camera=0: api.FuseFrame(image, pose, camera, 0)

    def raw_fuse(first, members, recs, fw=w, fh=h, fstep=1, min_views=1, voxel=0.05, groups=None):
        arr = (api.FuseFrame * max(1, len(members)))(*members)
        gf = np.asarray(first, np.int32)
        cam_arr = (api.Camera * 1)(api.Camera(*pc.CAMERA))
        prm = api.FuseParams(voxel, 0, 1, min_views)
        out = (api.FusedCloud * len(recs))(*recs)
        g = len(first) - 1 if groups is None else groups
        n_out = np.full(max(1, g), -7, np.int32)
        a = [reducer.h, g, gf.ctypes.data_as(ip), arr, fw, fh, fstep, cam_arr, C.byref(prm), out]
        assert (L.cvo_check_fuse_frames(*a) == 0) == (L.cvo_fuse_device_frames(*a, n_out.ctypes.data_as(ip), None) == 0)
        return n_out

    fuse_cases = [("a group without members", dict(first=[0, 1, 1], members=[member()], recs=frecs)),
                  ("65 members", dict(first=[0, 65], members=[member()] * 65, recs=frecs[:1], fstep=16)),
                  ("5 x 4096 points above max_points", dict(first=[0, 5], members=[member()] * 5, recs=frecs[:1])),
                  ("group_first[0] != 0", dict(first=[1, 2], members=[member()] * 2, recs=frecs[:1])),
                  ("groups 0", dict(first=[0], members=[member()], recs=frecs[:1], groups=0)),
                  ("groups above max_clouds", dict(first=list(range(10)), members=[member()] * 9, recs=frecs[:1] * 9)),
                  ("min_views 0", dict(first=[0, 1], members=[member()], recs=frecs[:1], min_views=0)),
                  ("min_views 65", dict(first=[0, 1], members=[member()], recs=frecs[:1], min_views=65)),
                  ("voxel inf", dict(first=[0, 1], members=[member()], recs=frecs[:1], voxel=inf)),
                  ("a pose with a NaN", dict(first=[0, 2], members=[member(), member(pose=bad_pose)], recs=frecs[:1])),
                  ("a negative camera", dict(first=[0, 2], members=[member(), member(camera=-1)], recs=frecs[:1])),
                  ("step 17", dict(first=[0, 1], members=[member()], recs=frecs[:1], fstep=17)),
                  ("a null depth16", dict(first=[0, 2], members=[member(), member(image=img(depth16=None))], recs=frecs[:1])),
                  ("cap 65536", dict(first=[0, 1], members=[member()], recs=[api.FusedCloud(frecs[0].xyz, frecs[0].feat, None, None, None, None, None, 65536, 0)])),
                  ("view_mask not 8-byte aligned", dict(first=[0, 1], members=[member()],
                                                        recs=[api.FusedCloud(frecs[0].xyz, frecs[0].feat, None, None, None, None, frecs[0].view_mask + 4, 300, 0)]))]
    for what, kw in fuse_cases:
        n_out = raw_fuse(**kw)
        assert (n_out == -7).all() and L.cvo_last_error(), what
        torch.cuda.synchronize()
        assert all(r.untouched() for r in fraws + raws), what
    raw_fuse(first=[0, 2], members=[member(), member(pose=bad_pose)], recs=frecs[:1])
    assert b"group 0 member 1" in L.cvo_last_error() and b"pose[3]" in L.cvo_last_error()
    # and the reducer works after all that: 4 members of 4096 points fill max_points exactly
    n_out = raw_fuse(first=[0, 4], members=[member()] * 4, recs=frecs[:1])
    want = fur.fuse_reading([(xyz, feat)] * 4, [np.eye(4, dtype=np.float32)] * 4, 0.05)
    assert n_out.tolist() == [want["n_out"]] and want["n_out"] > 300
    assert fraws[0].host("xyz", np.float32).tobytes() == want["xyz"][:300].tobytes()
    assert fraws[0].guards_intact() and fraws[1].untouched()
    same(reducer.reduce_frames([t], pc.CAMERA, 0.05, want=WANT)[0], vr.reduce_reading(xyz, feat, 0.05), "after the refusals")


# ---- g. stream rule
def test_image_stream_orders_input_and_output(hiplib, torch, reducer, frames):
    bgr, dep, step, (xyz, feat) = frames["67x65"]
    want = vr.reduce_reading(xyz, feat, 0.05, 0, 1)
    side = torch.cuda.Stream()
    hb, hd = torch.from_numpy(bgr).pin_memory(), torch.from_numpy(dep.view(np.int16)).pin_memory()
    tb = torch.full(bgr.shape, 7, dtype=torch.uint8, device="cuda"); td = torch.zeros(dep.shape, dtype=torch.int16, device="cuda")
    a = torch.randn((4096, 4096), device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):                                             # work in front of the writes: without the edge in, the kernels would read depth 0
            a = a @ a * 1e-3
        tb.copy_(hb, non_blocking=True); td.copy_(hd, non_blocking=True)
    got = reducer.reduce_frames([(tb, td)], pc.CAMERA, 0.05, want=WANT, image_stream=side)[0]
    dense = reducer.dense_frames([(tb, td)], pc.CAMERA, image_stream=side)[0]
    with torch.cuda.stream(side):                                      # a read queued on that stream behind the calls, and an overwrite behind the read
        snap = {k: got[k].clone() for k in KEYS}
        dsnap = dense[0].clone()
        td.zero_()
        for k in KEYS:
            got[k].zero_()
    side.synchronize()
    same(dict(snap, n_out=got["n_out"]), want)
    np.testing.assert_array_equal(host(dsnap).view(np.uint32), xyz.view(np.uint32))


# ---- h. end to end
def test_reduced_frames_align_like_the_reading_s_rows(hiplib, torch):
    from cvo_slam_amd import synth
    from cvo_slam_amd.voxels import frame_voxel_for_budget
    R = hiplib.CvoReducer(2, 19200)
    (b0, d0), (b1, d1), _ = synth.make_frames(0)                       # 640 x 480; at step 4: 160 x 120 = 19200 points
    cam = synth.camera_tuple(synth.TUM1)
    tens = [tight(torch, np.ascontiguousarray(b0), np.ascontiguousarray(d0)), tight(torch, np.ascontiguousarray(b1), np.ascontiguousarray(d1))]
    voxel = frame_voxel_for_budget(R, tens[0], cam, 3072, 0.005, 1.0, step=4)
    got = R.reduce_frames(tens, cam, voxel, step=4, mode="mean", min_points=2, want=WANT)
    want = [vr.reduce_reading(*frd.dense_reading(b, d, cam, 4), voxel, "mean", 2) for b, d in ((b0, d0), (b1, d1))]
    for k in range(2):
        same(got[k], want[k], k)
        assert 300 < want[k]["n_out"] <= 3072
    B = hiplib.CvoBatch(1)
    B.set_pairs_clouds([(g["xyz"], g["feat"], "points_first") for g in got], [0], [1])      # the slices as they are: no copy
    B.align_async(1)
    r = B.wait(1)[0]
    Bh = hiplib.CvoBatch(1)
    Bh.set_pairs([(want[0]["xyz"], np.ascontiguousarray(want[0]["feat"].T), want[1]["xyz"], np.ascontiguousarray(want[1]["feat"].T))])
    q = Bh.align(1)[0]
    assert r["status"] == 0 and q["status"] == 0
    assert r["transform"].tobytes() == q["transform"].tobytes() and r["ell"] == q["ell"] and r["iter"] == q["iter"] and r["A_nonzero"] == q["A_nonzero"]
    B.close(); Bh.close(); R.close()
