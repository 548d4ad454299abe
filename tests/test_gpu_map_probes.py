"""Probing resident maps (cvo_maps_probe_clouds / cvo_maps_probe_frames, CvoMaps.probe / probe_frames) against the reading of the definition
(tests/map_probe_reading.py).  Every comparison is exact, on bytes: rows, squared distances, counts, views, stamps, hit bytes and the four
class counts; and after every call the maps are byte-identical."""
import ctypes as C

import numpy as np
import pytest

import frame_reading as frd
import fuse_reading as fr
import map_probe_reading as mp
import map_reading as mr
import map_view_reading as mv
import pcd_cases as pc
import voxel_reading as vr
from test_gpu_maps import snapshot, unchanged
from test_gpu_view_clouds import loaded_hip
from test_map_probe_reading import tie_maps

pytestmark = pytest.mark.gpu

INVALID = 4
KEYS = ("row", "dist2", "count", "views", "last_stamp", "hit")
WANT = ("dist2", "count", "views", "last_stamp")
EYE = np.eye(4, dtype=np.float32)
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 3000)
MAX_ROWS = 20000
LOOSEST = mv.FILTERS[0]
TWO_VIEWS = mv.filter_of(1, 2, -2 ** 31)
G = 64                                                                 # guard bytes behind every raw array


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


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev(torch, members):
    return [(up(torch, x), up(torch, f), "points_first") for x, f in members]


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else t


def same(got, want, what="", keys=KEYS, counts=True):
    for key in keys:
        g = host(got[key])
        assert g.dtype == want[key].dtype and g.shape == want[key].shape, (what, key, g.dtype, g.shape, want[key].shape)
        assert g.tobytes() == want[key].tobytes(), (what, key)
    if counts:
        assert got["counts"].dtype == np.int32 and got["counts"].tolist() == want["counts"].tolist(), (what, got["counts"], want["counts"])


def per_probe(flts):
    return {k: [f[k] for f in flts] for k in ("min_points", "min_views", "min_last_stamp")}


@pytest.fixture(scope="module")
def hist(hiplib, torch, reducer):
    """the small wall scene: map 0 stays empty, map 1 has map_view_reading.history, map 2 holds members 0 .. 2 in one call; the readings; and
    `world`, 3095 points of members 5 (never integrated) and 1 (integrated then removed) in the scene's frame"""
    S = mv.scene("small")
    members, poses = S["windows"]
    tens = dev(torch, members)
    steps, R1 = mv.history(S["windows"], MAX_ROWS)
    M = hiplib.CvoMaps(reducer, 3, MAX_ROWS, mv.VOXEL)
    for sign, m, st in steps:
        (M.integrate if sign > 0 else M.remove)([1], [[tens[m]]], [[poses[m]]], [[st]])
    M.integrate([2], [tens[:3]], [poses[:3]], [[0, 1, 2]])
    R2 = mr.Map(MAX_ROWS, mv.VOXEL); R2.update(members[:3], poses[:3], [0, 1, 2])
    parts = [fr.moved_concat([members[m]], [poses[m]]) for m in (5, 1)]
    world = (np.ascontiguousarray(np.concatenate([p[0] for p in parts])), np.ascontiguousarray(np.concatenate([p[1] for p in parts])))
    assert world[0].shape[0] >= 3000 and np.isfinite(world[0]).all()
    out = dict(S=S, M=M, R=[mr.Map(MAX_ROWS, mv.VOXEL), R1, R2], members=members, poses=poses, tens=tens, world=world)
    yield out
    M.close()


# ---- 1. member sizes, both reaches, eight probes a call
@pytest.mark.parametrize("reach", [0, 1, (0, 1, 1, 0, 1, 0, 0, 1)])
def test_edge_sizes_eight_probes_a_call(hiplib, torch, hist, reach):
    M, R, S = hist["M"], hist["R"], hist["S"]
    before = snapshot(M, None)
    wx, wf = hist["world"]
    for sizes, ks in ((SIZES[:8], [1, 2, 1, 1, 2, 0, 1, 2]), ((3000, 257, 1, 0, 64, 65, 63, 255), [1, 1, 2, 1, 0, 2, 1, 2])):
        assert ks.count(1) >= 2                                        # one map in several probes of the call
        clouds = [(np.ascontiguousarray(wx[:n]), np.ascontiguousarray(wf[:n])) for n in sizes]
        reaches = [reach] * 8 if isinstance(reach, int) else list(reach)
        got = M.probe(ks, dev(torch, clouds), S["poses"], reach=reach if isinstance(reach, int) else reaches, min_views=0, min_last_stamp=-2 ** 31, want=WANT, hit=True)
        assert len(got) == 8
        for k in range(8):
            want = mp.probe_reading(R[ks[k]], LOOSEST, clouds[k], S["poses"][k], reaches[k])
            same(got[k], want, (sizes[k], ks[k], reaches[k]))
            assert host(got[k]["row"]).shape == (sizes[k],) and host(got[k]["hit"]).shape == (R[ks[k]].rows,)
        big = got[sizes.index(3000)]["counts"] if 3000 in sizes else None
        assert big is None or (big[0] > 500 and big.sum() == 3000)
    unchanged(M, None, before)                                          # a probe only reads


# ---- 2. the filters
@pytest.mark.parametrize("reach", [0, 1])
def test_the_history_map_under_every_filter(hiplib, torch, hist, reach):
    M, R = hist["M"], hist["R"][1]
    flts = list(mv.FILTERS) + [TWO_VIEWS]
    for m in (5, 1):
        member, pose = hist["members"][m], hist["poses"][m]
        got = M.probe([1] * len(flts), [hist["tens"][m]] * len(flts), [pose] * len(flts), reach=reach, want=WANT, hit=True, **per_probe(flts))
        for k, flt in enumerate(flts):
            same(got[k], mp.probe_reading(R, flt, member, pose, reach), (m, k, reach))
        if m == 5:
            assert (got[-1]["counts"][:3] >= 100).all()                # found, absent and filtered all populated
        else:
            assert got[0]["counts"][2] >= (100 if reach == 0 else 0)   # the removed member's dead rows


# ---- 3. the tie and the rim
def test_the_tie_pair_and_the_rim(hiplib, torch, reducer):
    (ab, ba), point = tie_maps()
    f = point[1]
    a = (np.array([[0.75, 0.25, 0.25]], np.float32), f); b = (np.array([[1.25, 0.25, 0.25]], np.float32), f)
    M = hiplib.CvoMaps(reducer, 2, 8, 0.5)
    for k, (first, second) in enumerate(((a, b), (b, a))):
        M.integrate([k], [dev(torch, [first])], [[EYE]], [[0]]); M.integrate([k], [dev(torch, [second])], [[EYE]], [[1]])
    got = M.probe([0, 1, 0, 1], dev(torch, [point] * 4), [EYE] * 4, reach=[1, 1, 0, 0], min_views=0, want=WANT, hit=True)
    for k, (R, reach) in enumerate(((ab, 1), (ba, 1), (ab, 0), (ba, 0))):
        same(got[k], mp.probe_reading(R, LOOSEST, point, EYE, reach), ("tie", k))
    assert [int(host(g["row"])[0]) for g in got] == [0, 0, 1, 0] and all(float(host(g["dist2"])[0]) == 0.0625 for g in got)
    M.close()
    voxel = 2.0 ** -5
    hi = np.float32((2 ** 20 - 1) * voxel + voxel / 2); lo = np.float32(-(2 ** 20 - 1) * voxel + voxel / 2)
    f2 = np.zeros((2, 5), np.float32)
    pts = (np.array([[hi, hi, hi], [lo, lo, lo]], np.float32), f2)
    inner = ((pts[0] - np.float32(voxel) * np.sign(pts[0])).astype(np.float32), f2)
    mixed = (np.array([[hi, 0.0, lo], [lo, hi, 0.01]], np.float32), f2)         # rim cells in some coordinates only
    M = hiplib.CvoMaps(reducer, 1, 8, voxel); R = mr.Map(8, voxel)
    M.integrate([0], [dev(torch, [pts, mixed])], [[EYE, EYE]], [[0, 1]]); R.update([pts, mixed], [EYE, EYE], [0, 1])
    assert R.rows == 4
    clouds = [pts, inner, mixed, pts, inner, mixed]
    got = M.probe([0] * 6, dev(torch, clouds), [EYE] * 6, reach=[0, 0, 0, 1, 1, 1], min_views=0, want=WANT, hit=True)
    for k in range(6):
        same(got[k], mp.probe_reading(R, LOOSEST, clouds[k], EYE, k // 3), ("rim", k))
    assert host(got[0]["row"]).tolist() == [0, 1] and host(got[1]["row"]).tolist() == [-1, -1] and host(got[4]["row"]).tolist() == [0, 1]
    M.close()


# ---- 4. bad floats and far moves
def test_bad_floats_and_far_moves_are_invalid(hiplib, torch, reducer):
    rng = np.random.default_rng(43)
    x, f = fr.surface(rng, 600, 0.01)
    good = (x.copy(), f.copy())
    P = np.concatenate([x, f], axis=1)
    for j, val in enumerate([np.nan, np.inf, -np.inf, 32768.0, -40000.0]):    # one bad float in each of the 8 places
        for k in range(8):
            P[200 + 8 * j + k, k] = val
    bad = (np.ascontiguousarray(P[:, :3]), np.ascontiguousarray(P[:, 3:]))
    past_2_15 = EYE.copy(); past_2_15[0, 3] = 32767.5
    past_2_20 = EYE.copy(); past_2_20[1, 3] = 10485.0                  # at voxel 0.01 cell y' >= 2^20 for y >= 0.76
    zero_row = EYE.copy(); zero_row[0, 0] = 0.0                        # 0 * 40000 = 0: the source float must be refused on its own
    poses = [EYE, past_2_15, past_2_20, zero_row]
    for voxel in (0.25, 0.01):
        M = hiplib.CvoMaps(reducer, 1, MAX_ROWS, voxel); R = mr.Map(MAX_ROWS, voxel)
        M.integrate([0], [dev(torch, [good])], [[EYE]], [[0]]); R.update([good], [EYE], [0])
        for reach in (0, 1):
            got = M.probe([0] * 4, dev(torch, [bad] * 4), poses, reach=reach, want=WANT, hit=True)
            for k in range(4):
                want = mp.probe_reading(R, mv.filter_of(1, 1, 0), bad, poses[k], reach)
                same(got[k], want, (voxel, reach, k))
            assert got[0]["counts"][3] == 40 and got[1]["counts"][3] > 40 and got[3]["counts"][3] == 40
            assert (voxel == 0.25) or got[2]["counts"][3] > 40
        M.close()


# ---- 5. layouts
def test_layouts_give_the_tight_copy_s_bytes(hiplib, torch, hist):
    M, R = hist["M"], hist["R"][1]
    x, f = hist["members"][5]
    pose = hist["poses"][5]
    n = x.shape[0]
    rng = np.random.default_rng(2)
    float4 = (up(torch, np.concatenate([x, rng.normal(size=(n, 1)).astype(np.float32)], axis=1))[:, :3], up(torch, f.T), "channels_first")
    big = rng.normal(size=(n, 8)).astype(np.float32); big[:, 2:5] = x
    ff = rng.normal(size=(2 * n, 5)).astype(np.float32); ff[::2] = f
    strided = (up(torch, big)[:, 2:5], up(torch, ff)[::2], "points_first")
    for reach in (0, 1):
        want = mp.probe_reading(R, TWO_VIEWS, (x, f), pose, reach)
        got = M.probe([1] * 3, [hist["tens"][5], float4, strided], [pose] * 3, reach=reach, want=WANT, hit=True, **per_probe([TWO_VIEWS] * 3))
        for k in range(3):
            same(got[k], want, (reach, k))


# ---- 6. frames
@pytest.mark.parametrize("size,steps", [((64, 64), (1, 2, 3, 16)), ((100, 70), (1, 2, 3, 16))])
def test_frames_read_in_place(hiplib, torch, reducer, size, steps):
    """64 x 64 is the smallest frame cvo_check_device_images lets through (the refusals test holds a 64 x 48 frame to that rule)"""
    from cvo_slam_amd.voxels import probe_pixels
    w, h = size
    rng = np.random.default_rng(45)
    cams = [pc.CAMERA, pc.CAMERA_B]
    kf, poses, tens = [], [], []
    for m in range(4):
        bgr, dep = pc.image(w, h, "noise"), pc.depth(w, h, "holes" if m % 2 else "full")
        kf.append((bgr, dep)); poses.append(fr.rigid(rng, 0.02, 0.04))
        if m >= 2:                                                     # BGRA with both pitches above the rows' bytes
            bgra = rng.integers(0, 256, (h, w + 3, 4), dtype=np.uint8); bgra[:, :w, :3] = bgr
            wide = rng.integers(0, 65536, (h, w + 5), dtype=np.uint16); wide[:, :w] = dep
            tens.append((up(torch, bgra)[:, :w, :3], up(torch, wide.view(np.int16))[:, :w]))
        else:
            tens.append((up(torch, bgr), up(torch, dep.view(np.int16))))
    ci = [0, 1, 0, 1]
    voxel = 0.1
    M = hiplib.CvoMaps(reducer, 1, MAX_ROWS, voxel); R = mr.Map(MAX_ROWS, voxel)
    M.integrate_frames([0], [tens[:2]], [poses[:2]], [[0, 1]], cams, cam_index=[ci[:2]], step=2)
    R.update([frd.dense_reading(*kf[m], cams[ci[m]], 2) for m in range(2)], poses[:2], [0, 1])
    before = snapshot(M, None)
    for step in steps:
        dense = [mp.frame_member(*kf[m], cams[ci[m]], step) for m in range(4)]
        for reach in (0, 1):
            flts = [LOOSEST, TWO_VIEWS, LOOSEST, TWO_VIEWS]
            M.check_probe_frames([0] * 4, tens, poses, cams, cam_index=ci, step=step, reach=reach)
            got = M.probe_frames([0] * 4, tens, poses, cams, cam_index=ci, step=step, reach=reach, want=WANT, hit=True, **per_probe(flts))
            for m in range(4):
                want = mp.probe_reading(R, flts[m], dense[m], poses[m], reach)
                same(got[m], want, (size, step, reach, m))
                assert want["row"].shape == (-(-w // step) * -(-h // step),)
            assert got[0]["counts"][0] > 0 and (step == 16 or got[3]["counts"][3] > 0)      # found points; holes are invalid points
            img = probe_pixels(got[3]["row"], w, h, step)
            assert host(img).shape == (h, w) and np.array_equal(host(img)[::step, ::step].reshape(-1), host(got[3]["row"]))
    unchanged(M, None, before)
    M.close()


# ---- 7. raw calls: guard bytes, count only, no counts
class Raw:
    """one probe's output arrays as byte tensors prefilled with 0xA5, each with G guard bytes behind its extent"""
    NAMES = ("row", "dist2", "count", "views", "last_stamp", "hit")

    def __init__(self, torch, n, rows, arrays=NAMES):
        self.size = {k: (rows if k == "hit" else 4 * n) for k in arrays}
        self.t = {k: torch.full((b + G,), 0xA5, dtype=torch.uint8, device="cuda") for k, b in self.size.items()}

    def record(self, api, **over):
        ptr = {k: (self.t[k].data_ptr() if k in self.t else None) for k in self.NAMES} | over
        return api.ProbedPoints(*[ptr[k] for k in self.NAMES])

    def host(self, key):
        b = self.t[key].cpu().numpy()[:self.size[key]]
        return b if key == "hit" else b.view(np.float32 if key == "dist2" else np.int32)

    def guards_intact(self):
        return all((t.cpu().numpy()[self.size[k]:] == 0xA5).all() for k, t in self.t.items())

    def untouched(self):
        return all((t.cpu().numpy() == 0xA5).all() for t in self.t.values())


def member_of(api, tens, pose):
    d = tens if isinstance(tens, api.DeviceCloud) else api.device_cloud(*tens, max_n=api.REDUCE_MAX_POINTS)
    return api.FuseMember(d, (C.c_float * 12)(*np.asarray(pose, np.float32)[:3].reshape(-1).tolist()))


def probe_of(api, k, reach=0, flt=LOOSEST):
    return api.MapProbe(k, reach, api.MapFilter(flt["min_points"], flt["min_views"], flt["min_last_stamp"], 0))


def raw_probe(hiplib, M, probes, members, recs, counts=True, stream=None, check_only=False, n=None):
    api = hiplib.api
    n = len(probes) if n is None else n
    P = (api.MapProbe * max(1, len(probes)))(*probes); A = (api.FuseMember * max(1, len(members)))(*members); D = (api.ProbedPoints * max(1, len(recs)))(*recs)
    cnt = np.full((max(1, n), 4), -7, np.int32)
    if check_only:
        return M.L.cvo_check_maps_probe_clouds(M.h, n, P, A, D), cnt
    return M.L.cvo_maps_probe_clouds(M.h, n, P, A, D, cnt.ctypes.data_as(C.POINTER(C.c_int)) if counts else None, api._stream_arg(stream)), cnt


def test_guards_count_only_and_no_counts(hiplib, torch, hist):
    api = hiplib.api
    M, R = hist["M"], hist["R"]
    members, poses, tens = hist["members"], hist["poses"], hist["tens"]
    n5, n1 = members[5][0].shape[0], members[1][0].shape[0]
    raws = [Raw(torch, n5, R[1].rows), Raw(torch, n1, R[1].rows), Raw(torch, n5, R[2].rows, arrays=("row", "hit")), Raw(torch, n5, R[0].rows, arrays=("hit",))]
    probes = [probe_of(api, 1, 1, TWO_VIEWS), probe_of(api, 1, 0), probe_of(api, 2, 1), probe_of(api, 0, 1)]
    mem = [member_of(api, tens[5], poses[5]), member_of(api, tens[1], poses[1]), member_of(api, tens[5], poses[5]), member_of(api, tens[5], poses[5])]
    torch.cuda.synchronize()
    rc, cnt = raw_probe(hiplib, M, probes, mem, [r.record(api) for r in raws])
    assert rc == 0, api.load_library().cvo_last_error()
    wants = [mp.probe_reading(R[1], TWO_VIEWS, members[5], poses[5], 1), mp.probe_reading(R[1], LOOSEST, members[1], poses[1], 0),
             mp.probe_reading(R[2], LOOSEST, members[5], poses[5], 1), mp.probe_reading(R[0], LOOSEST, members[5], poses[5], 1)]
    for k, (r, want) in enumerate(zip(raws, wants)):
        assert r.guards_intact(), k
        for key in r.t:
            assert r.host(key).tobytes() == want[key].tobytes(), (k, key)
        assert cnt[k].tolist() == want["counts"].tolist(), k
    assert wants[3]["counts"][1] == n5 and raws[3].size["hit"] == 0    # the empty map: every valid point absent, no hit byte
    # count only: every array NULL
    rc, cnt = raw_probe(hiplib, M, probes, mem, [api.ProbedPoints()] * 4)
    assert rc == 0 and [c.tolist() for c in cnt] == [w["counts"].tolist() for w in wants]
    # counts NULL: the arrays alone, on the caller's stream without a host wait, and with no stream
    for stream in (torch.cuda.Stream(), None):
        fresh = [Raw(torch, n5, R[1].rows), Raw(torch, n1, R[1].rows)]
        torch.cuda.synchronize()
        rc, cnt = raw_probe(hiplib, M, probes[:2], mem[:2], [r.record(api) for r in fresh], counts=False, stream=stream)
        assert rc == 0 and (cnt == -7).all()
        if stream is not None:
            assert M.extract([2], cap=0, want=())[0]["n_out"] == R[2].extract()["n_out"]    # the next call on the reducer settles the table's copy
            stream.synchronize()
        for r, want in zip(fresh, wants[:2]):
            assert r.guards_intact() and all(r.host(key).tobytes() == want[key].tobytes() for key in r.t)
    got = M.probe([1, 1], [tens[5], tens[1]], [poses[5], poses[1]], reach=[1, 0], want=None, **per_probe([TWO_VIEWS, LOOSEST]))
    assert [set(g) for g in got] == [{"counts"}] * 2 and [g["counts"].tolist() for g in got] == [w["counts"].tolist() for w in wants[:2]]
    side = torch.cuda.Stream()
    got = M.probe([1], [tens[5]], [poses[5]], reach=1, want=WANT, hit=True, counts=None, cloud_stream=side, **per_probe([TWO_VIEWS]))[0]
    side.synchronize()
    assert "counts" not in got
    same(got, wants[0], "no counts", counts=False)


# ---- 8. many blocks, and rows past 65 536
def test_a_member_of_65537_points(hiplib, torch, hist):
    M, R = hist["M"], hist["R"][1]
    wx, wf = hist["world"]
    rng = np.random.default_rng(7)
    n = 65537                                                          # 257 blocks: the sum kernel's second trip
    pick = rng.integers(0, wx.shape[0], n)
    x = (wx[pick] + rng.normal(scale=0.02, size=(n, 3))).astype(np.float32); f = np.ascontiguousarray(wf[pick])
    x[65536] = wx[0]; x[65535] = np.nan
    for reach in (0, 1):
        want = mp.probe_reading(R, TWO_VIEWS, (x, f), EYE, reach)
        got = M.probe([1], dev(torch, [(x, f)]), [EYE], reach=reach, want=WANT, hit=True, **per_probe([TWO_VIEWS]))[0]
        same(got, want, reach)
        assert want["counts"].sum() == n and (want["counts"] > 0).all() and want["row"][65536] != mp.INVALID


def test_rows_past_65536(hiplib, torch):
    members, poses = mv.past_the_cap()
    red = hiplib.CvoReducer(2, 98304)
    M = hiplib.CvoMaps(red, 2, mv.PAST_MAX_ROWS, mv.PAST_VOXEL)
    R = mr.Map(mv.PAST_MAX_ROWS, mv.PAST_VOXEL)
    try:
        M.integrate([0], [dev(torch, members)], [poses], [[0, 1, 2]]); R.update(members, poses, [0, 1, 2])
        assert R.extract(**LOOSEST)["n_out"] > 65535
        rng = np.random.default_rng(8)
        x, f = members[2]
        # the last member's last points: the cells they were born into are the map's last rows
        cloud = (np.ascontiguousarray((x[-6000:] + rng.normal(scale=0.05, size=(6000, 3))).astype(np.float32)), np.ascontiguousarray(f[-6000:]))
        got = M.probe([0, 0], dev(torch, [cloud, cloud]), [poses[2]] * 2, reach=[0, 1], min_views=0, want=WANT, hit=True)
        for reach in (0, 1):
            want = mp.probe_reading(R, LOOSEST, cloud, poses[2], reach)
            same(got[reach], want, reach)
            assert (want["row"] > 65536).sum() > 100 and want["hit"][65536:].any()
    finally:
        M.close(); red.close()


# ---- 9. refusals
def test_refusals_launch_nothing_and_change_nothing(hiplib, torch, reducer, hist):
    api = hiplib.api
    M, R = hist["M"], hist["R"]
    tens, poses = hist["tens"], hist["poses"]
    n5 = hist["members"][5][0].shape[0]
    before = snapshot(M, None)
    good = member_of(api, tens[5], poses[5])
    raws = [Raw(torch, n5, R[1].rows) for _ in range(17)]
    recs = [r.record(api) for r in raws]
    r0 = raws[0]
    nan, inf = float("nan"), float("inf")

    def posed(k, val):
        m = api.FuseMember(good.cloud, good.pose); m.pose[k] = val; return m

    host_x = np.zeros((100, 3), np.float32)
    host_out = np.full(4 * n5, 0x5A, np.uint8)
    pageable = api.FuseMember(api.DeviceCloud(host_x.ctypes.data, good.cloud.feat, 12, 20, 4, 100, 0), good.pose)
    odd_stride = api.FuseMember(api.DeviceCloud(good.cloud.xyz, good.cloud.feat, 14, 20, 4, 100, 0), good.pose)
    too_many = api.FuseMember(api.DeviceCloud(good.cloud.xyz, good.cloud.feat, 12, 20, 4, 1048576, 0), good.pose)
    p1 = probe_of(api, 1)
    hip = loaded_hip()                                                  # an allocation of the runtime's own, so that its end is known: one byte short of hit
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; hip.hipFree.argtypes = [C.c_void_p]
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), R[1].rows - 1) == 0 and 4 * n5 > R[1].rows
    cases = [("probes 0", [p1], [good], recs[:1], dict(n=0)), ("probes 17", [p1] * 17, [good] * 17, recs, {}),
             ("map 3", [p1, probe_of(api, 3)], [good] * 2, recs[:2], {}), ("map -1", [probe_of(api, -1)], [good], recs[:1], {}),
             ("reach 2", [p1, api.MapProbe(1, 2, p1.filter)], [good] * 2, recs[:2], {}), ("reach -1", [api.MapProbe(1, -1, p1.filter)], [good], recs[:1], {}),
             ("min_views 65", [probe_of(api, 1, 0, mv.filter_of(1, 65, 0))], [good], recs[:1], {}), ("min_views -1", [probe_of(api, 1, 1, mv.filter_of(1, -1, 0))], [good], recs[:1], {}),
             ("pose NaN", [p1], [posed(7, nan)], recs[:1], {}), ("pose inf", [p1, p1], [good, posed(0, inf)], recs[:2], {}),
             ("pageable input", [p1, p1], [good, pageable], recs[:2], {}), ("stride 14", [p1, p1], [good, odd_stride], recs[:2], {}),
             ("n 1048576", [p1], [too_many], [api.ProbedPoints()], {}),
             ("pageable output", [p1], [good], [r0.record(api, row=host_out.ctypes.data)], {}),
             ("dist2 2 bytes off", [p1], [good], [r0.record(api, dist2=r0.t["dist2"].data_ptr() + 2)], {}),
             ("count too short", [p1], [good], [r0.record(api, count=short.value)], {}),
             ("hit too short", [p1], [good], [r0.record(api, hit=short.value)], {}),
             ("dist2 without row", [p1], [good], [r0.record(api, row=None)], {}),
             ("last_stamp without row", [p1], [good], [api.ProbedPoints(None, None, None, None, r0.t["last_stamp"].data_ptr(), None)], {})]
    torch.cuda.synchronize()
    msg = lambda: api.load_library().cvo_last_error().decode()
    for what, probes, mem, out, kw in cases:
        for check_only in (True, False):
            rc, cnt = raw_probe(hiplib, M, probes, mem, out, check_only=check_only, **kw)
            assert rc == INVALID, what
            assert msg(), what
            assert (cnt == -7).all(), what
        torch.cuda.synchronize()
        assert all(r.untouched() for r in raws), what
        assert (host_out == 0x5A).all(), what
    for call in (lambda: M.L.cvo_check_maps_probe_clouds(None, 1, None, None, None), lambda: M.L.cvo_check_maps_probe_clouds(M.h, 1, None, None, None),
                 lambda: M.L.cvo_maps_probe_frames(M.h, 1, (api.MapProbe * 1)(p1), None, 64, 48, 1, None, None, None, None)):
        assert call() == INVALID and "null" in msg()
    # the messages name probe and field
    raw_probe(hiplib, M, [p1, p1, p1], [good, good, posed(7, nan)], [api.ProbedPoints()] * 3)
    assert "probe 2" in msg() and "pose[7]" in msg()
    raw_probe(hiplib, M, [p1, api.MapProbe(1, 2, p1.filter)], [good] * 2, [api.ProbedPoints()] * 2)
    assert "probe 1" in msg() and "reach 2" in msg()
    raw_probe(hiplib, M, [p1, p1], [good] * 2, [api.ProbedPoints(), r0.record(api, hit=short.value)])
    assert "probe 1" in msg() and "dst hit" in msg()
    raw_probe(hiplib, M, [p1], [good], [r0.record(api, row=None)])
    assert "probe 0" in msg() and "dist2" in msg() and "row is null" in msg()
    rc, cnt = raw_probe(hiplib, M, [p1], [good], [api.ProbedPoints(None, None, None, None, None, r0.t["hit"].data_ptr())])
    assert rc == 0 and cnt[0].sum() == n5                              # hit stands without row
    hip.hipFree(short)
    # frames: the grid, the camera, the image
    frame = (torch.zeros((64, 64, 3), dtype=torch.uint8, device="cuda"), torch.zeros((64, 64), dtype=torch.int16, device="cuda"))
    low = (frame[0][:48], frame[1][:48])                               # 64 x 48: below the smallest device image
    with pytest.raises(hiplib.CvoError, match="image size out of range"):
        M.check_probe_frames([1], [low], [EYE], (5000.0, 58.3, 57.1, 31.2, 23.7))
    for match, kw in (("camera 0: fx is 0", dict(cameras=(5000.0, 0.0, 57.1, 31.2, 23.7))), ("scaling_factor is not finite", dict(cameras=(nan, 58.3, 57.1, 31.2, 23.7)))):
        with pytest.raises(hiplib.CvoError, match=match):
            M.check_probe_frames([1], [frame], [EYE], **kw)
    fm = api.FuseFrame(api.device_image(*frame)[0], good.pose, -1, 0)
    cam = (api.Camera * 1)(api.Camera(5000.0, 58.3, 57.1, 31.2, 23.7))
    for step, cam_i, text in ((0, 0, "step 0"), (17, 0, "step 17"), (1, -1, "camera index -1")):
        fm.cam = cam_i
        for fn, tail in ((M.L.cvo_check_maps_probe_frames, ()), (M.L.cvo_maps_probe_frames, (None, None))):
            assert fn(M.h, 1, (api.MapProbe * 1)(p1), (api.FuseFrame * 1)(fm), 64, 64, step, cam, (api.ProbedPoints * 1)(), *tail) == INVALID and text in msg()
    # a member above its region of the scratch: refused with both figures
    tiny = hiplib.CvoReducer(1, 1)
    T = hiplib.CvoMaps(tiny, 1, 16, 0.5)
    region = tiny.scratch_bytes()
    n_fit = 256 * (region // 16)
    x = torch.zeros((n_fit + 1, 3), dtype=torch.float32, device="cuda"); f = torch.zeros((n_fit + 1, 5), dtype=torch.float32, device="cuda")
    with pytest.raises(hiplib.CvoError, match=f"{n_fit + 1} points takes {region + 16} bytes of scratch, above the {region} bytes"):
        T.check_probe([0], [(x, f, "points_first")], [EYE])
    assert T.probe([0], [(x[:n_fit], f[:n_fit], "points_first")], [EYE], reach=1)[0]["counts"].tolist() == [0, n_fit, 0, 0]   # far above max_points, and it fits
    T.close(); tiny.close()
    with pytest.raises(hiplib.CvoError, match="probes 17"):
        M.check_probe([1] * 17, [tens[5]] * 17, [EYE] * 17)
    unchanged(M, None, before)
    same(M.probe([1], [tens[5]], [poses[5]], reach=1, min_views=2, min_last_stamp=-2 ** 31, want=WANT, hit=True)[0],
         mp.probe_reading(R[1], TWO_VIEWS, hist["members"][5], poses[5], 1), "after the refusals")


# ---- 10. the stream rule
def test_stream_orders_input_and_output(hiplib, torch, hist):
    M, R = hist["M"], hist["R"][1]
    x, f = hist["members"][5]
    pose = hist["poses"][5]
    want = mp.probe_reading(R, TWO_VIEWS, (x, f), pose, 1)
    side = torch.cuda.Stream()
    hx, hf = torch.from_numpy(x).pin_memory(), torch.from_numpy(f).pin_memory()
    tx = torch.full(x.shape, 1000.0, dtype=torch.float32, device="cuda"); tf = torch.zeros(f.shape, dtype=torch.float32, device="cuda")
    a = torch.randn((4096, 4096), device="cuda")
    torch.cuda.synchronize()
    for counts in (True, None):
        tx.fill_(1000.0); torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(8):                                         # work in front of the writes: without the edge in, the kernel would read the 1000s
                a = a @ a * 1e-3
            tx.copy_(hx, non_blocking=True); tf.copy_(hf, non_blocking=True)
        got = M.probe([1], [(tx, tf, "points_first")], [pose], reach=1, want=WANT, hit=True, counts=counts, cloud_stream=side, **per_probe([TWO_VIEWS]))[0]
        with torch.cuda.stream(side):                                  # a read queued on that stream behind the call, and overwrites behind the read
            snap = {k: got[k].clone() for k in KEYS}
            for k in KEYS:
                got[k].zero_()
            tx.fill_(-3.0)
        side.synchronize()
        same(dict(snap, counts=got.get("counts")), want, counts, counts=bool(counts))


# ---- 11. coexistence, table sizes, compaction
def test_every_kind_of_call_interleaved_on_one_reducer(hiplib, torch, reducer, hist):
    members, poses, tens = hist["members"], hist["poses"], hist["tens"]
    S = hist["S"]
    M = hiplib.CvoMaps(reducer, 2, MAX_ROWS, mv.VOXEL)
    R = mr.Map(MAX_ROWS, mv.VOXEL)
    scratch = reducer.scratch_bytes()
    for t in range(4):
        M.integrate([1], [[tens[t]]], [[poses[t]]], [[t]]); R.update([members[t]], [poses[t]], [t])
        g = reducer.reduce([tens[t]], 0.05, "mean", 1, want=("count",))[0]
        w = vr.reduce_reading(members[t][0], members[t][1], 0.05, "mean", 1)
        assert g["n_out"] == w["n_out"] and host(g["xyz"]).tobytes() == w["xyz"].tobytes()
        p = M.probe([1, 1], [tens[t + 1], tens[5]], [poses[t + 1], poses[5]], reach=[t % 2, 1 - t % 2], min_views=[1, 2], want=WANT, hit=True)
        assert host(reducer.fuse([tens[:t + 1]], [poses[:t + 1]], 0.05, want=("count",))[0]["xyz"]).tobytes() == fr.fuse_reading(members[:t + 1], poses[:t + 1], 0.05)["xyz"].tobytes()
        v = M.view([1], [S["poses"][t]], S["camera"], S["size"], cell=2, want=("source",))[0]
        e = M.extract([1], want=("row",))[0]
        cv = reducer.view([(e["xyz"], e["feat"], "points_first")], [S["poses"][t]], S["camera"], S["size"], cell=2, want=("source",))[0]
        assert v["n_out"] == cv["n_out"] > 0
        same(p[0], mp.probe_reading(R, mv.filter_of(1, 1, 0), members[t + 1], poses[t + 1], t % 2), (t, 0))
        same(p[1], mp.probe_reading(R, mv.filter_of(1, 2, 0), members[5], poses[5], 1 - t % 2), (t, 1))
    assert reducer.scratch_bytes() == scratch
    M.close()


def test_two_table_sizes_and_a_compaction_between_two_probes(hiplib, torch, reducer, hist):
    members, poses, tens = hist["members"], hist["poses"], hist["tens"]
    runs = []
    for max_rows in (MAX_ROWS, 3500):                                  # another table size: another layout, which must not show
        M = hiplib.CvoMaps(reducer, 1, max_rows, mv.VOXEL)
        for sign, m, st in hist_steps():
            (M.integrate if sign > 0 else M.remove)([0], [[tens[m]]], [[poses[m]]], [[st]])
        first = M.probe([0, 0], [tens[5]] * 2, [poses[5]] * 2, reach=[0, 1], want=WANT, hit=True, **per_probe([TWO_VIEWS] * 2))
        new_row = M.compact([0], min_views=2, probation_from=9, new_row=True)[1][0]
        second = M.probe([0, 0], [tens[5]] * 2, [poses[5]] * 2, reach=[0, 1], want=WANT, hit=True, **per_probe([LOOSEST] * 2))
        runs.append(([{k: (host(v).copy() if hasattr(v, "cpu") else v) for k, v in g.items()} for g in first + second], host(new_row).copy()))
        M.close()
    steps, R = mv.history((members, poses), MAX_ROWS)
    assert R.rows <= 3500
    wants = [mp.probe_reading(R, TWO_VIEWS, members[5], poses[5], reach) for reach in (0, 1)]
    moved = R.compact(min_views=2, probation_from=9)
    assert (moved == -1).any() and (moved >= 0).any()
    wants += [mp.probe_reading(R, LOOSEST, members[5], poses[5], reach) for reach in (0, 1)]
    for got, new_row in runs:
        assert np.array_equal(new_row, moved)
        for k in range(4):
            same(got[k], wants[k], k)
    assert wants[2]["hit"].shape != wants[0]["hit"].shape and (wants[3]["row"] >= 0).sum() > 100


def hist_steps():
    return [(1, 0, 0), (1, 1, 1), (1, 2, 2), (1, 3, 3), (-1, 1, 1), (1, 4, 9)]
