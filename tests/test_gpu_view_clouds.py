"""Viewing posed device clouds (cvo_view_device_clouds, CvoReducer.view) against the numpy reading of its definition (tests/view_reading.py).
Every comparison with the reading is exact, on bytes: positions, features, sources, pixels, relations, maps, the two z-buffer images, the row
counts and the relation counts."""
import ctypes as C

import numpy as np
import pytest

import fuse_reading as fr
import view_reading as vw
import voxel_reading as vr

pytestmark = pytest.mark.gpu

INVALID = 4
KEYS = ("xyz", "feat", "source", "pixel", "map", "depth", "index")
WANT = ("source", "pixel", "map", "depth", "index")
ALL = WANT + ("relation",)
EYE = np.eye(4, dtype=np.float32)
MODES = (("front", 0.0), ("surface", 0.0), ("surface", 0.05))


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
def scenes(torch):
    """both scenes of tests/view_reading.py with their clouds on the device and, per view of either call, the observed depth of the relation
    comparisons: the view's own rendering shifted by bands"""
    out = {}
    for which in ("small", "wide"):
        S = vw.scene(which)
        S["tens"] = {n: dev(torch, c) for n, c in S["clouds"].items()}
        S["observed"] = [[vw.shifted_rendering(S["clouds"][n], S["poses"][k], S["camera"], S["size"]) for k, n in enumerate(call)] for call in vw.SCENE_CALLS]
        out[which] = S
    return out


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev(torch, cloud):
    return (up(torch, cloud[0]), up(torch, cloud[1]), "points_first")


def up_depth(torch, d):
    """a uint16 depth image on the device, in torch's int16 carrier (the same bytes)"""
    return up(torch, np.asarray(d, np.uint16).view(np.int16))


def loaded_hip():
    """the HIP runtime this process already has (torch's copy: tests/conftest.py)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise AssertionError("no HIP runtime loaded")


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else t


def same(got, want, what="", keys=KEYS):
    assert got["n_out"] == want["n_out"], (what, got["n_out"], want["n_out"])
    for key in keys:
        g = host(got[key])
        assert g.dtype == want[key].dtype and g.shape == want[key].shape, (what, key, g.dtype, g.shape, want[key].shape)
        assert g.tobytes() == want[key].tobytes(), (what, key)
    if "relation" in keys:
        assert np.array_equal(got["relation_counts"], want["relation_counts"]), (what, got["relation_counts"], want["relation_counts"])


def mode_of(name):
    return dict(front=vw.FRONT, surface=vw.SURFACE)[name]


# ---- 1. boundaries
@pytest.mark.parametrize("cell", [1, 2, 3, 16])
@pytest.mark.parametrize("which", ["small", "wide"])
def test_boundaries_one_call_of_eight_views(hiplib, torch, reducer, scenes, which, cell):
    S = scenes[which]
    w, h = S["size"]
    for mode, slack in MODES:
        p = vw.params(w, h, cell, mode_of(mode), slack)
        for call, obs in zip(vw.SCENE_CALLS, S["observed"]):
            assert call.count(3000) == 2                               # the same cloud in two views, under different poses
            got = reducer.view([S["tens"][n] for n in call], S["poses"], S["camera"], (w, h), cell, mode, slack,
                               observed=[up_depth(torch, o) for o in obs], want=ALL)
            assert len(got) == 8
            for k, n in enumerate(call):
                want = vw.view_reading(S["clouds"][n], S["poses"][k], S["camera"], p, obs[k])
                same(got[k], want, (which, cell, mode, slack, k, n), KEYS + ("relation",))
                assert host(got[k]["depth"]).shape == (-(-h // cell), -(-w // cell))
            assert got[0]["n_out"] == 0 or call[0] != 0
            rows = [g["n_out"] for g, n in zip(got, call) if n == 3000]
            assert min(rows) > 0 and (mode != "front" or max(rows) <= -(-w // cell) * -(-h // cell))


# ---- 2. the edges of the definition
def test_edges_of_the_definition(hiplib, torch, reducer):
    x, f, names = vw.edge_cloud()
    cloud = (x, f)
    t = dev(torch, cloud)
    w, h = vw.EDGE_SIZE
    empty = (torch.zeros((0, 3), dtype=torch.float32, device="cuda"), torch.zeros((0, 5), dtype=torch.float32, device="cuda"), "points_first")
    for mode, slack in MODES:
        for z_range in ((0.05, 30.0), (1e-6, 30.0)):
            p = vw.params(w, h, 1, mode_of(mode), slack, z_near=z_range[0], z_far=z_range[1])
            got = reducer.view([t, t, empty], [EYE, vw.EDGE_FAR_MOVE, EYE], vw.EDGE_CAM, (w, h), 1, mode, slack, z_range=z_range, want=WANT)
            same(got[0], vw.view_reading(cloud, EYE, vw.EDGE_CAM, p), (mode, slack, z_range, "identity"))
            same(got[1], vw.view_reading(cloud, vw.EDGE_FAR_MOVE, vw.EDGE_CAM, p), (mode, slack, z_range, "past 2^15"))
            none = vw.view_reading((np.zeros((0, 3), np.float32), np.zeros((0, 5), np.float32)), EYE, vw.EDGE_CAM, p)
            same(got[2], none, (mode, slack, z_range, "empty"))
            assert got[1]["n_out"] == 0 and got[2]["n_out"] == 0 and (host(got[2]["index"]) == -1).all() and (host(got[2]["depth"]) == 0).all()
    m = host(reducer.view([t], [EYE], vw.EDGE_CAM, (w, h), want=("map", "index"))[0]["map"])
    assert m[0] >= 0 and m[1] == -2 and m[2] == -2 and m[3] >= 0 and m[12] >= 0 and m[13] == -1   # (tests/test_view_reading.py holds all of them)


def test_layouts_give_the_tight_copy_s_bytes(hiplib, torch, reducer, scenes):
    S = scenes["small"]
    x, f = S["clouds"][3000]
    n = x.shape[0]
    rng = np.random.default_rng(2)
    big = rng.normal(size=(n, 8)).astype(np.float32); big[:, 2:5] = x
    ff = rng.normal(size=(2 * n, 5)).astype(np.float32); ff[::2] = f
    bx = rng.normal(size=3 * n + 1).astype(np.float32); bx[1:] = x.reshape(-1)
    other = [(up(torch, np.concatenate([x, rng.normal(size=(n, 1)).astype(np.float32)], axis=1))[:, :3], up(torch, f.T), "channels_first"),   # float4 points, channel-major
             (up(torch, big)[:, 2:5], up(torch, ff)[::2], "points_first"),                # columns of a wider tensor, every other row
             (up(torch, bx)[1:].view(n, 3), up(torch, f.T), "channels_first")]            # 4 bytes past a 16-byte boundary
    d = [hiplib.api.device_cloud(*c, max_n=hiplib.api.REDUCE_MAX_POINTS) for c in other]
    assert [q.xyz_stride for q in d] == [16, 32, 12] and [q.feat_point_stride for q in d] == [4, 40, 4]
    w, h = S["size"]
    for mode, slack in MODES:
        want = vw.view_reading((x, f), S["poses"][0], S["camera"], vw.params(w, h, 2, mode_of(mode), slack))
        got = reducer.view([S["tens"][3000]] + other, [S["poses"][0]] * 4, S["camera"], (w, h), 2, mode, slack, want=WANT)
        for k in range(4):
            same(got[k], want, (mode, slack, k))


# ---- the C ABI itself, with arrays of the test's own
class Raw:
    """one view's output arrays as byte tensors prefilled with 0xA5, each with 64 guard bytes behind its extent"""
    G = 64
    ROW = dict(xyz=12, feat=20, source=4, pixel=4, relation=4)
    ORDER = ("xyz", "feat", "source", "pixel", "relation", "map", "depth", "index")

    def __init__(self, torch, cap, n_in, cells, arrays=ORDER):
        self.cap = cap
        self.sizes = {k: b * cap for k, b in self.ROW.items()} | dict(map=4 * n_in, depth=4 * cells, index=4 * cells)
        self.t = {k: torch.full((self.sizes[k] + self.G,), 0xA5, dtype=torch.uint8, device="cuda") for k in arrays}

    def record(self, api, **over):
        p = lambda k: over[k] if k in over else (self.t[k].data_ptr() if k in self.t else None)
        return api.ViewedCloud(*[p(k) for k in self.ORDER], over.get("cap", self.cap), 0)

    def host(self, key, dtype):
        return self.t[key].cpu().numpy()[:self.sizes[key]].view(dtype)

    def guards_intact(self):
        return all((t.cpu().numpy()[self.sizes[k]:] == 0xA5).all() for k, t in self.t.items())

    def untouched(self):
        return all((t.cpu().numpy() == 0xA5).all() for t in self.t.values())


def a_view(api, tens, pose, cam=0):
    d = tens if isinstance(tens, api.DeviceCloud) else api.device_cloud(*tens, max_n=api.REDUCE_MAX_POINTS)
    return api.View(d, (C.c_float * 12)(*np.asarray(pose, np.float32)[:3].reshape(-1).tolist()), cam, 0)


def raw_view(hiplib, R, views, recs, cams, size=(64, 48), cell=1, mode=0, z_near=0.05, z_far=30.0, slack=0.0, depth_tol=0.02, observed=None, stream=None,
             count=None, check_only=False, want_counts=True):
    api = hiplib.api
    count = len(views) if count is None else count
    arr = (api.View * max(1, len(views)))(*views); out = (api.ViewedCloud * max(1, len(recs)))(*recs)
    cs = (api.Camera * len(cams))(*[api.Camera(*c) for c in cams])
    prm = api.ViewParams(size[0], size[1], cell, mode, z_near, z_far, slack, depth_tol)
    obs = None if observed is None else (api.DeviceImage * len(observed))(*observed)
    n_out = np.full(max(1, count), -7, np.int32); counts = np.full((max(1, count), 4), -7, np.int32)
    ip = C.POINTER(C.c_int)
    if check_only:
        return R.L.cvo_check_view_clouds(R.h, count, arr, cs, C.byref(prm), obs, out), n_out, counts
    rc = R.L.cvo_view_device_clouds(R.h, count, arr, cs, C.byref(prm), obs, out, n_out.ctypes.data_as(ip), counts.ctypes.data_as(ip) if want_counts else None, stream)
    return rc, n_out, counts


def depth_image(api, t, pitch=0):
    return api.DeviceImage(None, t.data_ptr(), 0, pitch, 3, 0)


# ---- 3. cap
@pytest.mark.parametrize("mode,slack", [(0, 0.0), (1, 0.05)], ids=["front", "surface"])
def test_cap_below_the_row_count(hiplib, torch, reducer, scenes, mode, slack):
    api = hiplib.api
    S = scenes["small"]
    w, h = S["size"]
    cloud, pose, obs = S["clouds"][3000], S["poses"][6], S["observed"][0][6]
    want = vw.view_reading(cloud, pose, S["camera"], vw.params(w, h, 2, mode, slack), obs)
    cap = 100
    assert want["n_out"] > cap and want["relation"][cap:].shape[0] > 0
    raw = Raw(torch, cap, 3000, (w // 2) * (h // 2))
    d_obs = up_depth(torch, obs)
    views = [a_view(api, S["tens"][3000], pose)]
    torch.cuda.synchronize()
    rc, n_out, counts = raw_view(hiplib, reducer, views, [raw.record(api)], [S["camera"]], (w, h), 2, mode, slack=slack, observed=[depth_image(api, d_obs)])
    assert rc == 0, api.load_library().cvo_last_error()
    torch.cuda.synchronize()
    assert n_out[0] == want["n_out"]                                   # the full row count
    for key, dt in (("xyz", np.float32), ("feat", np.float32), ("source", np.int32), ("pixel", np.int32), ("relation", np.int32)):
        assert raw.host(key, dt).tobytes() == want[key][:cap].tobytes(), key
    assert raw.host("map", np.int32).tobytes() == want["map"].tobytes() and want["map"].max() == want["n_out"] - 1   # full row numbers
    assert raw.host("depth", np.float32).tobytes() == want["depth"].tobytes() and raw.host("index", np.int32).tobytes() == want["index"].tobytes()
    assert counts[0].tolist() == want["relation_counts"].tolist() and counts[0].sum() == want["n_out"]   # over all rows, those past cap too
    assert raw.guards_intact()
    with pytest.raises(hiplib.CvoError, match="cap 100"):
        reducer.view([S["tens"][3000]], [pose], S["camera"], (w, h), 2, mode, slack, cap=100)
    # cap = 0 with only depth asked for: counts, and writes the one image
    only = Raw(torch, 0, 3000, (w // 2) * (h // 2), arrays=("depth",))
    rc, n_out, counts = raw_view(hiplib, reducer, views, [only.record(api)], [S["camera"]], (w, h), 2, mode, slack=slack, want_counts=False)
    assert rc == 0 and n_out[0] == want["n_out"]
    torch.cuda.synchronize()
    assert only.host("depth", np.float32).tobytes() == want["depth"].tobytes() and only.guards_intact()
    counted = reducer.view([S["tens"][3000]], [pose], S["camera"], (w, h), 2, mode, slack, cap=0, want=("depth",))[0]
    assert counted["n_out"] == want["n_out"] and counted["xyz"].shape[0] == 0 and host(counted["depth"]).tobytes() == want["depth"].tobytes()
    rc, n_out, counts = raw_view(hiplib, reducer, views, [api.ViewedCloud(None, None, None, None, None, None, None, None, 0, 0)], [S["camera"]], (w, h), 2, mode, slack=slack)
    assert rc == 0 and n_out[0] == want["n_out"] and counts[0].tolist() == [0, 0, 0, 0]   # every array NULL: the count alone


# ---- 4. relation
@pytest.mark.parametrize("which", ["small", "wide"])
def test_relation_against_a_shifted_rendering(hiplib, torch, reducer, scenes, which):
    S = scenes[which]
    w, h = S["size"]
    cloud, pose, obs = S["clouds"][3000], S["poses"][6], S["observed"][0][6]
    padded = torch.zeros((h + 3, w + 6), dtype=torch.int16, device="cuda")                # the observed depth as a crop of a larger image
    crop = padded[2:2 + h, 4:4 + w]
    crop.copy_(up(torch, obs.view(np.int16)))
    for (mode, slack), cell, tol in zip(MODES, (1, 2, 3), (0.02, 0.0, 0.3)):
        want = vw.view_reading(cloud, pose, S["camera"], vw.params(w, h, cell, mode_of(mode), slack, depth_tol=tol), obs)
        for carrier in (up_depth(torch, obs), crop, (None, crop)):
            got = reducer.view([S["tens"][3000]], [pose], S["camera"], (w, h), cell, mode, slack, observed=[carrier], depth_tol=tol, want=ALL)[0]
            same(got, want, (which, mode, cell, tol), KEYS + ("relation",))
        # the cloud as a descriptor and the observed depth fresh from a kernel on torch's current stream: view settles that writer too
        desc = hiplib.api.device_cloud(*S["tens"][3000], max_n=hiplib.api.REDUCE_MAX_POINTS)
        got = reducer.view([desc], [pose], S["camera"], (w, h), cell, mode, slack, observed=[(crop + 1) - 1], depth_tol=tol, want=ALL)[0]
        same(got, want, (which, mode, cell, tol, "descriptor"), KEYS + ("relation",))
        if tol == 0.02:
            assert (want["relation_counts"] >= 0.02 * want["n_out"]).all()   # all four values are there
        if tol == 0.3:
            assert want["relation_counts"][1] == 0 and want["relation_counts"][3] == 0   # 1.2 and 0.8 times agree within 30 %


# ---- 5. refusals
def test_refusals_change_nothing(hiplib, torch, reducer, scenes):
    api = hiplib.api
    S = scenes["small"]
    cam = S["camera"]
    tens = S["tens"][3000]
    good = a_view(api, tens, S["poses"][0])
    want = vw.view_reading(S["clouds"][3000], S["poses"][0], cam, vw.params(64, 48))
    scratch_before = reducer.scratch_bytes()
    raws = [Raw(torch, 300, 3000, 64 * 48) for _ in range(9)]
    recs = [r.record(api) for r in raws]
    r0 = raws[0]
    bigx = torch.zeros((32769, 3), dtype=torch.float32, device="cuda"); bigf = torch.zeros((32769, 5), dtype=torch.float32, device="cuda")
    too_big = a_view(api, (bigx, bigf, "points_first"), EYE)
    host_x = np.zeros((100, 3), np.float32)                              # pageable host memory
    pageable = api.View(api.DeviceCloud(host_x.ctypes.data, good.cloud.feat, 12, 20, 4, 100, 0), good.pose, 0, 0)
    odd_stride = api.View(api.DeviceCloud(good.cloud.xyz, good.cloud.feat, 14, 20, 4, 100, 0), good.pose, 0, 0)
    def posed(k, val):
        v = api.View(good.cloud, good.pose, 0, 0); v.pose[k] = val; return v
    host_out = np.full(12 * 300, 0x5A, np.uint8)
    d_obs = torch.zeros((48, 64), dtype=torch.int16, device="cuda")
    hip = loaded_hip()                                                  # an allocation of the runtime's own, so that its end is known: 47 rows of depth
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; hip.hipFree.argtypes = [C.c_void_p]
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), 47 * 128) == 0
    host_obs = np.zeros((48, 64), np.uint16)
    ok_obs = [depth_image(api, d_obs)]
    no_relation = Raw(torch, 300, 3000, 64 * 48, arrays=("xyz", "feat"))
    nan, inf = float("nan"), float("inf")
    one = [good]
    cases = [("views 0", one, recs[:1], dict(count=0)), ("views 9", [good] * 9, recs, {}),
             ("n > max_points", [good, too_big], recs[:2], {}), ("z-cells > max_points", one, recs[:1], dict(size=(256, 256))),
             ("width 0", one, recs[:1], dict(size=(0, 48))), ("width 8193", one, recs[:1], dict(size=(8193, 1), cell=16)),
             ("height 0", one, recs[:1], dict(size=(64, 0))), ("height 8193", one, recs[:1], dict(size=(1, 8193), cell=16)),
             ("cell 0", one, recs[:1], dict(cell=0)), ("cell 17", one, recs[:1], dict(cell=17)), ("mode 2", one, recs[:1], dict(mode=2)), ("mode -1", one, recs[:1], dict(mode=-1)),
             ("z_near 0", one, recs[:1], dict(z_near=0.0)), ("z_near negative", one, recs[:1], dict(z_near=-1.0)), ("z_near NaN", one, recs[:1], dict(z_near=nan)),
             ("z_near inf", one, recs[:1], dict(z_near=inf)), ("z_far = z_near", one, recs[:1], dict(z_near=1.0, z_far=1.0)), ("z_far NaN", one, recs[:1], dict(z_far=nan)),
             ("z_far inf", one, recs[:1], dict(z_far=inf)), ("z_far above 32768", one, recs[:1], dict(z_far=32769.0)),
             ("slack negative", one, recs[:1], dict(slack=-0.1)), ("slack NaN", one, recs[:1], dict(slack=nan)), ("slack inf", one, recs[:1], dict(slack=inf)),
             ("depth_tol negative", one, recs[:1], dict(depth_tol=-0.1)), ("depth_tol NaN", one, recs[:1], dict(depth_tol=nan)),
             ("pose NaN", [posed(7, nan)], recs[:1], {}), ("pose inf", [good, posed(0, inf)], recs[:2], {}),
             ("camera index -1", [api.View(good.cloud, good.pose, -1, 0)], recs[:1], {}),
             ("camera fx NaN", one, recs[:1], dict(cams=[(5000.0, nan, 57.1, 31.2, 23.7)])), ("camera cy inf", one, recs[:1], dict(cams=[(5000.0, 58.3, 57.1, 31.2, inf)])),
             ("camera fx 0", one, recs[:1], dict(cams=[(5000.0, 0.0, 57.1, 31.2, 23.7)])), ("camera fy 0", one, recs[:1], dict(cams=[(5000.0, 58.3, 0.0, 31.2, 23.7)])),
             ("camera scaling_factor 0", one, recs[:1], dict(cams=[(0.0, 58.3, 57.1, 31.2, 23.7)])),
             ("pageable input", [good, pageable], recs[:2], {}), ("stride 14", [good, odd_stride], recs[:2], {}),
             ("pageable output", one, [r0.record(api, xyz=host_out.ctypes.data)], {}), ("cap 65536", one, [r0.record(api, cap=65536)], {}),
             ("cap -1", one, [r0.record(api, cap=-1)], {}), ("null xyz with cap", one, [r0.record(api, xyz=None)], {}),
             ("null feat with cap", one, [r0.record(api, feat=None)], {}), ("pixel 2 bytes off", one, [r0.record(api, pixel=r0.t["pixel"].data_ptr() + 2)], {}),
             ("depth too short", one, [r0.record(api, depth=short.value)], {}),
             ("index too short", one, [r0.record(api, index=short.value)], {}),
             ("map too short", one, [r0.record(api, map=short.value)], {}),
             ("relation without observed", one, recs[:1], {}),
             ("observed depth16 null", one, [no_relation.record(api)], dict(observed=[api.DeviceImage(None, None, 0, 0, 3, 0)])),
             ("observed depth16 odd", one, [no_relation.record(api)], dict(observed=[api.DeviceImage(None, d_obs.data_ptr() + 1, 0, 0, 3, 0)])),
             ("observed pitch below the row", one, [no_relation.record(api)], dict(observed=[depth_image(api, d_obs, 126)])),
             ("observed pitch odd", one, [no_relation.record(api)], dict(observed=[depth_image(api, d_obs, 129)])),
             ("observed rows outside the allocation", one, [no_relation.record(api)], dict(observed=[api.DeviceImage(None, short.value, 0, 0, 3, 0)])),
             ("observed pageable", one, [no_relation.record(api)], dict(observed=[api.DeviceImage(None, host_obs.ctypes.data, 0, 0, 3, 0)]))]
    torch.cuda.synchronize()
    msg = lambda: api.load_library().cvo_last_error().decode()
    for what, views, out, kw in cases:
        kw = dict(kw)
        cams = kw.pop("cams", [cam])
        if "observed" not in kw and what != "relation without observed":
            out = [api.ViewedCloud(o.xyz, o.feat, o.source, o.pixel, None, o.map, o.depth, o.index, o.cap, 0) for o in out]   # (relation needs observed)
        for check_only in (True, False):
            rc, n_out, counts = raw_view(hiplib, reducer, views, out, cams, check_only=check_only, **kw)
            assert rc == INVALID, what
            assert msg(), what
            assert (n_out == -7).all() and (counts == -7).all(), what
        torch.cuda.synchronize()
        assert all(r.untouched() for r in raws) and no_relation.untouched(), what
        assert (host_out == 0x5A).all(), what
    # the messages name view and field
    raw_view(hiplib, reducer, [good, too_big], [api.ViewedCloud()] * 2, [cam])
    assert "view 1" in msg() and "n 32769" in msg()
    raw_view(hiplib, reducer, [good, good, posed(7, nan)], [api.ViewedCloud()] * 3, [cam])
    assert "view 2" in msg() and "pose[7]" in msg()
    raw_view(hiplib, reducer, [good, good], [api.ViewedCloud(), r0.record(api, relation=None, pixel=r0.t["pixel"].data_ptr() + 2)], [cam])
    assert "view 1" in msg() and "pixel" in msg() and "4-byte" in msg()
    raw_view(hiplib, reducer, [good], [api.ViewedCloud()], [cam], observed=[api.DeviceImage(None, short.value, 0, 0, 3, 0)])
    assert "view 0" in msg() and "observed depth16" in msg()
    rc, n_out, counts = raw_view(hiplib, reducer, [good], [api.ViewedCloud()], [cam], size=(64, 47), observed=[api.DeviceImage(None, short.value, 0, 0, 3, 0)], check_only=True)
    assert rc == 0, msg()                                              # 47 rows end where the allocation ends
    hip.hipFree(short)
    raw_view(hiplib, reducer, [good], [api.ViewedCloud()], [cam], cell=17)
    assert "cell 17" in msg()
    # python refuses what it can before the library; the library's refusals come up as CvoError
    with pytest.raises(hiplib.CvoError, match="z-cells"):
        reducer.check_view([tens], [EYE], cam, (256, 256))
    reducer.check_view([tens], [EYE], cam, (64, 48), observed=[d_obs])
    # and the reducer works after all that, with the scratch it had
    same(reducer.view([tens], [S["poses"][0]], cam, (64, 48), want=WANT)[0], want)
    assert reducer.scratch_bytes() == scratch_before == 8 * 32768 * 384


# ---- 6. stream rule
def test_cloud_stream_orders_input_and_output(hiplib, torch, reducer, scenes):
    S = scenes["small"]
    w, h = S["size"]
    x, f = S["clouds"][3000]
    obs = S["observed"][0][6]
    want = vw.view_reading((x, f), S["poses"][6], S["camera"], vw.params(w, h, 2, vw.SURFACE, 0.05), obs)
    side = torch.cuda.Stream()
    hx, hf, ho = torch.from_numpy(x).pin_memory(), torch.from_numpy(f).pin_memory(), torch.from_numpy(obs.view(np.int16)).pin_memory()
    tx = torch.full(x.shape, 1000.0, dtype=torch.float32, device="cuda"); tf = torch.zeros(f.shape, dtype=torch.float32, device="cuda")
    to = torch.zeros(obs.shape, dtype=torch.int16, device="cuda")
    a = torch.randn((4096, 4096), device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):                                             # work in front of the writes: without the edge in, the kernel would read the 1000s
            a = a @ a * 1e-3
        tx.copy_(hx, non_blocking=True); tf.copy_(hf, non_blocking=True); to.copy_(ho, non_blocking=True)
    got = reducer.view([(tx, tf, "points_first")], [S["poses"][6]], S["camera"], (w, h), 2, "surface", 0.05, observed=[to], want=ALL, stream=side)[0]
    with torch.cuda.stream(side):                                      # a read queued on that stream behind the call, and an overwrite behind the read
        snap = {k: got[k].clone() for k in KEYS + ("relation",)}
        tx.fill_(-3.0); to.zero_()
        for k in KEYS + ("relation",):
            got[k].zero_()
    side.synchronize()
    same(dict(snap, n_out=got["n_out"], relation_counts=got["relation_counts"]), want, "side stream", KEYS + ("relation",))


# ---- 7. one reducer
def test_reduce_fuse_and_view_on_one_reducer(hiplib, torch, reducer, scenes):
    S = scenes["wide"]
    w, h = S["size"]
    members, poses = fr.windows(np.random.default_rng(12))
    tens = [dev(torch, m) for m in members]
    before = reducer.scratch_bytes()
    def view_is_its_reading(cell, mode, slack):
        got = reducer.view([S["tens"][3000], S["tens"][257]], S["poses"][:2], S["camera"], (w, h), cell, mode, slack, want=WANT)
        for g, n, pose in zip(got, (3000, 257), S["poses"]):
            same(g, vw.view_reading(S["clouds"][n], pose, S["camera"], vw.params(w, h, cell, mode_of(mode), slack)), (cell, mode, n))
    view_is_its_reading(1, "front", 0.0)
    got = reducer.reduce(tens, 0.05, "mean", 1, want=("count", "source", "map"))
    for g, (x, f) in zip(got, members):
        r = vr.reduce_reading(x, f, 0.05, "mean", 1)
        assert g["n_out"] == r["n_out"] and all(host(g[k]).tobytes() == r[k].tobytes() for k in ("xyz", "feat", "count", "source", "map"))
    view_is_its_reading(3, "surface", 0.05)
    fused = reducer.fuse([tens], [poses], 0.05, "central", 1, 2, want=("count", "source", "map", "views", "view_mask"))[0]
    r = fr.fuse_reading(members, poses, 0.05, "central", 1, 2)
    assert fused["n_out"] == r["n_out"] and all(host(fused[k]).tobytes() == r[k].tobytes() for k in ("xyz", "feat", "count", "source", "map", "views"))
    view_is_its_reading(16, "surface", 0.0)
    assert reducer.scratch_bytes() == before


# ---- 8. end to end
def test_a_viewed_map_aligns_like_the_reading_s_rows(hiplib, torch):
    from cvo_slam_amd import synth
    from cvo_slam_amd.voxels import lift, view_cell_for_budget
    frames, cam_poses = synth.make_sequence(0, 5)
    clouds = []
    for bgr, dep in frames:
        c = synth.dense_cloud(bgr, dep, synth.TUM1)
        pick = np.unique(np.linspace(0, c.n - 1, 5000).astype(np.int64))
        clouds.append((np.ascontiguousarray(c.xyz[pick]), np.ascontiguousarray(c.feat[:, pick].T)))
    window, newest = clouds[:4], 3
    poses = [(np.linalg.inv(cam_poses[newest]) @ cam_poses[k]).astype(np.float32) for k in range(4)]   # keyframe k in the newest keyframe's frame
    T = synth.TUM1
    cam = (T["depth_factor"], T["fx"], T["fy"], T["cx"], T["cy"])
    R = hiplib.CvoReducer(2, 20000)
    tens = [dev(torch, m) for m in window]
    fused = R.fuse([tens], [poses], 0.02, "mean", 1, 1, want=("map",))[0]           # the window's local map, in the newest keyframe's frame
    fmap = fr.fuse_reading(window, poses, 0.02, "mean", 1, 1)
    assert fused["n_out"] == fmap["n_out"] and host(fused["xyz"]).tobytes() == fmap["xyz"].tobytes() and host(fused["feat"]).tobytes() == fmap["feat"].tobytes()
    # the view of the map from where frame 4 is predicted to be: the newest keyframe's frame moved into camera 4's
    predicted = (np.linalg.inv(cam_poses[4]) @ cam_poses[newest]).astype(np.float32)
    cell = view_cell_for_budget(T["w"], T["h"], 3072)
    got = R.view([(fused["xyz"], fused["feat"], "points_first")], [predicted], cam, (T["w"], T["h"]), cell, "front", want=("source", "pixel", "map"))[0]
    want = vw.view_reading((fmap["xyz"], fmap["feat"]), predicted, cam, vw.params(T["w"], T["h"], cell, vw.FRONT))
    same(got, want, "viewed map", ("xyz", "feat", "source", "pixel", "map"))
    assert 300 < want["n_out"] <= 3072 and want["n_out"] < fmap["n_out"] and (want["map"] == -1).any()
    moving = R.reduce([dev(torch, clouds[4])], 0.05, "mean", 1, want=())[0]
    mw = vr.reduce_reading(clouds[4][0], clouds[4][1], 0.05, "mean", 1)
    B = hiplib.CvoBatch(1)
    B.set_pairs_clouds([(got["xyz"], got["feat"], "points_first"), (moving["xyz"], moving["feat"], "points_first")], [0], [1])   # the viewed rows as they are
    B.align_async(1)
    res = B.wait(1)[0]
    Bh = hiplib.CvoBatch(1)
    Bh.set_pairs([(want["xyz"], np.ascontiguousarray(want["feat"].T), mw["xyz"], np.ascontiguousarray(mw["feat"].T))])
    ref = Bh.align(1)[0]
    assert res["status"] == 0 and ref["status"] == 0
    assert res["transform"].tobytes() == ref["transform"].tobytes() and res["ell"] == ref["ell"] and res["iter"] == ref["iter"]
    # per-row support of the viewed map back to the map's rows, and through the fusion's map to the window's dense points
    sup = B.point_support([0])[0]
    on_map = lift(host(got["map"]), sup["sum_fixed"], -1.0)
    assert on_map.shape == (fmap["n_out"],) and np.array_equal(on_map == -1.0, want["map"] < 0)
    B.close(); Bh.close(); R.close()
