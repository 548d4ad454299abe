"""Fusing posed device clouds (cvo_fuse_device_clouds, CvoReducer.fuse) against the numpy reading of its definition (tests/fuse_reading.py).
Every comparison with the reading is exact, on bytes: positions, features, counts, sources, views, view masks, maps and row counts."""
import ctypes as C

import numpy as np
import pytest

import fuse_reading as fr
import voxel_reading as vr

pytestmark = pytest.mark.gpu

INVALID = 4
KEYS = ("xyz", "feat", "count", "source", "views", "view_mask", "map")
WANT = ("count", "source", "map", "views", "view_mask")
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 3000)
EYE = np.eye(4, dtype=np.float32)


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
def four():
    """groups of 1, 2, 5 and 64 members with sizes from SIZES -- empty members, wave edges and block edges -- on a noisy sheet, under poses that
    bring every moved coordinate into (0, 10): one 64 m voxel holds a whole group, and at 1e-5 m the cell coordinates stay below 2^20"""
    rng = np.random.default_rng(11)
    sizes = [[3000], [0, 65], [256, 1, 0, 63, 3000], [SIZES[k % 8] for k in range(64)]]
    sizes[3][5] = 3000; sizes[3][40] = 3000
    assert sizes[3][63] > 0 and sizes[3][0] == 0 and set(n for g in sizes for n in g) == set(SIZES)
    groups, poses = [], []
    for g in sizes:
        assert sum(g) <= 20000
        groups.append([fr.surface(rng, n, 0.01) for n in g])
        ps = []
        for _ in g:
            P = fr.rigid(rng, 0.1, 0.2); P[:2, 3] += np.float32(4.0); ps.append(P)
        poses.append(ps)
    return groups, poses


@pytest.fixture(scope="module")
def seen_four_times():
    return fr.windows(np.random.default_rng(12))


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev(torch, members):
    return [(up(torch, x), up(torch, f), "points_first") for x, f in members]


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else t


def same(got, want, what="", keys=KEYS):
    assert got["n_out"] == want["n_out"], (what, got["n_out"], want["n_out"])
    for key in keys:
        g = host(got[key])
        if key == "view_mask":
            g = g.view(np.uint64)                                      # (torch carries the 64 bits as int64)
        assert g.dtype == want[key].dtype and g.shape == want[key].shape, (what, key, g.dtype, g.shape, want[key].shape)
        assert g.tobytes() == want[key].tobytes(), (what, key)
    assert np.array_equal(got["offsets"], want["offsets"]), what


# ---- 1. boundaries
@pytest.mark.parametrize("voxel", [0.05, 0.5, 64.0, 1e-5], ids=["5cm", "50cm", "one_cell", "own_cells"])
def test_boundaries_one_call_many_groups(hiplib, torch, reducer, four, voxel):
    groups, poses = four
    tens = [dev(torch, g) for g in groups]
    for mode in ("mean", "central"):
        got = reducer.fuse(tens, poses, voxel, mode, want=WANT)
        assert len(got) == 4
        for k, (g, ps) in enumerate(zip(groups, poses)):
            want = fr.fuse_reading(g, ps, voxel, mode)
            same(got[k], want, (voxel, mode, k))
            total = sum(x.shape[0] for x, f in g)
            if voxel == 64.0:                                          # every point of the group in one row, every nonempty member a view
                assert want["n_out"] == 1 and want["count"].tolist() == [total]
                assert int(want["view_mask"][0]) == sum(1 << m for m, (x, f) in enumerate(g) if x.shape[0])
                assert k != 3 or int(want["view_mask"][0]) >> 63 == 1   # bit 63 is real
            if voxel == 1e-5:                                          # as many cells as points: the table at its fullest
                assert want["n_out"] == total and (want["views"] == 1).all()


# ---- 2. filters
@pytest.mark.parametrize("mode", ["mean", "central"])
def test_filters_min_points_and_min_views(hiplib, torch, reducer, seen_four_times, mode):
    members, poses = seen_four_times
    tens = dev(torch, members)
    free = fr.fuse_reading(members, poses, 0.05, mode, 1, 1)
    assert (free["views"] == 1).sum() > 50 and (free["views"] >= 2).sum() > 50 and (free["views"] == 4).sum() > 0   # one view and several both exist
    assert (free["count"] == 1).sum() > 50 and (free["count"] >= 2).sum() > 50
    n_outs = {}
    for min_points in (1, 2):
        for min_views in (1, 2, 4):
            want = fr.fuse_reading(members, poses, 0.05, mode, min_points, min_views)
            got = reducer.fuse([tens], [poses], 0.05, mode, min_points, min_views, want=WANT)[0]
            same(got, want, (mode, min_points, min_views))
            assert (want["map"] == -1).any() == (min_points > 1 or min_views > 1) and want["n_out"] > 0
            n_outs[min_points, min_views] = want["n_out"]
    assert n_outs[1, 1] > n_outs[2, 1] > n_outs[2, 2] > n_outs[2, 4]   # each filter bites; two views are two points, so
    assert n_outs[1, 2] == n_outs[2, 2] and n_outs[1, 4] == n_outs[2, 4]


# ---- 3. bad floats, far moves, faces
@pytest.mark.parametrize("mode", ["mean", "central"])
def test_bad_floats_far_moves_negative_coordinates_and_faces(hiplib, torch, reducer, mode):
    rng = np.random.default_rng(13)
    v = np.float32(0.25)
    x, f = fr.surface(rng, 600, 0.01)
    P = np.concatenate([x, f], axis=1)
    bad = []
    for j, val in enumerate([np.nan, np.inf, -np.inf, 32768.0, -40000.0]):    # one bad float in each of the 8 places
        for k in range(8):
            P[200 + 8 * j + k, k] = val; bad.append(200 + 8 * j + k)
    x, f = np.ascontiguousarray(P[:, :3]), np.ascontiguousarray(P[:, 3:])
    # points on cell faces after an exact move (multiples of the voxel, moved by multiples of it), at negative coordinates too
    special = np.array([0.0, v, -v, 2 * v, -2 * v, 3 * v, np.nextafter(-v, np.float32(-1)), np.nextafter(v, np.float32(0)), 5 * v, -7 * v], np.float32)
    y = rng.uniform(-1.0, 1.0, (300, 3)).astype(np.float32)
    for axis in range(3):
        y[axis * 10:axis * 10 + 10, axis] = special
    y[30:40] = special[:, None]
    y[40:100, 0] = rng.integers(-4, 5, 60).astype(np.float32) * v
    fy = rng.uniform(0, 255, (300, 5)).astype(np.float32)
    onto_faces = EYE.copy(); onto_faces[:3, 3] = (-0.5, 0.25, -1.0)
    past_2_15 = EYE.copy(); past_2_15[0, 3] = 32767.5                  # x' >= 2^15 for x >= 0.5
    past_2_20 = EYE.copy(); past_2_20[1, 3] = 10485.0                  # at voxel 0.01 cell y' >= 2^20 for y >= 0.76
    zero_row = EYE.copy(); zero_row[0, 0] = 0.0                        # 0 * 40000 = 0: the source float must be refused on its own
    members = [(x, f), (y, fy), (x, f), (x, f), (x, f)]
    poses = [EYE, onto_faces, past_2_15, past_2_20, zero_row]
    tens = dev(torch, members)
    for voxel in (0.25, 0.01):
        want = fr.fuse_reading(members, poses, voxel, mode)
        got = reducer.fuse([tens], [poses], voxel, mode, want=WANT)[0]  # (the call does not fail)
        same(got, want, (mode, voxel))
        off = want["offsets"]; m = want["map"]
        for k in (0, 2, 3, 4):
            assert (m[off[k] + np.array(bad)] == -1).all(), k
        ok = np.setdiff1d(np.arange(600), bad)
        assert (m[ok] >= 0).all() and (m[off[1]:off[2]] >= 0).all()
        def invalid(col, shift):                                       # past 2^15, or its cell past 2^20
            moved = col + np.float32(shift)
            return (moved >= 32768.0) | (np.floor(moved / np.float32(voxel)) >= 1048576.0)
        far = m[off[2]:off[3]][ok]
        assert np.array_equal(far == -1, invalid(x[ok, 0], 32767.5))
        assert voxel != 0.25 or ((far == -1).any() and (far >= 0).any())          # (at 0.01 every cell of that member is past 2^20)
        cells = m[off[3]:off[4]][ok]
        assert np.array_equal(cells == -1, invalid(x[ok, 1], 10485.0))
        assert ((cells == -1).any() and (cells >= 0).any()) if voxel == 0.01 else (cells >= 0).all()
        assert np.isfinite(want["xyz"]).all() and np.isfinite(want["feat"]).all() and (want["xyz"] < 0).any()
    # the face points of member 1 (0, -voxel and 2 voxel in all three coordinates) land on faces of three different cells
    w = fr.fuse_reading([(y, fy)], [onto_faces], 0.25, mode)
    assert len({w["map"][30], w["map"][32], w["map"][33]}) == 3


# ---- 4. one call against many; repeats
@pytest.mark.parametrize("mode", ["mean", "central"])
def test_one_call_of_many_groups_is_many_calls_of_one(hiplib, torch, reducer, four, mode):
    groups, poses = four
    tens = [dev(torch, g) for g in groups]
    clone = lambda run: [{k: (v.clone() if hasattr(v, "clone") else v) for k, v in g.items()} for g in run]
    first = clone(reducer.fuse(tens, poses, 0.05, mode, 1, 1, want=WANT))
    for _ in range(2):
        again = reducer.fuse(tens, poses, 0.05, mode, 1, 1, want=WANT)
        for a, b in zip(again, first):
            assert a["n_out"] == b["n_out"] and all(torch.equal(a[k], b[k]) for k in KEYS)
    for k in range(4):
        alone = reducer.fuse([tens[k]], [poses[k]], 0.05, mode, 1, 1, want=WANT)[0]
        assert alone["n_out"] == first[k]["n_out"] and all(torch.equal(alone[key], first[k][key]) for key in KEYS)


# ---- 5. layouts
def test_layouts_give_the_tight_copy_s_bytes(hiplib, torch, reducer, seen_four_times):
    members, poses = seen_four_times
    rng = np.random.default_rng(2)
    tight = dev(torch, members)
    other = []
    for k, (x, f) in enumerate(members):
        n = x.shape[0]
        if k == 0:                                                     # float4 points (stride 16), channel-major features
            other.append((up(torch, np.concatenate([x, rng.normal(size=(n, 1)).astype(np.float32)], axis=1))[:, :3], up(torch, f.T), "channels_first"))
        elif k == 1:                                                   # columns 2 .. 4 of an (n, 8) tensor, features every other row of a (2 n, 5) one
            big = rng.normal(size=(n, 8)).astype(np.float32); big[:, 2:5] = x
            ff = rng.normal(size=(2 * n, 5)).astype(np.float32); ff[::2] = f
            other.append((up(torch, big)[:, 2:5], up(torch, ff)[::2], "points_first"))
        elif k == 2:                                                   # both arrays 4 bytes past a 16-byte boundary
            bx = rng.normal(size=3 * n + 1).astype(np.float32); bx[1:] = x.reshape(-1)
            bf = rng.normal(size=5 * n + 1).astype(np.float32); bf[1:] = f.reshape(-1)
            other.append((up(torch, bx)[1:].view(n, 3), up(torch, bf)[1:].view(n, 5), "points_first"))
        else:
            other.append((tight[k][0], up(torch, f.T), "channels_first"))
    d = [hiplib.api.device_cloud(*c) for c in other]
    assert [q.xyz_stride for q in d] == [16, 32, 12, 12] and [q.feat_point_stride for q in d] == [4, 40, 20, 4]
    for mode in ("mean", "central"):
        want = fr.fuse_reading(members, poses, 0.05, mode, 1, 2)
        got = reducer.fuse([tight, other], [poses, poses], 0.05, mode, 1, 2, want=WANT)
        same(got[0], want, (mode, "tight")); same(got[1], want, (mode, "layouts"))


# ---- the C ABI itself, with arrays of the test's own
class Raw:
    """one group's output arrays as byte tensors prefilled with 0xA5, each with 64 guard bytes behind its cap rows"""
    G = 64
    ROW = dict(xyz=12, feat=20, count=4, source=4, views=4, view_mask=8)

    def __init__(self, torch, cap, n_in, arrays=KEYS):
        self.cap = cap
        self.sizes = {k: b * cap for k, b in self.ROW.items()} | dict(map=4 * n_in)
        self.t = {k: torch.full((self.sizes[k] + self.G,), 0xA5, dtype=torch.uint8, device="cuda") for k in arrays}

    def record(self, api, **over):
        p = lambda k: over[k] if k in over else (self.t[k].data_ptr() if k in self.t else None)
        return api.FusedCloud(p("xyz"), p("feat"), p("count"), p("source"), p("map"), p("views"), p("view_mask"), over.get("cap", self.cap), 0)

    def host(self, key, dtype):
        return self.t[key].cpu().numpy()[:self.sizes[key]].view(dtype)

    def guards_intact(self):
        return all((t.cpu().numpy()[self.sizes[k]:] == 0xA5).all() for k, t in self.t.items())

    def untouched(self):
        return all((t.cpu().numpy() == 0xA5).all() for t in self.t.values())


def member(api, tens, pose):
    d = tens if isinstance(tens, api.DeviceCloud) else api.device_cloud(*tens, max_n=api.REDUCE_MAX_POINTS)
    return api.FuseMember(d, (C.c_float * 12)(*np.asarray(pose, np.float32)[:3].reshape(-1).tolist()))


def raw_fuse(hiplib, R, group_first, members, recs, voxel=0.05, mode=0, min_points=1, min_views=1, stream=None, groups=None, check_only=False):
    api = hiplib.api
    first = np.asarray(group_first, np.int32)
    groups = len(group_first) - 1 if groups is None else groups
    arr = (api.FuseMember * max(1, len(members)))(*members); out = (api.FusedCloud * max(1, len(recs)))(*recs)
    prm = api.FuseParams(voxel, mode, min_points, min_views)
    n_out = np.full(max(1, groups), -7, np.int32)
    ip = C.POINTER(C.c_int)
    if check_only:
        return R.L.cvo_check_fuse_clouds(R.h, groups, first.ctypes.data_as(ip), arr, C.byref(prm), out), n_out
    rc = R.L.cvo_fuse_device_clouds(R.h, groups, first.ctypes.data_as(ip), arr, C.byref(prm), out, n_out.ctypes.data_as(ip), stream)
    return rc, n_out


# ---- 6. cap
@pytest.mark.parametrize("mode", [0, 1])
def test_cap_below_the_row_count(hiplib, torch, reducer, four, seen_four_times, mode):
    api = hiplib.api
    groups = [seen_four_times[0], four[0][2]]; poses = [seen_four_times[1], four[1][2]]
    tens = [dev(torch, g) for g in groups]
    mem = [member(api, t, p) for g, ps in zip(tens, poses) for t, p in zip(g, ps)]
    first = [0, len(groups[0]), len(groups[0]) + len(groups[1])]
    want = [fr.fuse_reading(g, ps, 0.05, mode) for g, ps in zip(groups, poses)]
    caps = [100, 7]
    assert all(w["n_out"] > c for w, c in zip(want, caps))
    raws = [Raw(torch, c, w["map"].shape[0]) for c, w in zip(caps, want)]
    torch.cuda.synchronize()
    rc, n_out = raw_fuse(hiplib, reducer, first, mem, [r.record(api) for r in raws], 0.05, mode)
    assert rc == 0, api.load_library().cvo_last_error()
    torch.cuda.synchronize()
    for k, (r, w) in enumerate(zip(raws, want)):
        c = caps[k]
        assert n_out[k] == w["n_out"]                                  # the full row count
        for key, dt in (("xyz", np.float32), ("feat", np.float32), ("count", np.int32), ("source", np.int32), ("views", np.int32), ("view_mask", np.uint64)):
            assert r.host(key, dt).tobytes() == w[key][:c].tobytes(), (k, key)
        assert r.host("map", np.int32).tobytes() == w["map"].tobytes()  # full row numbers
        assert r.guards_intact()
    with pytest.raises(hiplib.CvoError, match="cap 100"):
        reducer.fuse(tens, poses, 0.05, mode, cap=100)
    # cap = 0 with every array NULL counts only, through the ABI and through fuse
    rc, n_out = raw_fuse(hiplib, reducer, first, mem, [api.FusedCloud(None, None, None, None, None, None, None, 0, 0)] * 2, 0.05, mode)
    assert rc == 0 and n_out.tolist() == [w["n_out"] for w in want]
    counted = reducer.fuse(tens, poses, 0.05, mode, cap=0, want=())
    assert [g["n_out"] for g in counted] == [w["n_out"] for w in want] and all(g["xyz"].shape[0] == 0 for g in counted)


# ---- 7. refusals
def test_refusals_change_nothing(hiplib, torch, reducer, seen_four_times):
    api = hiplib.api
    members, poses = seen_four_times
    tens = dev(torch, members)
    good = [member(api, t, p) for t, p in zip(tens, poses)]
    n = sum(x.shape[0] for x, f in members)
    want = fr.fuse_reading(members, poses, 0.05, 0)
    scratch_before = reducer.scratch_bytes()
    raws = [Raw(torch, 300, 40000) for _ in range(9)]
    recs = [r.record(api) for r in raws]
    bigx = torch.zeros((32769, 3), dtype=torch.float32, device="cuda"); bigf = torch.zeros((32769, 5), dtype=torch.float32, device="cuda")
    too_big = member(api, (bigx, bigf, "points_first"), EYE)
    half = member(api, (bigx[:20000], bigf[:20000], "points_first"), EYE)     # two of them: each fits, the group does not
    host_x = np.zeros((100, 3), np.float32)                              # pageable host memory
    pageable = api.FuseMember(api.DeviceCloud(host_x.ctypes.data, good[0].cloud.feat, 12, 20, 4, 100, 0), good[0].pose)
    odd_stride = api.FuseMember(api.DeviceCloud(good[0].cloud.xyz, good[0].cloud.feat, 14, 20, 4, 100, 0), good[0].pose)
    def posed(k, val):
        m = api.FuseMember(good[1].cloud, good[1].pose); m.pose[k] = val; return m
    host_out = np.full(12 * 300, 0x5A, np.uint8)
    one = [0, 4]
    cases = [("voxel 0", one, good, recs[:1], dict(voxel=0.0)), ("voxel negative", one, good, recs[:1], dict(voxel=-0.05)), ("voxel NaN", one, good, recs[:1], dict(voxel=float("nan"))),
             ("voxel inf", one, good, recs[:1], dict(voxel=float("inf"))), ("mode 2", one, good, recs[:1], dict(mode=2)), ("min_points 0", one, good, recs[:1], dict(min_points=0)),
             ("min_views 0", one, good, recs[:1], dict(min_views=0)), ("min_views 65", one, good, recs[:1], dict(min_views=65)),
             ("group_first from 1", [1, 4], good, recs[:1], {}), ("group_first descending", [0, 3, 2], good, recs[:2], {}),
             ("a group with no members", [0, 2, 2, 4], good, recs[:3], {}), ("65 members", [0, 65], [good[0]] * 65, recs[:1], {}),
             ("groups 0", [0], good, recs[:1], dict(groups=0)), ("groups 9", list(range(10)), [good[0]] * 9, recs, {}),
             ("member n > max_points", [0, 2], [good[0], too_big], recs[:1], {}), ("group total > max_points", [0, 2], [half, half], recs[:1], {}),
             ("pageable input", [0, 2], [good[0], pageable], recs[:1], {}), ("stride 14", [0, 2], [good[0], odd_stride], recs[:1], {}),
             ("pose NaN", one, [good[0], posed(7, float("nan")), good[2], good[3]], recs[:1], {}), ("pose inf", one, [good[0], posed(0, float("inf")), good[2], good[3]], recs[:1], {}),
             ("pageable output", one, good, [raws[0].record(api, xyz=host_out.ctypes.data)], {}), ("cap 65536", one, good, [raws[0].record(api, cap=65536)], {}),
             ("cap -1", one, good, [raws[0].record(api, cap=-1)], {}), ("null xyz with cap", one, good, [raws[0].record(api, xyz=None)], {}),
             ("null feat with cap", one, good, [raws[0].record(api, feat=None)], {}),
             ("view_mask 4 bytes off", one, good, [raws[0].record(api, view_mask=raws[0].t["view_mask"].data_ptr() + 4)], {}),
             ("count 2 bytes off", one, good, [raws[0].record(api, count=raws[0].t["count"].data_ptr() + 2)], {})]
    assert n <= 40000
    torch.cuda.synchronize()
    msg = lambda: api.load_library().cvo_last_error().decode()
    for what, first, mem, out, kw in cases:
        for check_only in (True, False):
            rc, n_out = raw_fuse(hiplib, reducer, first, mem, out, check_only=check_only, **kw)
            assert rc == INVALID, what
            assert msg(), what
            assert (n_out == -7).all(), what
        torch.cuda.synchronize()
        assert all(r.untouched() for r in raws), what
        assert (host_out == 0x5A).all(), what
    # the messages name group, member and field
    raw_fuse(hiplib, reducer, [0, 1, 3], [good[0], good[1], too_big], recs[:2])
    assert "group 1 member 1" in msg() and "n 32769" in msg()
    raw_fuse(hiplib, reducer, [0, 1, 4], [good[0], good[0], good[1], posed(7, float("nan"))], recs[:2])
    assert "group 1 member 2" in msg() and "pose[7]" in msg()
    raw_fuse(hiplib, reducer, [0, 1, 2], [good[0], good[1]], [recs[0], raws[1].record(api, view_mask=raws[1].t["view_mask"].data_ptr() + 4)])
    assert "group 1" in msg() and "view_mask" in msg() and "8-byte" in msg()
    # more than 4096 members in a call: 65 groups of 64, on a reducer that takes 70 groups
    wide = hiplib.CvoReducer(70, 256)
    tiny = member(api, (bigx[:4], bigf[:4], "points_first"), EYE)
    rc, n_out = raw_fuse(hiplib, wide, [64 * g for g in range(66)], [tiny] * (64 * 65), [api.FusedCloud(None, None, None, None, None, None, None, 0, 0)] * 65)
    assert rc == INVALID and "4096" in msg() and (n_out == -7).all()
    rc, n_out = raw_fuse(hiplib, wide, [64 * g for g in range(65)], [tiny] * (64 * 64), [api.FusedCloud(None, None, None, None, None, None, None, 0, 0)] * 64, voxel=64.0)
    assert rc == 0 and (n_out == 1).all()                               # exactly 4096 members go through
    wide.close()
    # and the reducer works after all that, with the scratch it had
    same(reducer.fuse([tens], [poses], 0.05, want=WANT)[0], want)
    assert reducer.scratch_bytes() == scratch_before == 8 * 32768 * 384


# ---- 8. stream rule
def test_cloud_stream_orders_input_and_output(hiplib, torch, reducer, seen_four_times):
    members, poses = seen_four_times
    want = fr.fuse_reading(members, poses, 0.05, 0, 1, 2)
    side = torch.cuda.Stream()
    pinned = [(torch.from_numpy(x).pin_memory(), torch.from_numpy(f).pin_memory()) for x, f in members]
    tens = [(torch.full(x.shape, 1000.0, dtype=torch.float32, device="cuda"), torch.zeros(f.shape, dtype=torch.float32, device="cuda"), "points_first") for x, f in members]
    a = torch.randn((4096, 4096), device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):                                             # work in front of the writes: without the edge in, the kernel would read the 1000s
            a = a @ a * 1e-3
        for (tx, tf, _), (hx, hf) in zip(tens, pinned):
            tx.copy_(hx, non_blocking=True); tf.copy_(hf, non_blocking=True)
    got = reducer.fuse([tens], [poses], 0.05, "mean", 1, 2, want=WANT, cloud_stream=side)[0]
    with torch.cuda.stream(side):                                      # a read queued on that stream behind the call, and an overwrite behind the read
        snap = {k: got[k].clone() for k in KEYS}
        for tx, tf, _ in tens:
            tx.fill_(-3.0)
        for k in KEYS:
            got[k].zero_()
    side.synchronize()
    same(dict(snap, n_out=got["n_out"], offsets=got["offsets"]), want)


# ---- 9. coexistence
def test_reduce_fuse_reduce_on_one_reducer(hiplib, torch, reducer, seen_four_times):
    members, poses = seen_four_times
    tens = dev(torch, members)
    rkeys = ("xyz", "feat", "count", "source", "map")
    def reduce_is_its_reading(mode):
        got = reducer.reduce(tens, 0.05, mode, 1, want=("count", "source", "map"))
        for g, (x, f) in zip(got, members):
            w = vr.reduce_reading(x, f, 0.05, mode, 1)
            assert g["n_out"] == w["n_out"] and all(host(g[k]).tobytes() == w[k].tobytes() for k in rkeys)
    before = reducer.scratch_bytes()
    reduce_is_its_reading("mean")
    same(reducer.fuse([tens, tens[:2]], [poses, poses[:2]], 0.05, "central", 1, 2, want=WANT)[0], fr.fuse_reading(members, poses, 0.05, "central", 1, 2))
    reduce_is_its_reading("central")
    counts = reducer.count_voxels(tens, [0.05, 0.5])
    assert counts[:, 0].tolist() == [vr.count_reading(x, f, 0.05) for x, f in members]
    same(reducer.fuse([tens], [poses], 0.05, "mean", 2, 1, want=WANT)[0], fr.fuse_reading(members, poses, 0.05, "mean", 2, 1))
    assert reducer.scratch_bytes() == before


# ---- 10. the two kernel families share their passes
@pytest.mark.parametrize("mode", ["mean", "central"])
def test_one_member_under_the_identity_is_the_reduction(hiplib, torch, reducer, mode):
    """groups of one member under the identity pose, one fusion for all of them, against one reduction of the same clouds: the same bytes
    (tests/test_fuse_reading.py holds the two readings to the same on these clouds)"""
    clouds = fr.lone_clouds()
    assert tuple(x.shape[0] for x, f in clouds) == (1, 63, 64, 65, 255, 256, 257, 3000)
    for x, f in clouds:
        assert not (np.signbit(x) & (x == 0)).any()                    # an identity move would make a -0.0 a +0.0
    tens = dev(torch, clouds)
    fused = [{k: (host(v).copy() if hasattr(v, "cpu") else v) for k, v in g.items()}
             for g in reducer.fuse([[t] for t in tens], [[EYE]] * len(tens), 0.05, mode, want=WANT)]
    reduced = reducer.reduce(tens, 0.05, mode, 1, want=("count", "source", "map"))
    assert len(fused) == len(reduced) == len(clouds)
    for (x, f), a, b in zip(clouds, fused, reduced):
        n = x.shape[0]
        assert a["n_out"] == b["n_out"] >= 1, n
        for key in ("xyz", "feat", "count", "source", "map"):
            want = host(b[key])
            assert a[key].dtype == want.dtype and a[key].shape == want.shape and a[key].tobytes() == want.tobytes(), (n, key)
        assert a["map"].shape == (n,) and (a["views"] == 1).all() and (a["view_mask"] == 1).all(), n
    assert fused[-1]["n_out"] > 100


# ---- 11. end to end
def test_a_fused_map_aligns_like_the_reading_s_rows(hiplib, torch):
    from cvo_slam_amd import synth
    from cvo_slam_amd.voxels import fuse_voxel_for_budget, split_source, lift
    frames, cam_poses = synth.make_sequence(0, 5)
    clouds = []
    for bgr, dep in frames:
        c = synth.dense_cloud(bgr, dep, synth.TUM1)
        pick = np.unique(np.linspace(0, c.n - 1, 5000).astype(np.int64))
        clouds.append((np.ascontiguousarray(c.xyz[pick]), np.ascontiguousarray(c.feat[:, pick].T)))
    window, newest = clouds[:4], 3
    poses = [(np.linalg.inv(cam_poses[newest]) @ cam_poses[k]).astype(np.float32) for k in range(4)]   # keyframe k in the newest keyframe's frame
    R = hiplib.CvoReducer(2, 20000)
    tens = dev(torch, window)
    voxel = fuse_voxel_for_budget(R, tens, poses, 3072, 0.005, 1.0)    # (sized without the views filter: see its docstring)
    got = R.fuse([tens], [poses], voxel, "mean", 1, 2, want=WANT)[0]
    want = fr.fuse_reading(window, poses, voxel, "mean", 1, 2)
    same(got, want)
    assert 500 < want["n_out"] <= 3072 and (want["map"] == -1).any()
    member_of, index = split_source(got["source"], got["offsets"])
    assert np.array_equal(want["offsets"][host(member_of)] + host(index), want["source"])
    assert {0} <= set(host(member_of).tolist()) <= {0, 1, 2}           # (a cell with two views never has its lowest member in the last one)
    moving = R.reduce([dev(torch, clouds[4:])[0]], voxel, "mean", 1, want=())[0]
    mw = vr.reduce_reading(clouds[4][0], clouds[4][1], voxel, "mean", 1)
    B = hiplib.CvoBatch(1)
    B.set_pairs_clouds([(got["xyz"], got["feat"], "points_first"), (moving["xyz"], moving["feat"], "points_first")], [0], [1])   # the fused rows as they are
    B.align_async(1)
    res = B.wait(1)[0]
    Bh = hiplib.CvoBatch(1)
    Bh.set_pairs([(want["xyz"], np.ascontiguousarray(want["feat"].T), mw["xyz"], np.ascontiguousarray(mw["feat"].T))])
    ref = Bh.align(1)[0]
    assert res["status"] == 0 and ref["status"] == 0
    assert res["transform"].tobytes() == ref["transform"].tobytes() and res["ell"] == ref["ell"] and res["iter"] == ref["iter"]
    # per-row support of the fused map back to the window's dense points
    sup = B.point_support([0])[0]
    dense = lift(host(got["map"]), sup["sum_fixed"], -1.0)
    assert dense.shape == (20000,) and np.array_equal(dense == -1.0, want["map"] == -1)
    B.close(); Bh.close(); R.close()
