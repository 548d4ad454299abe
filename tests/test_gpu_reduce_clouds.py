"""The cloud reducer (cvo_reducer: cvo_reduce_device_clouds, cvo_count_voxels) against the numpy reading of its definition
(tests/voxel_reading.py).  Every comparison with the reading is exact, on bytes: positions, features, counts, sources, maps and row counts."""
import ctypes as C

import numpy as np
import pytest

import voxel_reading as vr

pytestmark = pytest.mark.gpu

INVALID = 4
SIZES = [0, 1, 2, 255, 257, 4099, 20000]
KEYS = ("xyz", "feat", "count", "source", "map")
WANT = ("count", "source", "map")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def dense():
    """four synthetic frame pairs back-projected densely, 20000 points of each frame spread evenly over the image: [(fixed, moving)] of
    (xyz (n, 3), feat (n, 5))"""
    from cvo_slam_amd import synth
    out = []
    for i in range(4):
        fa, fb, _ = synth.make_frames(i)
        pair = []
        for bgr, dep in (fa, fb):
            c = synth.dense_cloud(bgr, dep, synth.TUM1)
            pick = np.unique(np.linspace(0, c.n - 1, 20000).astype(np.int64))
            assert pick.shape[0] == 20000
            pair.append((np.ascontiguousarray(c.xyz[pick]), np.ascontiguousarray(c.feat[:, pick].T)))
        out.append(tuple(pair))
    return out


@pytest.fixture(scope="module")
def seven(dense):
    """clouds of SIZES points: a scene's points, every third replaced by uniform noise in a 4 m box; all moved into the positive octant, so
    that one large voxel can hold a whole cloud (negative coordinates: the point cases and the permuted cloud below)"""
    rng = np.random.default_rng(77)
    x0, f0 = dense[0][0]
    out = []
    for n in SIZES:
        pick = np.sort(rng.choice(x0.shape[0], n, replace=False))
        x, f = x0[pick].copy(), f0[pick].copy()
        x[2::3] = rng.uniform(-2.0, 2.0, x[2::3].shape).astype(np.float32)
        x[2::3, 2] += np.float32(2.0)
        f[2::3] = rng.uniform(0.0, 255.0, f[2::3].shape).astype(np.float32)
        x[:, :2] += np.float32(4.0)
        assert (x > 0).all() and (x < 8).all()
        out.append((np.ascontiguousarray(x), np.ascontiguousarray(f)))
    return out


@pytest.fixture(scope="module")
def reducer(hiplib):
    R = hiplib.CvoReducer(8, 20000)
    yield R
    R.close()


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev(torch, clouds):
    return [(up(torch, x), up(torch, f), "points_first") for x, f in clouds]


def same(got, want, what=""):
    assert got["n_out"] == want["n_out"], (what, got["n_out"], want["n_out"])
    for key in KEYS:
        g = got[key].cpu().numpy() if hasattr(got[key], "cpu") else got[key]
        assert g.dtype == want[key].dtype and g.shape == want[key].shape, (what, key, g.shape, want[key].shape)
        assert g.tobytes() == want[key].tobytes(), (what, key)


# ---- 1. one call, many clouds
@pytest.mark.parametrize("voxel", [0.05, 0.5, 64.0, 1e-5], ids=["5cm", "50cm", "one_cell", "own_cells"])
def test_one_call_many_clouds(hiplib, torch, reducer, seven, voxel):
    clouds = dev(torch, seven)
    for mode in ("mean", "central"):
        for min_points in (1, 2):
            got = reducer.reduce(clouds, voxel, mode, min_points, want=WANT)
            assert len(got) == len(SIZES)
            for k, (x, f) in enumerate(seven):
                want = vr.reduce_reading(x, f, voxel, mode, min_points)
                same(got[k], want, (voxel, mode, min_points, SIZES[k]))
                if voxel == 64.0:                                      # the contention case: every point of the cloud in one row
                    assert want["n_out"] == (1 if x.shape[0] >= min_points else 0)
                    assert min_points > x.shape[0] or want["count"].tolist() == [x.shape[0]]
                if voxel == 1e-5:                                      # the full-table case: as many cells as points
                    assert want["n_out"] == (x.shape[0] if min_points == 1 else 0)


# ---- 2. layouts
def test_layouts_give_the_tight_copy_s_bytes(hiplib, torch, reducer, seven):
    x, f = seven[5]; n = x.shape[0]
    rng = np.random.default_rng(2)
    tight = (up(torch, x), up(torch, f), "points_first")
    f4 = up(torch, np.concatenate([x, rng.normal(size=(n, 1)).astype(np.float32)], axis=1))             # float4 points: stride 16
    big = rng.normal(size=(n, 8)).astype(np.float32); big[:, 2:5] = x
    wide = up(torch, big)                                                                                # columns 2..4 of an (n, 8) tensor
    fc = up(torch, np.ascontiguousarray(f.T))                                                            # channel-major (5, n)
    bx = rng.normal(size=3 * n + 1).astype(np.float32); bx[1:] = x.reshape(-1)
    bf = rng.normal(size=5 * n + 1).astype(np.float32); bf[1:] = f.reshape(-1)
    ox, of = up(torch, bx), up(torch, bf)
    assert ox.data_ptr() % 16 == 0 and of.data_ptr() % 16 == 0                                           # so the views start 4 bytes past a 16-byte boundary
    clouds = [tight, (f4[:, :3], tight[1], "points_first"), (wide[:, 2:5], fc, "channels_first"), (tight[0], fc, "channels_first"),
              (ox[1:].view(n, 3), of[1:].view(n, 5), "points_first")]
    d = [hiplib.api.device_cloud(*c) for c in clouds]
    assert [q.xyz_stride for q in d] == [12, 16, 32, 12, 12] and [q.feat_point_stride for q in d] == [20, 20, 4, 4, 20]
    assert d[4].xyz % 16 == 4 and d[4].feat % 16 == 4
    for mode in ("mean", "central"):
        want = vr.reduce_reading(x, f, 0.05, mode, 1)
        got = reducer.reduce(clouds, 0.05, mode, 1, want=WANT)
        for k in range(len(clouds)):
            same(got[k], want, (mode, k))


# ---- 3. point cases
def edge_cloud(voxel):
    """points on cell faces and at negative coordinates in every axis, among ordinary ones; then a block of points each with one bad float"""
    v = np.float32(voxel)
    rng = np.random.default_rng(31)
    special = np.array([0.0, -0.0, v, -v, np.nextafter(-v, np.float32(-1)), np.nextafter(v, np.float32(0)), 2 * v, -2 * v, 3 * v,
                        np.nextafter(np.float32(0), np.float32(-1))], np.float32)
    x = rng.uniform(-1.0, 1.0, (600, 3)).astype(np.float32)
    for axis in range(3):
        x[axis * 10:axis * 10 + 10, axis] = special
    x[30:40] = special[:, None]                                        # all three coordinates at once
    x[40:100, 0] = (rng.integers(-4, 5, 60).astype(np.float32) * v)    # more faces, with company in their cells
    f = rng.uniform(0, 255, (600, 5)).astype(np.float32)
    P = np.concatenate([x, f], axis=1)
    bad = []
    for j, val in enumerate([np.nan, np.inf, -np.inf, 40000.0, -40000.0]):
        for k in range(8):
            i = 200 + 8 * j + k
            P[i, k] = val; bad.append(i)
    return np.ascontiguousarray(P[:, :3]), np.ascontiguousarray(P[:, 3:]), np.array(bad)


@pytest.mark.parametrize("mode", ["mean", "central"])
def test_faces_negative_coordinates_and_bad_floats(hiplib, torch, reducer, mode):
    x, f, bad = edge_cloud(0.25)
    assert np.signbit(x[1, 0]) and x[1, 0] == 0 and x[4, 0] < -np.float32(0.25)
    for min_points in (1, 2):
        want = vr.reduce_reading(x, f, np.float32(0.25), mode, min_points)
        got = reducer.reduce(dev(torch, [(x, f)]), 0.25, mode, min_points, want=WANT)[0]
        same(got, want, (mode, min_points))
        assert (want["map"][bad] == -1).all()
        ok = np.setdiff1d(np.arange(x.shape[0]), bad)
        assert min_points > 1 or (want["map"][ok] >= 0).all()
        assert np.isfinite(want["xyz"]).all() and np.isfinite(want["feat"]).all()
    # points 30 .. 39 have the special value in all three coordinates: -0.0 and 0.0 share cell 0; -voxel is cell -1; one ulp below it is cell -2
    m = vr.reduce_reading(x, f, np.float32(0.25), mode, 1)["map"]
    assert m[30] == m[31] and len({m[30], m[33], m[34]}) == 3


# ---- 4. reproducibility
@pytest.mark.parametrize("mode", ["mean", "central"])
def test_same_bytes_every_time_and_under_permutation(hiplib, torch, reducer, dense, mode):
    x, f = dense[1][1]                                                 # (negative coordinates included)
    assert (x[:, 0] < 0).any() and (x[:, 1] < 0).any()
    clouds = dev(torch, [(x, f), (x[:4099], f[:4099])])
    runs = [reducer.reduce(clouds, 0.05, mode, 1, want=WANT) for _ in range(3)]
    first = [{k: (v.clone() if hasattr(v, "clone") else v) for k, v in c.items()} for c in runs[0]]
    for run in runs:
        for a, b in zip(run, first):
            assert a["n_out"] == b["n_out"] and all(torch.equal(a[k], b[k]) for k in KEYS)
    same(runs[0][0], vr.reduce_reading(x, f, 0.05, mode, 1))
    p = np.random.default_rng(9).permutation(x.shape[0])
    got = reducer.reduce(dev(torch, [(x[p], f[p])]), 0.05, mode, 1, want=WANT)[0]
    same(got, vr.reduce_reading(x[p], f[p], 0.05, mode, 1))

    def rows(g):
        a = np.concatenate([g["xyz"].cpu().numpy(), g["feat"].cpu().numpy()], axis=1)
        return [(a[r].tobytes(), int(g["count"][r])) for r in range(g["n_out"])]
    before, after = rows(runs[0][0]), rows(got)
    assert sorted(before) == sorted(after)                             # the same set of rows
    inv = np.argsort(p)                                                # old index -> new index
    m = runs[0][0]["map"].cpu().numpy()
    new_lowest = np.full(len(before), x.shape[0]); np.minimum.at(new_lowest, m[m >= 0], inv[m >= 0])
    assert [before[r] for r in np.argsort(new_lowest)] == after        # in the order of the new lowest indices


# ---- the C ABI itself, with arrays of the test's own
class Raw:
    """one cloud's output arrays as byte tensors prefilled with 0xA5, each with 64 guard bytes behind its cap rows"""
    G = 64

    def __init__(self, torch, cap, n_in, arrays=("xyz", "feat", "count", "source", "map")):
        self.cap = cap
        self.sizes = dict(xyz=12 * cap, feat=20 * cap, count=4 * cap, source=4 * cap, map=4 * n_in)
        self.t = {k: torch.full((self.sizes[k] + self.G,), 0xA5, dtype=torch.uint8, device="cuda") for k in arrays}

    def record(self, api):
        p = lambda k: self.t[k].data_ptr() if k in self.t else None
        return api.ReducedCloud(p("xyz"), p("feat"), p("count"), p("source"), p("map"), self.cap, 0)

    def host(self, key, dtype):
        return self.t[key].cpu().numpy()[:self.sizes[key]].view(dtype)

    def guards_intact(self):
        return all((t.cpu().numpy()[self.sizes[k]:] == 0xA5).all() for k, t in self.t.items())

    def untouched(self):
        return all((t.cpu().numpy() == 0xA5).all() for t in self.t.values())


def raw_reduce(hiplib, R, descs, recs, voxel, mode, min_points, stream=None):
    api = hiplib.api
    n = len(descs)
    arr = (api.DeviceCloud * n)(*descs); out = (api.ReducedCloud * n)(*recs)
    prm = api.ReduceParams(voxel, mode, min_points, 0)
    n_out = np.full(n, -7, np.int32)
    rc = R.L.cvo_reduce_device_clouds(R.h, n, arr, C.byref(prm), out, n_out.ctypes.data_as(C.POINTER(C.c_int)), stream)
    return rc, n_out


# ---- 5. cap
@pytest.mark.parametrize("mode", [0, 1])
def test_cap_below_the_row_count(hiplib, torch, reducer, seven, mode):
    api = hiplib.api
    clouds = [seven[5], seven[4]]
    tens = dev(torch, clouds)
    descs = [api.device_cloud(*t) for t in tens]
    want = [vr.reduce_reading(x, f, 0.05, mode, 1) for x, f in clouds]
    caps = [100, 7]
    assert all(w["n_out"] > c for w, c in zip(want, caps))
    raws = [Raw(torch, c, x.shape[0]) for c, (x, f) in zip(caps, clouds)]
    torch.cuda.synchronize()
    rc, n_out = raw_reduce(hiplib, reducer, descs, [r.record(api) for r in raws], 0.05, mode, 1)
    assert rc == 0, api.load_library().cvo_last_error()
    for k, (r, w) in enumerate(zip(raws, want)):
        c = caps[k]
        assert n_out[k] == w["n_out"]                                  # the full row count
        assert r.host("xyz", np.float32).tobytes() == w["xyz"][:c].tobytes() and r.host("feat", np.float32).tobytes() == w["feat"][:c].tobytes()
        assert r.host("count", np.int32).tobytes() == w["count"][:c].tobytes() and r.host("source", np.int32).tobytes() == w["source"][:c].tobytes()
        assert r.host("map", np.int32).tobytes() == w["map"].tobytes()  # full row numbers
        assert r.guards_intact()
    with pytest.raises(hiplib.CvoError, match="cap 100"):
        reducer.reduce(tens, 0.05, mode, 1, cap=100)
    # cap = 0 with every array NULL counts only
    rc, n_out = raw_reduce(hiplib, reducer, descs, [api.ReducedCloud(None, None, None, None, None, 0, 0)] * 2, 0.05, mode, 1)
    assert rc == 0 and n_out.tolist() == [w["n_out"] for w in want]


# ---- 6. count_voxels
@pytest.mark.parametrize("min_points", [1, 2])
def test_count_voxels_is_the_reading_and_the_reduction(hiplib, torch, reducer, seven, min_points):
    from cvo_slam_amd.voxels import voxel_ladder
    clouds = [seven[4], seven[5], seven[6]]
    tens = dev(torch, clouds)
    sizes = voxel_ladder(0.01, 3.0, 16)
    counts = reducer.count_voxels(tens, sizes, min_points)
    assert counts.shape == (3, 16) and counts.dtype == np.int32
    want = np.array([[vr.count_reading(x, f, v, min_points) for v in sizes] for x, f in clouds])
    assert np.array_equal(counts, want)
    assert len(np.unique(want[2])) >= 8                                # (the ladder really spans the range)
    for j, v in enumerate(sizes):
        got = reducer.reduce(tens, float(v), "mean", min_points, want=())
        assert [g["n_out"] for g in got] == counts[:, j].tolist()
    assert np.array_equal(reducer.count_voxels(tens, sizes, min_points), counts)


# ---- 7. refusals
def test_refusals_change_nothing(hiplib, torch, reducer, seven):
    api = hiplib.api
    x, f = seven[4]; n = x.shape[0]
    tx, tf = up(torch, x), up(torch, f)
    good = api.device_cloud(tx, tf, "points_first")
    bigx = torch.zeros((20001, 3), dtype=torch.float32, device="cuda"); bigf = torch.zeros((20001, 5), dtype=torch.float32, device="cuda")
    too_many_points = api.device_cloud(bigx, bigf, "points_first")
    host = np.zeros((n, 3), np.float32)                                # pageable host memory
    pageable = api.DeviceCloud(host.ctypes.data, good.feat, 12, 20, 4, n, 0)
    raws = [Raw(torch, 300, 20001) for _ in range(9)]
    recs = [r.record(api) for r in raws]
    torch.cuda.synchronize()
    host_out = np.full(12 * 300, 0x5A, np.uint8)
    out_pageable = api.ReducedCloud(host_out.ctypes.data, recs[0].feat, None, None, None, 300, 0)
    cases = [("voxel 0", [good], recs[:1], 0.0, 0, 1), ("voxel negative", [good], recs[:1], -0.05, 0, 1), ("voxel NaN", [good], recs[:1], float("nan"), 0, 1),
             ("voxel inf", [good], recs[:1], float("inf"), 0, 1), ("mode 2", [good], recs[:1], 0.05, 2, 1), ("min_points 0", [good], recs[:1], 0.05, 0, 0),
             ("n > max_points", [good, too_many_points], recs[:2], 0.05, 0, 1), ("count > max_clouds", [good] * 9, recs, 0.05, 0, 1),
             ("pageable input", [good, pageable], recs[:2], 0.05, 0, 1), ("pageable output", [good], [out_pageable], 0.05, 0, 1),
             ("cap 65536", [good], [api.ReducedCloud(recs[0].xyz, recs[0].feat, None, None, None, 65536, 0)], 0.05, 0, 1),
             ("null xyz with cap", [good], [api.ReducedCloud(None, recs[0].feat, None, None, None, 300, 0)], 0.05, 0, 1)]
    for what, descs, out, voxel, mode, min_points in cases:
        rc, n_out = raw_reduce(hiplib, reducer, descs, out, voxel, mode, min_points)
        assert rc == INVALID, what
        assert api.load_library().cvo_last_error(), what
        assert (n_out == -7).all(), what
        torch.cuda.synchronize()
        assert all(r.untouched() for r in raws), what
        assert (host_out == 0x5A).all(), what
    msg = lambda: api.load_library().cvo_last_error().decode()
    raw_reduce(hiplib, reducer, [good, too_many_points], recs[:2], 0.05, 0, 1)
    assert "cloud 1" in msg() and "n 20001" in msg()
    # count_voxels: k outside 1 .. 16, a bad size, min_points 0
    L = api.load_library(); fp = C.POINTER(C.c_float); ip = C.POINTER(C.c_int)
    arr = (api.DeviceCloud * 1)(good)
    for vs, min_points in ([[0.1] * 17, 1], [[], 1], [[0.1, 0.0], 1], [[0.1, float("nan")], 1], [[0.1], 0]):
        v = np.array(vs, np.float32); out = np.full(max(1, v.shape[0]), -7, np.int32)
        assert L.cvo_count_voxels(reducer.h, 1, arr, v.shape[0], v.ctypes.data_as(fp), min_points, out.ctypes.data_as(ip), None) == INVALID
        assert (out == -7).all()
    # and the reducer works after all that
    want = vr.reduce_reading(x, f, 0.05, 0, 1)
    same(reducer.reduce([(tx, tf, "points_first")], 0.05, want=WANT)[0], want)
    with pytest.raises(hiplib.CvoError):
        hiplib.CvoReducer(0, 100)
    with pytest.raises(hiplib.CvoError):
        hiplib.CvoReducer(1, api.REDUCE_MAX_POINTS + 1)


# ---- 8. stream rule
def test_cloud_stream_orders_input_and_output(hiplib, torch, reducer, dense):
    x, f = dense[2][0]
    want = vr.reduce_reading(x, f, 0.05, 0, 1)
    side = torch.cuda.Stream()
    hx, hf = torch.from_numpy(x).pin_memory(), torch.from_numpy(f).pin_memory()
    tx = torch.full((x.shape[0], 3), 1000.0, dtype=torch.float32, device="cuda"); tf = torch.zeros((x.shape[0], 5), dtype=torch.float32, device="cuda")
    a = torch.randn((4096, 4096), device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):                                             # work in front of the writes: without the edge in, the kernel would read the 1000s
            a = a @ a * 1e-3
        tx.copy_(hx, non_blocking=True); tf.copy_(hf, non_blocking=True)
    got = reducer.reduce([(tx, tf, "points_first")], 0.05, "mean", 1, want=WANT, cloud_stream=side)[0]
    with torch.cuda.stream(side):                                      # a read queued on that stream behind the call, and an overwrite behind the read
        snap = {k: got[k].clone() for k in KEYS}
        tx.fill_(-3.0)
        for k in KEYS:
            got[k].zero_()
    side.synchronize()
    same(dict(snap, n_out=got["n_out"]), want)


# ---- 9. end to end
def test_reduced_clouds_align_like_the_reading_s(hiplib, torch, dense):
    from cvo_slam_amd.voxels import voxel_for_budget, lift
    R = hiplib.CvoReducer(8, 20000)
    flat = [c for pair in dense for c in pair]                         # cloud 2 k: fixed of pair k, 2 k + 1: its moving cloud
    tens = dev(torch, flat)
    voxel = voxel_for_budget(R, tens[0], 3072, 0.005, 1.0)
    counts = R.count_voxels(tens[:1], [voxel])
    assert 1000 < counts[0, 0] <= 3072
    got = R.reduce(tens, voxel, "mean", 2, want=WANT)
    want = [vr.reduce_reading(x, f, voxel, "mean", 2) for x, f in flat]
    for k in range(8):
        same(got[k], want[k], k)
        assert 500 < want[k]["n_out"] < 6000
    fi, mi = [0, 2, 4, 6], [1, 3, 5, 7]
    B = hiplib.CvoBatch(4)
    B.set_pairs_clouds([(g["xyz"], g["feat"], "points_first") for g in got], fi, mi)    # the slices as they are: no copy
    B.align_async(4)
    res = B.wait(4)
    Bh = hiplib.CvoBatch(4)
    Bh.set_pairs([(want[a]["xyz"], np.ascontiguousarray(want[a]["feat"].T), want[b]["xyz"], np.ascontiguousarray(want[b]["feat"].T)) for a, b in zip(fi, mi)])
    ref = Bh.align(4)
    for r, q in zip(res, ref):
        assert r["status"] == 0 and q["status"] == 0
        assert r["transform"].tobytes() == q["transform"].tobytes() and r["ell"] == q["ell"] and r["iter"] == q["iter"] and r["A_nonzero"] == q["A_nonzero"]
    # per-point support of the reduced moving cloud, carried back to the dense cloud's points
    sup = B.point_support([0])[0]
    m = got[1]["map"].cpu().numpy()
    assert sup["sum_moving"].shape[0] == want[1]["n_out"]
    dense_sum = lift(m, sup["sum_moving"], -1.0)
    assert dense_sum.shape == (20000,) and (m == -1).any() and (m >= 0).any()
    assert np.array_equal(dense_sum == -1.0, m == -1) and (sup["sum_moving"] >= 0).all()
    assert np.array_equal(dense_sum[m >= 0], sup["sum_moving"][m[m >= 0]])
    on_dev = lift(got[1]["map"], torch.from_numpy(sup["sum_moving"]).cuda(), -1.0)
    assert np.array_equal(on_dev.cpu().numpy(), dense_sum)
    B.close(); Bh.close(); R.close()
