"""The numpy reading of the voxel-grid reduction (tests/voxel_reading.py) against a plain dict-and-loop restatement of the definition, and the
properties the definition promises: row order, map / count consistency, permutation invariance, what invalid points get.  No GPU."""
import math

import numpy as np
import pytest

import voxel_reading as vr

SIZES = [0, 1, 2, 257, 3000]
VOXEL = 0.25


def cloud(n, seed, voxel=VOXEL, corners=True):
    """n points in a 2 m box around the origin (so half the coordinates are negative); every fifth point lies exactly on a cell face in x
    (x = k * voxel, k of either sign and 0), every seventh in all three coordinates (corners: several points share such a place)"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    feat = rng.uniform(0.0, 1.0, (n, 5)).astype(np.float32)
    v = np.float32(voxel)
    k = rng.integers(-6, 7, (n, 3)).astype(np.float32)
    xyz[::5, 0] = k[::5, 0] * v
    if corners:
        xyz[::7] = k[::7] * v
    return xyz, feat


def loop_reading(xyz, feat, voxel, mode, min_points):
    """the definition, point by point"""
    v = np.float32(voxel)
    P = np.concatenate([np.asarray(xyz, np.float32).reshape(-1, 3), np.asarray(feat, np.float32).reshape(-1, 5)], axis=1)
    n = P.shape[0]
    members = {}                                                       # cell -> member indices, ascending (insertion order: the lowest member index)
    for i in range(n):
        if not all(math.isfinite(float(x)) and abs(float(x)) < 32768.0 for x in P[i]):
            continue
        with np.errstate(all="ignore"):
            c = tuple(float(np.floor(np.float32(P[i, k]) / v)) for k in range(3))
        if not all(math.isfinite(x) and abs(x) < 1048576.0 for x in c):
            continue
        members.setdefault(c, []).append(i)
    rows = [(c, m) for c, m in members.items() if len(m) >= min_points]
    map_ = np.full(n, -1, np.int32)
    out = np.zeros((len(rows), 8), np.float32); count = np.zeros(len(rows), np.int32); source = np.zeros(len(rows), np.int32)
    for r, (c, m) in enumerate(rows):
        map_[m] = r; count[r] = len(m)
        if mode == vr.MEAN:
            for k in range(8):
                total = 0
                for i in m:
                    total += int(np.rint(np.float64(P[i, k]) * 16777216.0))   # (python integers: no overflow to think about)
                out[r, k] = np.float32(np.float64(total) / (np.float64(len(m)) * 16777216.0))
            source[r] = m[0]
        else:
            best = None
            for i in m:
                with np.errstate(all="ignore"):
                    d = [np.float32(P[i, k]) - (np.float32(c[k]) + np.float32(0.5)) * v for k in range(3)]
                    d2 = np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                if best is None or d2 < best[0]:                       # (strict: a tie keeps the lower index)
                    best = (d2, i)
            source[r] = best[1]; out[r] = P[best[1]]
    return dict(xyz=out[:, :3].copy(), feat=out[:, 3:].copy(), count=count, source=source, map=map_, n_out=len(rows))


def same(a, b):
    assert a["n_out"] == b["n_out"]
    for key in ("xyz", "feat", "count", "source", "map"):
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, key
        assert a[key].tobytes() == b[key].tobytes(), key


@pytest.mark.parametrize("min_points", [1, 3])
@pytest.mark.parametrize("mode", [vr.MEAN, vr.CENTRAL])
@pytest.mark.parametrize("n", SIZES)
def test_reading_is_the_loop(n, mode, min_points):
    xyz, feat = cloud(n, 100 + n)
    got = vr.reduce_reading(xyz, feat, VOXEL, mode, min_points)
    same(got, loop_reading(xyz, feat, VOXEL, mode, min_points))
    assert vr.count_reading(xyz, feat, VOXEL, min_points) == got["n_out"]
    if n >= 257:
        assert 1 < got["n_out"] < n
    if n >= 257 and min_points == 1:                                   # the faces and the negative half are really there
        on_face = (xyz[:, 0] / np.float32(VOXEL)) == np.floor(xyz[:, 0] / np.float32(VOXEL))
        assert on_face.sum() >= n // 5 and (xyz < 0).any() and (xyz[on_face, 0] < 0).any() and (xyz[on_face, 0] == 0).any()


def test_faces_and_negative_coordinates_floor():
    v = np.float32(0.25)
    below = np.nextafter(-v, np.float32(-1))                           # -voxel minus one ulp
    xs = np.array([0.0, -0.0, v, -v, below, np.nextafter(v, np.float32(0)), 2 * v], np.float32)
    xyz = np.zeros((xs.shape[0], 3), np.float32); xyz[:, 0] = xs
    feat = np.zeros((xs.shape[0], 5), np.float32)
    got = vr.reduce_reading(xyz, feat, v, vr.CENTRAL, 1)
    # cells in x: 0, 0, 1, -1, -2, 0, 2 -> rows by lowest member index
    assert got["map"].tolist() == [0, 0, 1, 2, 3, 0, 4]
    assert got["count"].tolist() == [3, 1, 1, 1, 1]
    same(got, loop_reading(xyz, feat, v, vr.CENTRAL, 1))


@pytest.mark.parametrize("min_points", [1, 3])
@pytest.mark.parametrize("mode", [vr.MEAN, vr.CENTRAL])
def test_row_order_map_and_count(mode, min_points):
    xyz, feat = cloud(3000, 7)
    got = vr.reduce_reading(xyz, feat, VOXEL, mode, min_points)
    m = got["map"]
    assert np.array_equal(np.bincount(m[m >= 0], minlength=got["n_out"]), got["count"])
    assert (got["count"] >= min_points).all()
    lowest = np.array([np.flatnonzero(m == r)[0] for r in range(got["n_out"])])
    assert (np.diff(lowest) > 0).all()                                 # rows ascend with the lowest member index
    if mode == vr.MEAN:
        assert np.array_equal(got["source"], lowest)
    else:
        assert np.array_equal(m[got["source"]], np.arange(got["n_out"]))   # the central member is a member
        assert np.array_equal(got["xyz"], xyz[got["source"]]) and np.array_equal(got["feat"], feat[got["source"]])


@pytest.mark.parametrize("min_points", [1, 3])
@pytest.mark.parametrize("mode", [vr.MEAN, vr.CENTRAL])
def test_permutation_keeps_the_set_of_rows(mode, min_points):
    xyz, feat = cloud(3000, 11, corners=False)                         # (two points at one corner tie in d2, and the lower INDEX wins: not a property of the set)
    a = vr.reduce_reading(xyz, feat, VOXEL, mode, min_points)
    p = np.random.default_rng(5).permutation(3000)
    b = vr.reduce_reading(xyz[p], feat[p], VOXEL, mode, min_points)

    def rows(g):
        return sorted((g["xyz"][r].tobytes() + g["feat"][r].tobytes(), int(g["count"][r])) for r in range(g["n_out"]))
    assert _ties(xyz, a) == 0
    assert rows(a) == rows(b)
    assert a["n_out"] == b["n_out"] and a["n_out"] > 0
    # and the rows come in the order of the new lowest indices
    inv = np.argsort(p)                                                # old index -> new index
    new_lowest = np.array([inv[np.flatnonzero(a["map"] == r)].min() for r in range(a["n_out"])])
    order = np.argsort(new_lowest)
    assert np.array_equal(b["count"], a["count"][order]) and b["xyz"].tobytes() == a["xyz"][order].tobytes()


def _ties(xyz, g):
    """rows whose two nearest members are at exactly the same d2 (their winner depends on the order of the input)"""
    v = np.float32(VOXEL); t = 0
    c = np.floor(xyz / v).astype(np.float32)
    d = xyz - (c + np.float32(0.5)) * v
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    for r in range(g["n_out"]):
        q = np.sort(d2[g["map"] == r])
        t += int(q.shape[0] > 1 and q[0] == q[1])
    return t


def test_invalid_points_belong_to_no_cell():
    xyz, feat = cloud(64, 3)
    P = np.concatenate([xyz, feat], 1)
    bad = {}
    for j, val in enumerate([np.nan, np.inf, -np.inf, 40000.0, -40000.0, 32768.0]):
        for k in range(8):
            i = 8 * j + k
            P[i, k] = val; bad[i] = True
    xyz2, feat2 = P[:, :3].copy(), P[:, 3:].copy()
    for mode in (vr.MEAN, vr.CENTRAL):
        got = vr.reduce_reading(xyz2, feat2, VOXEL, mode, 1)
        assert (got["map"][list(bad)] == -1).all()
        assert (got["map"][[i for i in range(64) if i not in bad]] >= 0).all()
        assert np.isfinite(got["xyz"]).all() and np.isfinite(got["feat"]).all()
        same(got, loop_reading(xyz2, feat2, VOXEL, mode, 1))
    # a cell coordinate at or beyond 2^20 in magnitude: 30000 / 0.01 = 3e6
    got = vr.reduce_reading(np.array([[30000.0, 0, 0], [1.0, 0, 0]], np.float32), np.zeros((2, 5), np.float32), 0.01)
    assert got["map"].tolist() == [-1, 0]
    # 32767.99 is inside the range
    got = vr.reduce_reading(np.array([[32767.0, 0, 0]], np.float32), np.zeros((1, 5), np.float32), 1.0)
    assert got["map"].tolist() == [0]
