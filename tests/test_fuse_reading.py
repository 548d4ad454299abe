"""The numpy reading of a fusion (tests/fuse_reading.py) against the readings it is built from and against brute force: what the GPU tests
compare with must itself be right.  No GPU."""
import numpy as np
import pytest

import fuse_reading as fr
from fuse_reading import rigid, surface
import support_reading as sup
import voxel_reading as vr

KEYS = ("xyz", "feat", "count", "source", "map")


@pytest.mark.parametrize("mode", ["mean", "central"])
def test_one_member_under_the_identity_is_the_reduction(mode):
    rng = np.random.default_rng(1)
    x, f = surface(rng, 3000, 0.01)
    x[::7] *= np.float32(-1.0)                                         # negative coordinates, but no -0.0: an identity move makes it +0.0
    assert not (np.signbit(x) & (x == 0)).any()
    for pose in (np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)[:3]):
        for min_points in (1, 2):
            got = fr.fuse_reading([(x, f)], [pose], 0.05, mode, min_points)
            want = vr.reduce_reading(x, f, 0.05, mode, min_points)
            assert got["n_out"] == want["n_out"] > 100
            for key in KEYS:
                assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key
            assert (got["views"] == 1).all() and (got["view_mask"] == 1).all() and got["offsets"].tolist() == [0]


@pytest.mark.parametrize("mode", ["mean", "central"])
def test_lone_clouds_under_the_identity_are_their_reductions(mode):
    """what tests/test_gpu_fuse_clouds.py asks of the two kernel families -- a group of one member under the identity gives the reduction's
    bytes -- holds between the two readings, on the same clouds"""
    for x, f in fr.lone_clouds():
        assert not (np.signbit(x) & (x == 0)).any()
        got = fr.fuse_reading([(x, f)], [np.eye(4, dtype=np.float32)], 0.05, mode)
        want = vr.reduce_reading(x, f, 0.05, mode, 1)
        assert got["n_out"] == want["n_out"] >= 1
        for key in KEYS:
            assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), (x.shape[0], key)
        assert (got["views"] == 1).all() and (got["view_mask"] == 1).all()
    assert want["n_out"] > 100 and (want["count"] > 1).any()          # (the 3000-point cloud: many rows, and cells with several members)


@pytest.mark.parametrize("mode", ["mean", "central"])
def test_fusing_is_reducing_the_concatenation_of_the_moved_members(mode):
    rng = np.random.default_rng(2)
    members = [surface(rng, n, 0.01) for n in (700, 0, 1300, 257, 900)]
    poses = [rigid(rng) for _ in members]
    got = fr.fuse_reading(members, poses, 0.1, mode, 2)
    cat_x = np.concatenate([sup.move(p[:3], x).reshape(-1, 3) for (x, f), p in zip(members, poses)])
    cat_f = np.concatenate([f for x, f in members])
    want = vr.reduce_reading(cat_x, cat_f, 0.1, mode, 2)
    assert got["n_out"] == want["n_out"] > 50
    for key in KEYS:
        assert got[key].tobytes() == want[key].tobytes(), key
    assert got["offsets"].tolist() == [0, 700, 700, 2000, 2257]
    if mode == "central":                                              # the row is the winner's MOVED position and its own features
        assert got["xyz"].tobytes() == cat_x[got["source"]].tobytes() and got["feat"].tobytes() == cat_f[got["source"]].tobytes()


def test_views_agree_with_a_brute_force_count():
    rng = np.random.default_rng(3)
    members = [surface(rng, n, 0.02) for n in (400, 300, 0, 500, 350)]
    poses = [rigid(rng, 0.05, 0.05) for _ in members]
    voxel = np.float32(0.2)
    got = fr.fuse_reading(members, poses, voxel, "mean", 1, 1)
    assert got["n_out"] > 20 and got["map"].min() >= 0
    # brute force, point by point: the members whose moved points land in each row's cell
    who = [set() for _ in range(got["n_out"])]
    g = 0
    all_moved = [sup.move(p[:3], x).reshape(-1, 3) for (x, f), p in zip(members, poses)]
    for m, moved in enumerate(all_moved):
        for i in range(moved.shape[0]):
            cell = tuple(np.floor(moved[i] / voxel).astype(np.int64).tolist())
            r = got["map"][g]
            who[r].add(m)
            lo = int(got["source"][r])                                 # (MEAN: the lowest member) its cell is the row's cell
            mm = int(np.searchsorted(got["offsets"], lo, side="right") - 1)
            first = all_moved[mm][lo - got["offsets"][mm]]
            assert cell == tuple(np.floor(first / voxel).astype(np.int64).tolist())
            g += 1
    assert got["views"].tolist() == [len(w) for w in who]
    assert got["view_mask"].tolist() == [sum(1 << m for m in w) for w in who]
    assert got["view_mask"].dtype == np.uint64 and got["views"].dtype == np.int32
    assert not any(2 in w for w in who) and len(set(got["views"].tolist())) >= 3   # the empty member keeps its number; several view counts occur


def test_min_views_keeps_some_cells_and_drops_some():
    rng = np.random.default_rng(4)
    members, poses = fr.windows(rng)
    one = fr.fuse_reading(members, poses, 0.05, "mean", 1, 1)
    two = fr.fuse_reading(members, poses, 0.05, "mean", 1, 2)
    kept, dropped = two["n_out"], one["n_out"] - two["n_out"]
    assert kept > 50 and dropped > 50
    assert (one["views"] >= 2).sum() == kept and (two["views"] >= 2).all()
    keep = one["views"] >= 2
    for key in ("xyz", "feat", "count", "source", "views", "view_mask"):  # the kept rows are the unfiltered rows, in order
        assert two[key].tobytes() == one[key][keep].tobytes(), key
    assert ((two["map"] == -1) == ~np.append(keep, False)[one["map"]]).all()
    four = fr.fuse_reading(members, poses, 0.05, "mean", 1, 4)
    assert 0 < four["n_out"] < kept and (four["view_mask"] == 15).all()


def test_bad_source_floats_and_far_moves_are_invalid():
    rng = np.random.default_rng(5)
    x, f = surface(rng, 64)
    x[3, 1] = np.nan; x[4, 0] = np.inf; x[5, 2] = 32768.0; f[6, 2] = np.nan; f[7, 4] = -40000.0
    far = np.eye(4, dtype=np.float32); far[0, 3] = 32767.5               # moves x >= 0.5 past 2^15
    got = fr.fuse_reading([(x, f), (x, f)], [np.eye(4, dtype=np.float32), far], 0.25)
    assert (got["map"][[3, 4, 5, 6, 7]] == -1).all() and (np.delete(got["map"][:64], [3, 4, 5, 6, 7]) >= 0).all()
    second = got["map"][64:]
    assert ((second == -1) == ((x[:, 0] + np.float32(32767.5) >= 32768.0) | ~np.isfinite(x).all(axis=1) | (np.abs(x) >= 32768).any(axis=1)
                               | ~(np.abs(f) < 32768).all(axis=1))).all()
    assert (second == -1).any() and (second >= 0).any()
    # a zero pose row does not launder a bad source float: 0 * inf is NaN, but 0 * 40000 is 0
    flat = np.eye(4, dtype=np.float32); flat[0, 0] = 0.0
    y = x.copy(); y[10, 0] = 40000.0
    assert fr.fuse_reading([(y, f)], [flat], 0.25)["map"][10] == -1
