"""The dense numpy reading of a fusion (cvo_fuse_device_clouds): the definition the kernels are held to bit for bit (include/cvo_hip.h, "Fusing
clouds").  It is built from the two readings it rests on and adds only what is new:

  fusing a group  =  voxel_reading.reduce_reading of the concatenation of the members moved by support_reading.move, features unchanged
                     (a point with a bad SOURCE float is made invalid there too),
                  +  the views filter: a cell's view mask is the OR of 1 << m over its members' member numbers m, views its popcount, and a
                     cell is kept when it has at least min_points members AND at least min_views views,
                  +  the outputs `views` and `view_mask` per row.

Global index: the members' points one member after the other; `source` and `map` speak in it.  The views are computed apart from the
reduction's np.unique: with python sets over the cell keys."""
import numpy as np

import support_reading as sup
import voxel_reading as vr

MEAN, CENTRAL = vr.MEAN, vr.CENTRAL


def pose34(pose):
    M = np.asarray(pose, np.float32)
    assert M.shape in ((3, 4), (4, 4))
    return np.ascontiguousarray(M[:3])


def moved_concat(members, poses):
    """(xyz (N, 3) moved, feat (N, 5), member (N,) member numbers, offsets (members,)) of a group; a point with a source float that is not
    finite and below 2^15 gets a NaN position: invalid for the reduction, whatever its pose makes of it"""
    assert 1 <= len(members) <= 64 and len(poses) == len(members)
    xs, fs, ms, offsets, at = [], [], [], [], 0
    for m, ((x, f), pose) in enumerate(zip(members, poses)):
        P = vr.points8(x, f)
        with np.errstate(all="ignore"):
            moved = sup.move(pose34(pose), P[:, :3]).reshape(-1, 3)
            bad = ~(np.abs(P) < np.float32(32768.0)).all(axis=1)
        moved[bad] = np.nan
        xs.append(moved); fs.append(P[:, 3:]); ms.append(np.full(P.shape[0], m, np.int64)); offsets.append(at); at += P.shape[0]
    return (np.ascontiguousarray(np.concatenate(xs)), np.ascontiguousarray(np.concatenate(fs)), np.concatenate(ms), np.asarray(offsets, np.int64))


def cell_views(xyz, feat, member, voxel):
    """{cell key: set of member numbers} over the valid points"""
    ok, _, key = vr.cells(vr.points8(xyz, feat), voxel)
    seen = {}
    for k, m, good in zip(key.tolist(), member.tolist(), ok.tolist()):
        if good:
            seen.setdefault(k, set()).add(m)
    return seen, key


def fuse_reading(members, poses, voxel, mode=MEAN, min_points=1, min_views=1):
    """members: [(xyz (n, 3), feat (n, 5))], poses: 3 x 4 or 4 x 4 each.  dict(xyz, feat, count, source, views (rows,) i32, view_mask (rows,) u64,
    map (N,) i32, n_out, offsets)"""
    assert 1 <= min_views <= 64
    xyz, feat, member, offsets = moved_concat(members, poses)
    base = vr.reduce_reading(xyz, feat, voxel, mode, min_points)        # the cells with enough members, in row order
    seen, key = cell_views(xyz, feat, member, voxel)
    rows = base["n_out"]
    mask = np.zeros(rows, np.uint64); views = np.zeros(rows, np.int32)
    for r in range(rows):
        who = seen[int(key[base["source"][r]])]                          # (the source is a member of the row's cell in either mode)
        mask[r] = np.uint64(sum(1 << m for m in who)); views[r] = len(who)
    keep = views >= min_views
    new_row = np.full(rows + 1, -1, np.int32); new_row[:rows][keep] = np.arange(int(keep.sum()), dtype=np.int32)   # (row order is kept; [-1] -> -1)
    return dict(xyz=np.ascontiguousarray(base["xyz"][keep]), feat=np.ascontiguousarray(base["feat"][keep]), count=base["count"][keep],
                source=base["source"][keep], views=views[keep], view_mask=mask[keep], map=new_row[base["map"]], n_out=int(keep.sum()), offsets=offsets)


# ---- scenes the fusion tests share
def rigid(rng, angle=0.2, shift=0.3):
    """a random rigid 4 x 4 pose: rotation by up to `angle` about a random axis, translation up to `shift`"""
    a = rng.normal(size=3); a /= np.linalg.norm(a)
    t = rng.uniform(-angle, angle)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K
    M = np.eye(4); M[:3, :3] = R; M[:3, 3] = rng.uniform(-shift, shift, 3)
    return M.astype(np.float32)


def surface(rng, n, noise=0.0):
    """n points of a wavy sheet about 2 m in front, with features"""
    u = rng.uniform(-1.0, 1.0, (n, 2))
    z = 2.0 + 0.2 * np.sin(3 * u[:, 0]) * np.cos(2 * u[:, 1])
    x = np.stack([u[:, 0], u[:, 1], z], axis=1) + rng.normal(scale=noise, size=(n, 3)) if noise else np.stack([u[:, 0], u[:, 1], z], axis=1)
    return np.ascontiguousarray(x, np.float32), rng.uniform(0, 255, (n, 5)).astype(np.float32)


LONE_SIZES = (1, 63, 64, 65, 255, 256, 257, 3000)


def lone_clouds():
    """a cloud of each of LONE_SIZES points -- one point, wave edges, block edges, many blocks -- on the noisy sheet: each fused alone under the
    identity pose is its own reduction.  No coordinate is -0.0, which 1 * x + (0 * y + 0 * z) + 0 would turn into +0.0"""
    rng = np.random.default_rng(21)
    clouds = [surface(rng, n, 0.01) for n in LONE_SIZES]
    for x, f in clouds:
        assert not (np.signbit(x) & (x == 0)).any()
    return clouds


def windows(rng, members=4, n=4000, noise=0.004):
    """the same sheet seen `members` times: an overlapping window of it each, with noise, given in a camera frame of its own -- so that under the
    poses cells with one view and cells with several both exist.  ([(xyz, feat)], [4 x 4 pose])"""
    base_x, base_f = surface(rng, n)
    out, poses = [], []
    for m in range(members):
        lo = -1.0 + 0.3 * m
        pick = (base_x[:, 0] >= lo) & (base_x[:, 0] < lo + 1.1)
        x = base_x[pick] + rng.normal(scale=noise, size=(int(pick.sum()), 3)).astype(np.float32)
        P = rigid(rng, 0.1, 0.2)
        inv = np.linalg.inv(P.astype(np.float64))
        out.append((np.ascontiguousarray((x @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)), np.ascontiguousarray(base_f[pick]))); poses.append(P)
    return out, poses
