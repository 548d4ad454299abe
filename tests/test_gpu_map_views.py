"""Viewing resident maps in place (cvo_maps_view, CvoMaps.view) against the reading of its definition (tests/map_view_reading.py): the view of the
map's uncapped extract, in the map's row numbers.  Every comparison is exact, on bytes: positions, features, sources, pixels, relations, maps,
the two z-buffer images, the carve bytes, the row counts and the relation counts."""
import ctypes as C

import numpy as np
import pytest

import fuse_reading as fr
import map_reading as mr
import map_view_reading as mv
import view_reading as vw
import voxel_reading as vr
from test_gpu_maps import WANT as MAP_WANT, snapshot, unchanged
from test_gpu_view_clouds import Raw, depth_image, loaded_hip, up_depth

pytestmark = pytest.mark.gpu

INVALID = 4
KEYS = ("xyz", "feat", "source", "pixel", "map", "depth", "index")
WANT = ("source", "pixel", "map", "depth", "index")
ALL = WANT + ("relation",)
EYE = np.eye(4, dtype=np.float32)
MODES = (("front", 0.0), ("surface", 0.0), ("surface", 0.05))
MAX_ROWS = 20000
SHEET_CAM = (5000.0, 60.0, 60.0, 32.0, 24.0)                           # sees map_reading.sliding_windows' sheet from its maps' origin


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


@pytest.fixture(scope="module")
def window():
    members, poses = mr.sliding_windows(np.random.default_rng(42))
    return members, poses


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev(torch, members):
    return [(up(torch, x), up(torch, f), "points_first") for x, f in members]


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else t


def mode_of(name):
    return dict(front=vw.FRONT, surface=vw.SURFACE)[name]


def same(got, want, what="", keys=KEYS):
    """a view's dict against the reading's; "relation" brings relation_counts with it, "carve" is a key like any other"""
    assert got["n_out"] == want["n_out"], (what, got["n_out"], want["n_out"])
    for key in keys:
        g = host(got[key])
        assert g.dtype == want[key].dtype and g.shape == want[key].shape, (what, key, g.dtype, g.shape, want[key].shape)
        assert g.tobytes() == want[key].tobytes(), (what, key)
    if "relation" in keys:
        assert np.array_equal(got["relation_counts"], want["relation_counts"]), (what, got["relation_counts"], want["relation_counts"])


def per_view(flts):
    """a list of map_view_reading.filter_of dicts as CvoMaps.view's three keyword lists"""
    return {k: [f[k] for f in flts] for k in ("min_points", "min_views", "min_last_stamp")}


LOOSE = mv.filter_of(1, 1, 0)


@pytest.fixture(scope="module")
def lattices(hiplib, torch, reducer):
    """per scene: a CvoMaps whose map j has exactly SCENE_SIZES[j] rows (a lattice member, a cell per point), the readings, their extracts, and
    per view of either call of SCENE_CALLS the observed depth: the view's own rendering shifted by bands"""
    out = {}
    for which in ("small", "wide"):
        S = mv.scene(which)
        sizes = list(vw.SCENE_SIZES)
        M = hiplib.CvoMaps(reducer, len(sizes), 4096, mv.VOXEL)
        R = [mr.Map(4096, mv.VOXEL) for _ in sizes]
        M.integrate(list(range(len(sizes))), [dev(torch, [S["lattice"][n]]) for n in sizes], [[EYE]] * len(sizes), [[0]] * len(sizes))
        for j, n in enumerate(sizes):
            R[j].update([S["lattice"][n]], [EYE], [0])
            assert R[j].rows == n
        S["M"], S["R"], S["of"] = M, R, {n: j for j, n in enumerate(sizes)}
        S["E"] = [r.extract(**LOOSE) for r in R]
        S["observed"] = [[vw.shifted_rendering((S["E"][S["of"][n]]["xyz"], S["E"][S["of"][n]]["feat"]), S["poses"][k], S["camera"], S["size"])
                          for k, n in enumerate(call)] for call in vw.SCENE_CALLS]
        out[which] = S
    yield out
    for S in out.values():
        S["M"].close()


# ---- 1. edge row counts
@pytest.mark.parametrize("cell", [1, 2, 3, 16])
@pytest.mark.parametrize("which", ["small", "wide"])
def test_edge_row_counts_one_call_of_eight_views(hiplib, torch, reducer, lattices, which, cell):
    S = lattices[which]
    w, h = S["size"]
    M, R = S["M"], S["R"]
    before = snapshot(M, None)
    for mode, slack in MODES:
        p = vw.params(w, h, cell, mode_of(mode), slack)
        for call, obs in zip(vw.SCENE_CALLS, S["observed"]):
            assert call.count(3000) == 2                               # the same map in two views, under different poses
            ks = [S["of"][n] for n in call]
            got = M.view(ks, S["poses"], S["camera"], (w, h), cell, mode, slack, observed=[up_depth(torch, o) for o in obs], want=ALL, carve=True)
            assert len(got) == 8
            for k, n in enumerate(call):
                want = mv.map_view_reading(R[ks[k]], LOOSE, S["poses"][k], S["camera"], p, obs[k], E=S["E"][ks[k]])
                same(got[k], want, (which, cell, mode, slack, k, n), KEYS + ("relation", "carve"))
                assert host(got[k]["map"]).shape == (n,) and host(got[k]["carve"]).shape == (n,)
            rows = [g["n_out"] for g, n in zip(got, call) if n == 3000]
            assert min(rows) > 0 and (mode != "front" or max(rows) <= -(-w // cell) * -(-h // cell))
    unchanged(M, None, before)                                          # a view only reads


# ---- 2. dead rows and filters; 3. histories
@pytest.mark.parametrize("cell", [1, 3])
def test_dead_rows_and_every_clause_of_the_filter(hiplib, torch, reducer, cell):
    S = mv.scene("small")
    w, h = S["size"]
    members, poses = S["windows"]
    tens = dev(torch, members)
    steps, R = mv.history(S["windows"], MAX_ROWS)
    M = hiplib.CvoMaps(reducer, 2, MAX_ROWS, mv.VOXEL)
    for sign, m, st in steps:
        (M.integrate if sign > 0 else M.remove)([1], [[tens[m]]], [[poses[m]]], [[st]])
    assert R.rows > R.live > 1000
    flts = list(mv.FILTERS) + [mv.FILTERS[4], mv.FILTERS[1], LOOSE]     # different filters on the same map in one call, and other poses
    vposes = [S["poses"][1]] * 5 + S["poses"][5:8]
    for mode, slack in MODES:
        p = vw.params(w, h, cell, mode_of(mode), slack)
        got = M.view([1] * 8, vposes, S["camera"], (w, h), cell, mode, slack, want=WANT, **per_view(flts))
        for k in range(8):
            want = mv.map_view_reading(R, flts[k], vposes[k], S["camera"], p)
            same(got[k], want, (cell, mode, slack, k))
            assert (want["map"] == mv.FILTERED).sum() >= R.rows - R.live > 0
    p = vw.params(w, h, cell)
    for k, clause in mv.CLAUSE_OF.items():                             # each clause filters rows that would otherwise be fronts
        assert mv.fronts_lost_to(R, mv.FILTERS[k], clause, S["poses"][1], S["camera"], p) > 0, clause
    assert M.view([0], [EYE], S["camera"], (w, h), cell, want=("index",))[0]["n_out"] == 0   # the untouched map: nothing, and an empty z-buffer
    M.close()


def test_eight_maps_with_histories_of_their_own_in_one_call(hiplib, torch, reducer, window):
    members, poses = window
    members = members[:9] + [(np.zeros((0, 3), np.float32), np.zeros((0, 5), np.float32))]     # member 9 is empty
    tens = dev(torch, members)
    M = hiplib.CvoMaps(reducer, 8, MAX_ROWS, 0.05)
    R = [mr.Map(MAX_ROWS, 0.05) for _ in range(8)]
    # test_gpu_maps' history: call -> {map: (member numbers, sign)}; map 7 stays untouched, map 6 only ever gets the empty member
    calls = [{0: ([0], 1), 1: ([0, 1, 2], 1), 2: ([9, 3], 1), 3: ([5], 1), 6: ([9], 1)},
             {0: ([1], 1), 1: ([1], -1), 2: ([4, 9, 5], 1), 4: ([8, 7, 6], 1), 5: ([2], 1)},
             {0: ([0], -1), 2: ([3], -1), 3: ([5], -1), 4: ([7], -1), 5: ([2, 3], 1), 1: ([3], 1)},
             {3: ([6], 1), 5: ([2], -1), 0: ([2, 3, 4, 5], 1)},
             {0: ([6], 1), 1: ([6], 1), 2: ([6, 9], 1), 3: ([7], 1), 4: ([9, 0], 1), 5: ([1], 1), 6: ([9, 9], 1)}]
    rng = np.random.default_rng(61)
    vposes = [fr.rigid(rng, 0.05, 0.1) for _ in range(8)]
    flts = [mv.filter_of(1, 1 + k % 2, 0) for k in range(8)]
    for t, call in enumerate(calls):
        ks = list(call)
        for sign in (1, -1):
            pick = [k for k in ks if call[k][1] == sign]
            if not pick:
                continue
            args = (pick, [[tens[m] for m in call[k][0]] for k in pick], [[poses[min(m, 8)] for m in call[k][0]] for k in pick], [[m + 60 for m in call[k][0]] for k in pick])
            (M.integrate if sign > 0 else M.remove)(*args)
            for k, g, ps, st in zip(*args):
                R[k].update([members[m] for m in call[k][0]], ps, st, sign)
        mode, slack = MODES[t % 3]
        cell = (1, 2, 3, 16, 2)[t]
        obs = [vw.shifted_rendering((e["xyz"], e["feat"]), vposes[k], SHEET_CAM, (64, 48)) for k, e in enumerate(R[k].extract(**flts[k]) for k in range(8))]
        got = M.view(list(range(8)), vposes, SHEET_CAM, (64, 48), cell, mode, slack, observed=[up_depth(torch, o) for o in obs], want=ALL, carve=True, **per_view(flts))
        for k in range(8):
            want = mv.map_view_reading(R[k], flts[k], vposes[k], SHEET_CAM, vw.params(64, 48, cell, mode_of(mode), slack), obs[k])
            same(got[k], want, (t, k), KEYS + ("relation", "carve"))
    assert R[7].rows == 0 and R[6].rows == 0 and R[3].rows > R[3].live > 0 and got[0]["n_out"] > 200 and got[7]["n_out"] == 0
    M.close()


# ---- 4. the edges of the definition
def test_edges_of_the_definition_carry_over(hiplib, torch, reducer):
    """view_reading.edge_cloud's points as map rows: a voxel of 2^-10 m, and as many maps as it takes for every point to be alone in its cell.  A
    row's mean is the point itself wherever the point's floats lie on the sums' 2^-24 grid, which the reading shows for the image's four
    borders and z_far; floats such as 0.1f, 0.05f and 2e-6f have finer bits, and their rows hold the value rounded to that grid: the
    points at z_near and the twins are compared against the reading of what the map holds, like every other row"""
    x, f, names = vw.edge_cloud()
    voxel = 2.0 ** -10
    ok, _, key = vr.cells(np.concatenate([x, f], axis=1), voxel)
    groups, seen = [], []
    for i in np.flatnonzero(ok).tolist():                               # point i into the first map that does not hold its cell yet
        j = next((j for j, s in enumerate(seen) if int(key[i]) not in s), len(seen))
        if j == len(seen):
            groups.append([]); seen.append(set())
        groups[j].append(i); seen[j].add(int(key[i]))
    assert 2 <= len(groups) <= 4 and sum(len(g) for g in groups) == ok.sum() == len(names) - 2   # (the NaN and the source float past 2^15 enter no map)
    M = hiplib.CvoMaps(reducer, len(groups), 64, voxel)
    R = [mr.Map(64, voxel) for _ in groups]
    clouds = [(np.ascontiguousarray(x[g]), np.ascontiguousarray(f[g])) for g in groups]
    M.integrate(list(range(len(groups))), [dev(torch, [c]) for c in clouds], [[EYE]] * len(groups), [[0]] * len(groups))
    exact = []
    for r, c, g in zip(R, clouds, groups):
        r.update([c], [EYE], [0])
        e = r.extract(**LOOSE)
        assert r.rows == len(g) and e["feat"].tobytes() == c[1].tobytes()
        on_grid = (np.rint(c[0].astype(np.float64) * 2.0 ** 24) == c[0].astype(np.float64) * 2.0 ** 24).all(axis=1)
        assert e["xyz"][on_grid].tobytes() == (c[0][on_grid] + np.float32(0)).tobytes()      # (+ 0: a -0.0 is summed to +0.0)
        exact += [names[g[i]] for i in np.flatnonzero(on_grid)]
    assert len(exact) >= 8 and all(any(n.startswith(edge) for n in exact) for edge in ("u = -0.5", "u just below", "u = width", "u two steps", "v = -0.5", "v = height", "z' = z_far", "z' just above z_far"))
    w, h = vw.EDGE_SIZE
    ks = list(range(len(groups)))
    for mode, slack in MODES:
        for z_range in ((0.05, 30.0), (1e-6, 30.0)):
            p = vw.params(w, h, 1, mode_of(mode), slack, z_near=z_range[0], z_far=z_range[1])
            got = M.view(ks + ks, [EYE] * len(ks) + [vw.EDGE_FAR_MOVE] * len(ks), vw.EDGE_CAM, (w, h), 1, mode, slack, z_range=z_range, want=WANT)
            for k, j in enumerate(ks + ks):
                pose = EYE if k < len(ks) else vw.EDGE_FAR_MOVE
                same(got[k], mv.map_view_reading(R[j], LOOSE, pose, vw.EDGE_CAM, p), (mode, slack, z_range, k))
    far = [host(g["map"]) for g in got[len(ks):]]
    assert any((m == -3).any() for m in far) and any((m == -2).any() for m in far)    # x' past 2^15 is invalid; the row below it is valid and out of view
    M.close()


# ---- 5. observed depth, carve and the compaction
@pytest.mark.parametrize("which", ["small", "wide"])
def test_observed_depth_carve_and_the_compaction_it_feeds(hiplib, torch, reducer, which):
    from cvo_slam_amd.voxels import carve_mask
    S = mv.scene(which)
    w, h = S["size"]
    members, poses = S["windows"]
    tens = dev(torch, members)
    flt = mv.filter_of(1, 2, 0)
    for (mode, slack), cell, tol in zip(MODES, (1, 2, 3), (0.02, 0.0, 0.3)):
        M = hiplib.CvoMaps(reducer, 2, MAX_ROWS, mv.VOXEL)              # map 0: viewed in place; map 1: its twin on the extract + view + carve_mask route
        R = mr.Map(MAX_ROWS, mv.VOXEL)
        stamps = list(range(len(members)))                             # all six windows: the walls over the whole image, every band of the shifted rendering seen
        M.integrate([0, 1], [tens, tens], [poses, poses], [stamps] * 2); R.update(members, poses, stamps)
        E = R.extract(**flt)
        pose = S["poses"][3]
        obs = vw.shifted_rendering((E["xyz"], E["feat"]), pose, S["camera"], (w, h))
        d_obs = up_depth(torch, obs)
        want = mv.map_view_reading(R, flt, pose, S["camera"], vw.params(w, h, cell, mode_of(mode), slack, depth_tol=tol), obs, E=E)
        got = M.view([0], [pose], S["camera"], (w, h), cell, mode, slack, observed=[d_obs], depth_tol=tol, want=ALL, carve=True, **per_view([flt]))[0]
        same(got, want, (which, mode, cell, tol), KEYS + ("relation", "carve"))
        if tol == 0.02:
            assert (want["relation_counts"] >= 0.02 * want["n_out"]).all() and 0 < want["carve"].sum() == want["relation_counts"][1]
        if tol == 0.3:
            assert want["relation_counts"][1] == 0 and want["carve"].sum() == 0
        e = M.extract([1], want=("row",), **flt)[0]
        v = reducer.view([(e["xyz"], e["feat"], "points_first")], [pose], S["camera"], (w, h), cell, mode, slack, observed=[d_obs], depth_tol=tol, want=("source", "relation"))[0]
        old = carve_mask(R.rows, e["row"], v["source"], v["relation"])
        assert host(old).tobytes() == host(got["carve"]).tobytes()
        rows_out = M.compact([0, 1], drop=[got["carve"], old], new_row=True)
        new_row = R.compact(drop=want["carve"])
        assert rows_out[0].tolist() == [R.rows, R.rows] and all(host(t).tobytes() == new_row.tobytes() for t in rows_out[1])
        a, b = M.extract([0, 1], 0, 0, -2 ** 31, want=MAP_WANT)
        r = R.extract(0, 0, -2 ** 31)
        for e in (a, b):
            assert e["n_out"] == r["n_out"] and all(host(e[k]).view(r[k].dtype).tobytes() == r[k].tobytes() for k in mr.OUTPUTS)
        M.close()


# ---- 6. the tracker loop
def test_the_loop_with_carving_and_probation_on_view_beside_extract_and_view(hiplib, torch, reducer, window):
    """INTEGRATION.md's loop, two streams in every call, twice: object A carves by extract + CvoReducer.view + carve_mask, object B by
    CvoMaps.view's carve bytes.  After every step the two objects' maps have equal bytes, and both are the reading's"""
    from cvo_slam_amd.voxels import carve_mask
    members, poses = window
    tens = dev(torch, members)
    K, size = 3, (64, 48)
    A, B = hiplib.CvoMaps(reducer, 2, MAX_ROWS, 0.05), hiplib.CvoMaps(reducer, 2, MAX_ROWS, 0.05)
    R = [mr.Map(MAX_ROWS, 0.05) for _ in range(2)]
    shift = (0, 1)                                                     # stream s sees member t + shift[s]
    rng = np.random.default_rng(62)
    carved = 0
    for t in range(9):
        new = [t + d for d in shift]
        for M in (A, B):
            M.integrate([0, 1], [[tens[m]] for m in new], [[poses[m]] for m in new], [[t], [t]])
        for s in range(2):
            R[s].update([members[new[s]]], [poses[new[s]]], [t])
        if t >= K:
            old = [t - K + d for d in shift]
            for M in (A, B):
                M.remove([0, 1], [[tens[m]] for m in old], [[poses[m]] for m in old], [[t - K], [t - K]], present=True)
            for s in range(2):
                R[s].update([members[old[s]]], [poses[old[s]]], [t - K], -2)
        vposes = [fr.rigid(rng, 0.03, 0.05) for _ in range(2)]
        flt = mv.filter_of(1, 2, 0)
        E = [R[s].extract(**flt) for s in range(2)]
        obs = [vw.shifted_rendering((E[s]["xyz"], E[s]["feat"]), vposes[s], SHEET_CAM, size) for s in range(2)]
        d_obs = [up_depth(torch, o) for o in obs]
        want = [mv.map_view_reading(R[s], flt, vposes[s], SHEET_CAM, vw.params(*size, 2), obs[s], E=E[s]) for s in range(2)]
        # A: the parent's route
        ext = A.extract([0, 1], want=("row",), **flt)
        seen = reducer.view([(e["xyz"], e["feat"], "points_first") for e in ext], vposes, SHEET_CAM, size, 2, observed=d_obs, want=("source", "relation"))
        drop_a = [carve_mask(R[s].rows, ext[s]["row"], seen[s]["source"], seen[s]["relation"]) for s in range(2)]
        # B: in place
        got = B.view([0, 1], vposes, SHEET_CAM, size, 2, observed=d_obs, want=ALL, carve=True, **per_view([flt, flt]))
        for s in range(2):
            same(got[s], want[s], (t, s), KEYS + ("relation", "carve"))
            assert host(drop_a[s]).tobytes() == want[s]["carve"].tobytes()
            assert host(seen[s]["xyz"]).tobytes() == host(got[s]["xyz"]).tobytes() and host(ext[s]["row"])[host(seen[s]["source"])].tolist() == host(got[s]["source"]).tolist()
            carved += int(want[s]["carve"].sum())
        A.compact([0, 1], min_views=2, probation_from=t - 1, drop=drop_a)
        B.compact([0, 1], min_views=2, probation_from=t - 1, drop=[g["carve"] for g in got])
        for s in range(2):
            R[s].compact(min_views=2, probation_from=t - 1, drop=want[s]["carve"])
        a, b = snapshot(A, [0, 1]), snapshot(B, [0, 1])
        assert a[1:] == b[1:] == ([R[0].rows, R[1].rows], [R[0].live, R[1].live])
        for s in range(2):
            r = R[s].extract(0, 0, -2 ** 31)
            for e in (a[0][s], b[0][s]):
                assert e["n_out"] == r["n_out"] and all(host(e[k]).view(r[k].dtype).tobytes() == r[k].tobytes() for k in mr.OUTPUTS), (t, s)
    assert R[0].rows > 50 and carved > 20
    A.close(); B.close()


# ---- 7. past the extract's cap: what the feature is for
def test_a_map_whose_filter_keeps_more_than_65535_rows_is_seen(hiplib, torch):
    members, poses = mv.past_the_cap()
    red = hiplib.CvoReducer(2, 98304)
    M = hiplib.CvoMaps(red, 2, mv.PAST_MAX_ROWS, mv.PAST_VOXEL)
    R = mr.Map(mv.PAST_MAX_ROWS, mv.PAST_VOXEL)
    try:
        M.integrate([0], [dev(torch, members)], [poses], [[0, 1, 2]]); R.update(members, poses, [0, 1, 2])
        E = R.extract(**LOOSE)
        assert E["n_out"] > 65535 and -(-(-(-R.rows // 256)) // 256) == 2              # the block counts are scanned at two blocks per thread
        assert M.extract([0], cap=0, want=())[0]["n_out"] == E["n_out"] > 65535         # extract reports more rows than its cap can hold ...
        with pytest.raises(hiplib.CvoError, match="more than cap 65535"):
            M.extract([0])                                                              # ... and cannot return them
        obs = vw.shifted_rendering((E["xyz"], E["feat"]), mv.PAST_POSE, mv.PAST_CAMERA, mv.PAST_SIZE)
        d_obs = up_depth(torch, obs)
        for cell in (1, 2):
            for mode, slack in (("front", 0.0), ("surface", 0.05)):
                p = vw.params(*mv.PAST_SIZE, cell=cell, mode=mode_of(mode), slack=slack)
                want = mv.map_view_reading(R, LOOSE, mv.PAST_POSE, mv.PAST_CAMERA, p, obs, E=E)
                assert 10000 < want["V"]["n_out"] <= 65535 and want["source"].max() > 65536
                got = M.view([0], [mv.PAST_POSE], mv.PAST_CAMERA, mv.PAST_SIZE, cell, mode, slack, observed=[d_obs], want=ALL, carve=True)[0]
                same(got, want, (cell, mode), KEYS + ("relation", "carve"))
    finally:
        M.close(); red.close()


# ---- 8. more rows than the reducer's max_points: the region is laid out from the call's own sizes
def up16(v):
    return (v + 15) & ~15


def region_bytes(cells, rows):
    """the header's rule: the z-buffer, a code word per row, the blocks' counts and relation counts, each rounded up to 16 bytes"""
    blocks = -(-rows // 256)
    return up16(8 * cells) + up16(4 * rows) + up16(4 * blocks) + up16(16 * blocks)


def test_a_map_of_more_rows_than_max_points_fits_by_the_byte_rule_or_is_refused(hiplib, torch):
    max_points, size, cell, cam = 256, (64, 48), 4, vw.CAM_SMALL
    cells = 16 * 12
    region = 384 * max_points
    fit = max(r for r in range(23000, 25000) if region_bytes(cells, r) <= region)
    need = region_bytes(cells, fit + 4)
    assert region_bytes(cells, fit) <= region < need <= region + 64 and fit > 90 * max_points
    # fit + 4 points, each alone in its cell: a box of cells in front of the camera, in shuffled order
    rng = np.random.default_rng(63)
    c = np.stack(np.meshgrid(np.arange(-20, 21), np.arange(-15, 15), np.arange(30, 52), indexing="ij"), axis=-1).reshape(-1, 3)
    c = c[rng.permutation(c.shape[0])[:fit + 4]]
    assert c.shape[0] == fit + 4
    x = ((c + 0.5 + rng.uniform(-0.2, 0.2, c.shape)) * mv.VOXEL).astype(np.float32); f = rng.uniform(0, 255, (c.shape[0], 5)).astype(np.float32)
    red = hiplib.CvoReducer(2, max_points)
    M = hiplib.CvoMaps(red, 1, 30000, mv.VOXEL)
    R = mr.Map(30000, mv.VOXEL)
    try:
        tx, tf = up(torch, x), up(torch, f)
        def grow(lo, hi):
            for at in range(lo, hi, max_points):
                end = min(hi, at + max_points)
                M.integrate([0], [[(tx[at:end], tf[at:end], "points_first")]], [[EYE]], [[0]]); R.update([(x[at:end], f[at:end])], [EYE], [0])
        grow(0, fit)
        assert R.rows == fit == int(M.rows([0])[0][0])
        pose = fr.rigid(rng, 0.03, 0.05)
        E = R.extract(**LOOSE)
        for mode, slack in MODES[::2]:
            want = mv.map_view_reading(R, LOOSE, pose, cam, vw.params(*size, cell, mode_of(mode), slack), E=E)
            same(M.view([0], [pose], cam, size, cell, mode, slack, want=WANT)[0], want, (mode, "fits"))
        assert (want["map"] == -1).sum() > 1000 and want["source"].max() > 20000
        grow(fit, fit + 4)                                              # a few bytes more than a region has
        before = snapshot_rows(M)
        for call in (M.view, M.check_view):
            with pytest.raises(hiplib.CvoError, match=f"{need} bytes.*{region} bytes"):
                call([0], [pose], cam, size, cell)
        assert snapshot_rows(M) == before
    finally:
        M.close(); red.close()


def snapshot_rows(M):
    rows, live = M.rows(None)
    return rows.tolist(), live.tolist()


# ---- 9. the C ABI itself: cap, guards, count only, refusals
def a_view(api, k, pose, flt=LOOSE, cam=0):
    return api.MapView(k, cam, api.MapFilter(flt["min_points"], flt["min_views"], flt["min_last_stamp"], 0), (C.c_float * 12)(*np.asarray(pose, np.float32)[:3].reshape(-1).tolist()))


def raw_view(hiplib, M, views, recs, cams, size=(64, 48), cell=1, mode=0, z_near=0.05, z_far=30.0, slack=0.0, depth_tol=0.02, observed=None, carve=None, stream=None,
             count=None, check_only=False, want_counts=True, handle=True):
    api = hiplib.api
    count = len(views) if count is None else count
    arr = (api.MapView * max(1, len(views)))(*views); out = (api.ViewedCloud * max(1, len(recs)))(*recs)
    cs = (api.Camera * len(cams))(*[api.Camera(*c) for c in cams])
    prm = api.ViewParams(size[0], size[1], cell, mode, z_near, z_far, slack, depth_tol)
    obs = None if observed is None else (api.DeviceImage * len(observed))(*observed)
    cv = None if carve is None else (C.c_void_p * len(carve))(*carve)
    n_out = np.full(max(1, count), -7, np.int32); counts = np.full((max(1, count), 4), -7, np.int32)
    ip = C.POINTER(C.c_int)
    h = M.h if handle else None
    if check_only:
        return M.L.cvo_check_maps_view(h, count, arr, cs, C.byref(prm), obs, out, cv), n_out, counts
    rc = M.L.cvo_maps_view(h, count, arr, cs, C.byref(prm), obs, out, cv, n_out.ctypes.data_as(ip), counts.ctypes.data_as(ip) if want_counts else None, stream)
    return rc, n_out, counts


@pytest.mark.parametrize("mode,slack", [(0, 0.0), (1, 0.05)], ids=["front", "surface"])
def test_cap_below_the_row_count_guards_and_count_only(hiplib, torch, reducer, lattices, mode, slack):
    api = hiplib.api
    S = lattices["small"]
    w, h = S["size"]
    k, pose, obs = S["of"][3000], S["poses"][6], S["observed"][0][6]
    M, R = S["M"], S["R"][k]
    want = mv.map_view_reading(R, LOOSE, pose, S["camera"], vw.params(w, h, 2, mode, slack), obs, E=S["E"][k])
    cap = 100
    assert want["n_out"] > cap and want["relation"][cap:].shape[0] > 0 and want["carve"][want["source"][cap:]].sum() > 0   # rows past cap are carved too
    raw = Raw(torch, cap, 3000, (w // 2) * (h // 2))
    carve = torch.full((3000 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    d_obs = up_depth(torch, obs)
    views = [a_view(api, k, pose)]
    torch.cuda.synchronize()
    rc, n_out, counts = raw_view(hiplib, M, views, [raw.record(api)], [S["camera"]], (w, h), 2, mode, slack=slack, observed=[depth_image(api, d_obs)], carve=[carve.data_ptr()])
    assert rc == 0, api.load_library().cvo_last_error()
    torch.cuda.synchronize()
    assert n_out[0] == want["n_out"]                                   # the full row count
    for key, dt in (("xyz", np.float32), ("feat", np.float32), ("source", np.int32), ("pixel", np.int32), ("relation", np.int32)):
        assert raw.host(key, dt).tobytes() == want[key][:cap].tobytes(), key
    assert raw.host("map", np.int32).tobytes() == want["map"].tobytes() and want["map"].max() == want["n_out"] - 1   # full row numbers
    assert raw.host("depth", np.float32).tobytes() == want["depth"].tobytes() and raw.host("index", np.int32).tobytes() == want["index"].tobytes()
    assert counts[0].tolist() == want["relation_counts"].tolist() and counts[0].sum() == want["n_out"]   # over all rows, those past cap too
    assert host(carve)[:3000].tobytes() == want["carve"].tobytes() and (host(carve)[3000:] == 0xA5).all() and raw.guards_intact()
    with pytest.raises(hiplib.CvoError, match="more than cap 100"):
        M.view([k], [pose], S["camera"], (w, h), 2, mode, slack, cap=100)
    # cap = 0: counts only; one image may still be asked for; every array NULL gives the count alone
    only = Raw(torch, 0, 3000, (w // 2) * (h // 2), arrays=("depth",))
    rc, n_out, counts = raw_view(hiplib, M, views, [only.record(api)], [S["camera"]], (w, h), 2, mode, slack=slack, want_counts=False)
    assert rc == 0 and n_out[0] == want["n_out"]
    torch.cuda.synchronize()
    assert only.host("depth", np.float32).tobytes() == want["depth"].tobytes() and only.guards_intact()
    counted = M.view([k], [pose], S["camera"], (w, h), 2, mode, slack, cap=0, want=("depth",))[0]
    assert counted["n_out"] == want["n_out"] and counted["xyz"].shape[0] == 0 and host(counted["depth"]).tobytes() == want["depth"].tobytes()
    rc, n_out, counts = raw_view(hiplib, M, views, [api.ViewedCloud()], [S["camera"]], (w, h), 2, mode, slack=slack)
    assert rc == 0 and n_out[0] == want["n_out"] and counts[0].tolist() == [0, 0, 0, 0]


def test_refusals_change_nothing(hiplib, torch, reducer, lattices):
    api = hiplib.api
    S = lattices["small"]
    cam, M = S["camera"], S["M"]
    k = S["of"][3000]
    good = a_view(api, k, S["poses"][0])
    raws = [Raw(torch, 300, 3000, 64 * 48) for _ in range(3)]
    recs = [r.record(api, relation=None) for r in raws]
    r0 = raws[0]
    carve = torch.full((3000,), 0xA5, dtype=torch.uint8, device="cuda")
    def posed(i, val):
        v = a_view(api, k, S["poses"][0]); v.pose[i] = val; return v
    host_out = np.full(12 * 300, 0x5A, np.uint8); host_carve = np.full(3000, 0x5A, np.uint8)
    d_obs = torch.zeros((48, 64), dtype=torch.int16, device="cuda")
    hip = loaded_hip()                                                  # an allocation of the runtime's own, so that its end is known
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; hip.hipFree.argtypes = [C.c_void_p]
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), 2999) == 0                     # a byte short of the map's carve bytes; far short of its map entries
    ok_obs = [depth_image(api, d_obs)]
    nan, inf = float("nan"), float("inf")
    one = [good]
    many = len(vw.SCENE_SIZES)
    cases = [("null object", one, recs[:1], dict(handle=False)), ("views 0", one, recs[:1], dict(count=0)), ("views 17", [good] * 17, recs[:1] * 17, {}),
             ("map -1", [a_view(api, -1, EYE)], recs[:1], {}), (f"map {many}", [good, a_view(api, many, EYE)], recs[:2], {}),
             ("min_views 65", [a_view(api, k, EYE, mv.filter_of(1, 65, 0))], recs[:1], {}), ("min_views -1", [good, a_view(api, k, EYE, mv.filter_of(1, -1, 0))], recs[:2], {}),
             ("z-cells > max_points", one, recs[:1], dict(size=(256, 256))), ("width 0", one, recs[:1], dict(size=(0, 48))), ("height 8193", one, recs[:1], dict(size=(1, 8193), cell=16)),
             ("cell 0", one, recs[:1], dict(cell=0)), ("cell 17", one, recs[:1], dict(cell=17)), ("mode 2", one, recs[:1], dict(mode=2)),
             ("z_near 0", one, recs[:1], dict(z_near=0.0)), ("z_near NaN", one, recs[:1], dict(z_near=nan)), ("z_far = z_near", one, recs[:1], dict(z_near=1.0, z_far=1.0)),
             ("z_far above 32768", one, recs[:1], dict(z_far=32769.0)), ("slack negative", one, recs[:1], dict(slack=-0.1)), ("slack inf", one, recs[:1], dict(slack=inf)),
             ("depth_tol NaN", one, recs[:1], dict(depth_tol=nan)), ("pose NaN", [posed(7, nan)], recs[:1], {}), ("pose inf", [good, posed(0, inf)], recs[:2], {}),
             ("camera index -1", [a_view(api, k, EYE, cam=-1)], recs[:1], {}), ("camera fx NaN", one, recs[:1], dict(cams=[(5000.0, nan, 57.1, 31.2, 23.7)])),
             ("camera fy 0", one, recs[:1], dict(cams=[(5000.0, 58.3, 0.0, 31.2, 23.7)])), ("camera scaling_factor 0", one, recs[:1], dict(cams=[(0.0, 58.3, 57.1, 31.2, 23.7)])),
             ("pageable output", one, [r0.record(api, relation=None, xyz=host_out.ctypes.data)], {}), ("cap 65536", one, [r0.record(api, relation=None, cap=65536)], {}),
             ("cap -1", one, [r0.record(api, relation=None, cap=-1)], {}), ("null xyz with cap", one, [r0.record(api, relation=None, xyz=None)], {}),
             ("null feat with cap", one, [r0.record(api, relation=None, feat=None)], {}),
             ("pixel 2 bytes off", one, [r0.record(api, relation=None, pixel=r0.t["pixel"].data_ptr() + 2)], {}),
             ("map too short", one, [r0.record(api, relation=None, map=short.value)], {}), ("index too short", one, [r0.record(api, relation=None, index=short.value)], {}),
             ("relation without observed", one, [r0.record(api)], {}), ("carve without observed", one, recs[:1], dict(carve=[carve.data_ptr()])),
             ("carve pageable", one, recs[:1], dict(observed=ok_obs, carve=[host_carve.ctypes.data])), ("carve too short", one, recs[:1], dict(observed=ok_obs, carve=[short.value])),
             ("observed depth16 null", one, recs[:1], dict(observed=[api.DeviceImage(None, None, 0, 0, 3, 0)])),
             ("observed pitch odd", one, recs[:1], dict(observed=[depth_image(api, d_obs, 129)])),
             ("observed rows outside the allocation", one, recs[:1], dict(observed=[api.DeviceImage(None, short.value, 0, 0, 3, 0)]))]
    before = snapshot(M, None)
    torch.cuda.synchronize()
    msg = lambda: api.load_library().cvo_last_error().decode()
    for what, views, out, kw in cases:
        kw = dict(kw)
        cams = kw.pop("cams", [cam])
        for check_only in (True, False):
            rc, n_out, counts = raw_view(hiplib, M, views, out, cams, check_only=check_only, **kw)
            assert rc == INVALID, what
            assert msg(), what
            assert (n_out == -7).all() and (counts == -7).all(), what
        torch.cuda.synchronize()
        assert all(r.untouched() for r in raws) and (host(carve) == 0xA5).all(), what
        assert (host_out == 0x5A).all() and (host_carve == 0x5A).all(), what
    # null arguments, one at a time
    arr = (api.MapView * 1)(good); cs = (api.Camera * 1)(api.Camera(*cam)); prm = api.ViewParams(64, 48, 1, 0, 0.05, 30.0, 0.0, 0.02)
    out = (api.ViewedCloud * 1)(recs[0]); n_out = np.full(1, -7, np.int32)
    ip = n_out.ctypes.data_as(C.POINTER(C.c_int))
    for args in ((None, cs, C.byref(prm), None, out), (arr, None, C.byref(prm), None, out), (arr, cs, None, None, out), (arr, cs, C.byref(prm), None, None)):
        assert M.L.cvo_check_maps_view(M.h, 1, *args, None) == INVALID and "null argument" in msg()
        assert M.L.cvo_maps_view(M.h, 1, *args, None, ip, None, None) == INVALID and "null argument" in msg()
    assert M.L.cvo_maps_view(M.h, 1, arr, cs, C.byref(prm), None, out, None, None, None, None) == INVALID and "n_out" in msg()
    torch.cuda.synchronize()
    assert n_out[0] == -7 and all(r.untouched() for r in raws)
    unchanged(M, None, before)                                          # every map byte-identical
    # the messages name view and field
    raw_view(hiplib, M, [good, a_view(api, many, EYE)], [api.ViewedCloud()] * 2, [cam])
    assert "view 1" in msg() and f"map {many}" in msg()
    raw_view(hiplib, M, [good, good, posed(7, nan)], [api.ViewedCloud()] * 3, [cam])
    assert "view 2" in msg() and "pose[7]" in msg()
    raw_view(hiplib, M, [good, a_view(api, k, EYE, mv.filter_of(1, 65, 0))], [api.ViewedCloud()] * 2, [cam])
    assert "view 1" in msg() and "min_views 65" in msg()
    raw_view(hiplib, M, [good, good], [api.ViewedCloud()] * 2, [cam], observed=ok_obs * 2, carve=[None, short.value])
    assert "view 1" in msg() and "carve" in msg()
    raw_view(hiplib, M, one, [api.ViewedCloud()], [cam], carve=[carve.data_ptr()])
    assert "carve" in msg() and "observed" in msg()
    hip.hipFree(short)
    # a map may repeat, and carve[k] may be NULL where another view has one
    rc, n_out, counts = raw_view(hiplib, M, [good, good], [api.ViewedCloud()] * 2, [cam], observed=ok_obs * 2, carve=[None, carve.data_ptr()])
    assert rc == 0 and n_out[0] == n_out[1] > 0, msg()
    torch.cuda.synchronize()
    assert set(np.unique(host(carve)).tolist()) <= {0, 1}
    # python's refusals come first; the library's come up as CvoError
    with pytest.raises(hiplib.CvoError, match="z-cells"):
        M.check_view([k], [EYE], cam, (256, 256))
    M.check_view([k, k], [EYE, EYE], cam, (64, 48), observed=[d_obs, d_obs], min_views=[0, 64])
    unchanged(M, None, before)


# ---- 10. the stream rule
def test_stream_orders_map_writes_observed_and_output(hiplib, torch, reducer, window):
    members, poses = window[0][:4], window[1][:4]
    R = mr.Map(MAX_ROWS, 0.05); R.update(members, poses, [0, 1, 2, 3])
    flt = mv.filter_of(1, 2, 0)
    E = R.extract(**flt)
    obs = vw.shifted_rendering((E["xyz"], E["feat"]), EYE, SHEET_CAM, (64, 48))
    want = mv.map_view_reading(R, flt, EYE, SHEET_CAM, vw.params(64, 48, 2, vw.SURFACE, 0.05), obs, E=E)
    keys = KEYS + ("relation", "carve")
    side = torch.cuda.Stream()
    pinned = [(torch.from_numpy(x).pin_memory(), torch.from_numpy(f).pin_memory()) for x, f in members]
    ho = torch.from_numpy(obs.view(np.int16)).pin_memory()
    tens = [(torch.full(x.shape, 1000.0, dtype=torch.float32, device="cuda"), torch.zeros(f.shape, dtype=torch.float32, device="cuda"), "points_first") for x, f in members]
    to = torch.zeros(obs.shape, dtype=torch.int16, device="cuda")
    a = torch.randn((4096, 4096), device="cuda")
    M = hiplib.CvoMaps(reducer, 1, MAX_ROWS, 0.05)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):                                             # work in front of the writes: without the edge in, the kernels would read the 1000s and the 0s
            a = a @ a * 1e-3
        for (tx, tf, _), (hx, hf) in zip(tens, pinned):
            tx.copy_(hx, non_blocking=True); tf.copy_(hf, non_blocking=True)
        to.copy_(ho, non_blocking=True)
    M.integrate([0], [tens], [poses], [[0, 1, 2, 3]], cloud_stream=side)      # the merge is still queued on the reducer's stream when this returns
    got = M.view([0], [EYE], SHEET_CAM, (64, 48), 2, "surface", 0.05, observed=[to], want=ALL, carve=True, stream=side, **per_view([flt]))[0]
    with torch.cuda.stream(side):                                      # a read queued on that stream behind the call, and an overwrite behind the read
        snap = {k: got[k].clone() for k in keys}
        to.zero_()
        for k in keys:
            got[k].zero_()
    side.synchronize()
    same(dict(snap, n_out=got["n_out"], relation_counts=got["relation_counts"]), want, "side stream", keys)
    # NULL: everything is done on return
    again = M.view([0], [EYE], SHEET_CAM, (64, 48), 2, "surface", 0.05, observed=[up_depth(torch, obs)], want=ALL, carve=True, **per_view([flt]))[0]
    same(again, want, "no stream", keys)
    M.close()


# ---- 11. one reducer; 12. the table's size does not show
def test_reduce_fuse_view_maps_and_map_views_interleaved_on_one_reducer(hiplib, torch, reducer, window):
    members, poses = window[0][:4], window[1][:4]
    tens = dev(torch, members)
    M = hiplib.CvoMaps(reducer, 2, MAX_ROWS, 0.05)
    R = mr.Map(MAX_ROWS, 0.05)
    scratch = reducer.scratch_bytes()
    for t in range(4):
        M.integrate([1], [[tens[t]]], [[poses[t]]], [[t]]); R.update([members[t]], [poses[t]], [t])
        p = vw.params(64, 48, 2, vw.SURFACE, 0.05)
        same(M.view([1], [EYE], SHEET_CAM, (64, 48), 2, "surface", 0.05, want=WANT)[0], mv.map_view_reading(R, LOOSE, EYE, SHEET_CAM, p), (t, "before"))
        g = reducer.reduce([tens[t]], 0.05, "mean", 1, want=("count",))[0]
        w = vr.reduce_reading(members[t][0], members[t][1], 0.05, "mean", 1)
        assert g["n_out"] == w["n_out"] and host(g["xyz"]).tobytes() == w["xyz"].tobytes()
        f = reducer.fuse([tens[:t + 1]], [poses[:t + 1]], 0.05, want=("count",))[0]
        assert f["n_out"] == fr.fuse_reading(members[:t + 1], poses[:t + 1], 0.05)["n_out"]
        e = M.extract([1], want=("row",))[0]
        v = reducer.view([(e["xyz"], e["feat"], "points_first")], [EYE], SHEET_CAM, (64, 48), 2, "surface", 0.05, want=("source",))[0]
        got = M.view([1, 1], [EYE, poses[t]], SHEET_CAM, (64, 48), 2, "surface", 0.05, want=WANT)
        same(got[0], mv.map_view_reading(R, LOOSE, EYE, SHEET_CAM, p), (t, "after"))
        same(got[1], mv.map_view_reading(R, LOOSE, poses[t], SHEET_CAM, p), (t, "posed"))
        assert host(v["xyz"]).tobytes() == host(got[0]["xyz"]).tobytes() and v["n_out"] > 100
    assert reducer.scratch_bytes() == scratch
    M.close()


def test_two_table_sizes_give_the_same_bytes(hiplib, torch, reducer, window):
    members, poses = window
    tens = dev(torch, members)
    runs = []
    obs = None
    for max_rows in (MAX_ROWS, 7000):                                  # another table size: another layout, which must not show
        M = hiplib.CvoMaps(reducer, 1, max_rows, 0.05)
        for t in range(6):
            M.integrate([0], [[tens[t]]], [[poses[t]]], [[t]])
            if t >= 2:
                M.remove([0], [[tens[t - 2]]], [[poses[t - 2]]], [[t - 2]])
        M.compact([0], min_views=2, probation_from=5)
        M.integrate([0], [tens[6:8]], [poses[6:8]], [[6, 7]])
        if obs is None:
            R = mr.Map(MAX_ROWS, 0.05)                                  # the same history in the reading
            for t in range(6):
                R.update([members[t]], [poses[t]], [t])
                if t >= 2:
                    R.update([members[t - 2]], [poses[t - 2]], [t - 2], -1)
            R.compact(min_views=2, probation_from=5)
            R.update(members[6:8], poses[6:8], [6, 7])
            E = R.extract(1, 2, 6)
            obs = vw.shifted_rendering((E["xyz"], E["feat"]), EYE, SHEET_CAM, (64, 48))
        got = M.view([0], [EYE], SHEET_CAM, (64, 48), 1, "surface", 0.05, observed=[up_depth(torch, obs)], want=ALL, carve=True, min_views=2, min_last_stamp=6)[0]
        runs.append({k: (host(v).copy() if hasattr(v, "cpu") else v) for k, v in got.items()})
        M.close()
    want = mv.map_view_reading(R, mv.filter_of(1, 2, 6), EYE, SHEET_CAM, vw.params(64, 48, 1, vw.SURFACE, 0.05), obs)
    assert want["n_out"] > 100 and (want["map"] == mv.FILTERED).any()
    for run in runs:
        same(run, want, "table size", KEYS + ("relation", "carve"))


# ---- 13. end to end
def test_a_viewed_map_aligns_like_the_reading_s_rows(hiplib, torch):
    from cvo_slam_amd import synth
    from cvo_slam_amd.voxels import view_cell_for_budget
    frames, cam_poses = synth.make_sequence(0, 5)
    clouds = []
    for bgr, dep in frames:
        c = synth.dense_cloud(bgr, dep, synth.TUM1)
        pick = np.unique(np.linspace(0, c.n - 1, 5000).astype(np.int64))
        clouds.append((np.ascontiguousarray(c.xyz[pick]), np.ascontiguousarray(c.feat[:, pick].T)))
    poses = [(np.linalg.inv(cam_poses[3]) @ cam_poses[k]).astype(np.float32) for k in range(4)]   # keyframe k in the newest keyframe's frame
    T = synth.TUM1
    cam = (T["depth_factor"], T["fx"], T["fy"], T["cx"], T["cy"])
    Rd = hiplib.CvoReducer(2, 20000)
    M = hiplib.CvoMaps(Rd, 1, 20000, 0.04)
    R = mr.Map(20000, 0.04)
    tens = dev(torch, clouds[:4])
    for t in range(4):
        M.integrate([0], [[tens[t]]], [[poses[t]]], [[t]]); R.update([clouds[t]], [poses[t]], [t])
    predicted = (np.linalg.inv(cam_poses[4]) @ cam_poses[3]).astype(np.float32)      # the map's frame moved into camera 4's predicted frame
    cell = view_cell_for_budget(T["w"], T["h"], 3072)
    flt = mv.filter_of(1, 2, 0)
    got = M.view([0], [predicted], cam, (T["w"], T["h"]), cell, "front", want=("source", "pixel", "map"), **per_view([flt]))[0]
    want = mv.map_view_reading(R, flt, predicted, cam, vw.params(T["w"], T["h"], cell, vw.FRONT))
    same(got, want, "viewed map", ("xyz", "feat", "source", "pixel", "map"))
    assert 300 < want["n_out"] <= 3072 and (want["map"] == -1).any() and (want["map"] == mv.FILTERED).any()
    moving = Rd.reduce([dev(torch, clouds[4:])[0]], 0.04, "mean", 1, want=())[0]
    B = hiplib.CvoBatch(1)
    B.set_pairs_clouds([(got["xyz"], got["feat"], "points_first"), (moving["xyz"], moving["feat"], "points_first")], [0], [1])   # the viewed rows as they are
    B.align_async(1)
    res = B.wait(1)[0]
    Bh = hiplib.CvoBatch(1)
    Bh.set_pairs([(want["xyz"], np.ascontiguousarray(want["feat"].T), host(moving["xyz"]), np.ascontiguousarray(host(moving["feat"]).T))])
    ref = Bh.align(1)[0]
    assert res["status"] == 0 and ref["status"] == 0
    assert res["transform"].tobytes() == ref["transform"].tobytes() and res["ell"] == ref["ell"] and res["iter"] == ref["iter"]
    B.close(); Bh.close(); M.close(); Rd.close()
