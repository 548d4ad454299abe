"""tests/view_reading.py holds the definition of a view (cvo_hip.h, "Viewing clouds"); this file holds the reading: against a plain python loop
that follows the header sentence by sentence, against the frames whose dense clouds must reproject onto their own pixels, and to the scene
conditions without which a GPU comparison would be about nothing.  No GPU."""
import numpy as np
import pytest

import frame_reading as frd
import fuse_reading as fr
import pcd_cases as pc
import view_reading as vw

f32 = np.float32


def loop_reading(cloud, pose, camera, p, observed=None):
    """the header's sentences, a point at a time, in float32 scalars; a dict per z-cell"""
    x, f = cloud
    M = fr.pose34(pose)
    s, fx, fy, cx, cy = (f32(v) for v in camera)
    n = x.shape[0]
    gw, gh = vw.grid(p)
    moved, code, pix = [], [], []
    fronts = {}
    lim = f32(32768.0)
    with np.errstate(all="ignore"):
        for i in range(n):
            w = [(M[r, 0] * x[i, 0] + (M[r, 1] * x[i, 1] + M[r, 2] * x[i, 2])) + M[r, 3] for r in range(3)]
            moved.append(w)
            vals = [x[i, 0], x[i, 1], x[i, 2]] + list(f[i]) + w
            if not all(abs(v) < lim for v in vals):
                code.append(-3); pix.append(None); continue
            z = w[2]
            if not (p["z_near"] <= z and z <= p["z_far"]):
                code.append(-2); pix.append(None); continue
            u = (w[0] * fx) / z + cx
            v = (w[1] * fy) / z + cy
            if not (abs(u) < f32(1048576.0) and abs(v) < f32(1048576.0)):
                code.append(-2); pix.append(None); continue
            px = int(np.floor(u + f32(0.5))); py = int(np.floor(v + f32(0.5)))
            if not (0 <= px < p["width"] and 0 <= py < p["height"]):
                code.append(-2); pix.append(None); continue
            c = (px // p["cell"], py // p["cell"])
            code.append(c); pix.append((px, py))
            key = (int(np.array([z], f32).view(np.uint32)[0]) << 32) | i
            cellrec = fronts.setdefault(c, dict(key=key))
            if key < cellrec["key"]:
                cellrec["key"] = key
        rows = []
        for i in range(n):
            if not isinstance(code[i], tuple):
                continue
            key = fronts[code[i]]["key"]
            if p["mode"] == vw.FRONT:
                seen = (key & 0xFFFFFFFF) == i
            else:
                zf = np.array([key >> 32], np.uint32).view(f32)[0]
                seen = moved[i][2] <= zf + p["slack"] * zf
            if seen:
                rows.append(i)
        m = np.array([c if not isinstance(c, tuple) else -1 for c in code], np.int32).reshape(n)
        m[rows] = np.arange(len(rows), dtype=np.int32)
        depth = np.zeros((gh, gw), f32); index = np.full((gh, gw), -1, np.int32)
        for (cxx, cyy), rec in fronts.items():
            depth[cyy, cxx] = np.array([rec["key"] >> 32], np.uint32).view(f32)[0]; index[cyy, cxx] = rec["key"] & 0xFFFFFFFF
        out = dict(xyz=np.array([moved[i] for i in rows], f32).reshape(-1, 3), feat=np.ascontiguousarray(f[rows]).reshape(-1, 5), source=np.array(rows, np.int32),
                   pixel=np.array([pix[i][1] * p["width"] + pix[i][0] for i in rows], np.int32), map=m, depth=depth, index=index, n_out=len(rows))
        if observed is not None:
            rel = []
            for i in rows:
                d = int(observed[pix[i][1], pix[i][0]])
                zo = f32(d) / s; t = p["depth_tol"] * zo; z = moved[i][2]
                rel.append(0 if d == 0 else 1 if z < zo - t else 3 if z > zo + t else 2)
            out["relation"] = np.array(rel, np.int32)
            out["relation_counts"] = np.array([rel.count(k) for k in range(4)], np.int32)
    return out


def same(a, b, what):
    assert a["n_out"] == b["n_out"], what
    for key in b:
        if key == "n_out":
            continue
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, (what, key, a[key].dtype, a[key].shape, b[key].shape)
        assert a[key].tobytes() == b[key].tobytes(), (what, key)


@pytest.mark.parametrize("cell", [1, 3, 16])
@pytest.mark.parametrize("mode,slack", [(vw.FRONT, 0.0), (vw.SURFACE, 0.0), (vw.SURFACE, 0.05)], ids=["front", "surface_0", "surface_5pc"])
def test_the_reading_is_the_header_s_sentences(cell, mode, slack):
    rng = np.random.default_rng(5)
    for n in (0, 1, 64, 300):
        cloud = vw.two_walls(rng, n, vw.CAM_SMALL, vw.SIZE_SMALL)
        pose = fr.rigid(rng, 0.03, 0.05)
        if n == 300:                                                   # three points of one pixel and one depth: the lowest index is the front
            first = int(np.flatnonzero(vw.view_reading(cloud, pose, vw.CAM_SMALL, vw.params(*vw.SIZE_SMALL))["map"] >= -1)[0])
            assert first < 100
            cloud[0][200] = cloud[0][first]; cloud[0][100] = cloud[0][first]
        p = vw.params(*vw.SIZE_SMALL, cell, mode, slack)
        same(vw.view_reading(cloud, pose, vw.CAM_SMALL, p), loop_reading(cloud, pose, vw.CAM_SMALL, p), (n, "no observed"))
        obs = vw.shifted_rendering(cloud, pose, vw.CAM_SMALL, vw.SIZE_SMALL)
        got = vw.view_reading(cloud, pose, vw.CAM_SMALL, p, obs)
        same(got, loop_reading(cloud, pose, vw.CAM_SMALL, p, obs), (n, "observed"))
        if n == 300:
            gw, gh = vw.grid(p)
            assert got["n_out"] >= min(12, gw * gh) and (got["map"] == -2).any() and (got["map"] == -3).any()
            assert cell == 1 or (got["map"] == -1).any()               # (300 points on 3072 pixels hide little at cell 1)
            assert mode != vw.FRONT or got["n_out"] == (got["index"] >= 0).sum() <= gw * gh
            if mode == vw.FRONT:
                assert got["map"][100] == -1 and got["map"][200] == -1  # the later twins are never the front
            else:
                assert (got["map"][100] >= 0) == (got["map"][first] >= 0) == (got["map"][200] >= 0)   # one depth: seen or hidden together


@pytest.mark.parametrize("size,family,cam", [((64, 64), "noise", pc.CAMERA), ((100, 70), "checker", pc.CAMERA_B), ((185, 114), "smooth", pc.CAMERA)],
                         ids=["64x64", "100x70", "185x114"])
def test_a_frame_s_dense_cloud_reprojects_onto_its_own_pixels(size, family, cam):
    """the dense clouds of tests/frame_reading.py (held to the oracle by tests/test_frame_reading.py), viewed under the identity with their own
    camera at cell 1 in FRONT: every point with depth is visible at its own pixel with its own z, and agrees with its own depth"""
    w, h = size
    bgr, dep = pc.image(w, h, family, {"checker": 3, "smooth": 40}.get(family)), pc.depth(w, h, "holes")
    xyz, feat = frd.dense_reading(bgr, dep, cam)
    has = np.flatnonzero(dep.reshape(-1) != 0)
    assert 0 < has.shape[0] < w * h
    got = vw.view_reading((xyz, feat), np.eye(4, dtype=f32), cam, vw.params(w, h, 1, vw.FRONT, z_near=0.05, z_far=30.0), dep)
    assert got["n_out"] == has.shape[0]
    assert np.array_equal(got["source"], has) and np.array_equal(got["pixel"], has)      # every point with depth, at its own flat index
    z = np.where(dep != 0, xyz[:, 2].reshape(h, w), f32(0.0)).astype(f32)
    assert got["depth"].tobytes() == z.tobytes()                                         # the frame's z, bit for bit; 0 where it has none
    assert np.array_equal(got["index"].reshape(-1), np.where(dep.reshape(-1) != 0, np.arange(w * h), -1))
    assert (got["relation"] == 2).all() and got["relation_counts"].tolist() == [0, 0, has.shape[0], 0]
    assert got["xyz"].tobytes() == xyz[has].tobytes()                                    # (no coordinate is -0.0: the identity move keeps the bits)
    assert (got["map"][dep.reshape(-1) == 0] == -3).all()                                # no depth: NaN, invalid


@pytest.mark.parametrize("which", ["small", "wide"])
def test_the_scenes_of_the_gpu_tests_have_something_to_compare(which):
    """Every two_walls scene the GPU tests use, under each pose it is used with.  The shares are taken where the walls decide them -- SURFACE,
    slack 0.05, cell 3 (view_reading.SHARES_AT) -- and over the 3000-point scenes: a cloud of 1 .. 257 points has too few points for a share of
    hidden, outside and invalid points each (a single point is one of the three), so the small clouds ride on the same generator and of
    them is asserted what can hold: rows, outside and invalid points, and hidden points at the coarsest cell."""
    S = vw.scene(which)
    cloud = S["clouds"][3000]
    p = vw.params(*S["size"], **vw.SHARES_AT)
    used = sorted({k for call in vw.SCENE_CALLS for k, n in enumerate(call) if n == 3000})
    assert len(used) >= 2
    for k in used:
        hidden, outside, invalid = vw.shares(cloud, S["poses"][k], S["camera"], p)
        assert 0.2 <= hidden <= 0.6, (which, k, hidden)
        assert outside >= 0.05 and invalid >= 0.01, (which, k, outside, invalid)
    # the relation test: the scene's own rendering, shifted by bands of columns
    pose = S["poses"][used[0]]
    obs = vw.shifted_rendering(cloud, pose, S["camera"], S["size"])
    for mode, slack, cell in ((vw.FRONT, 0.0, 1), (vw.SURFACE, 0.05, 2)):
        r = vw.view_reading(cloud, pose, S["camera"], vw.params(*S["size"], cell, mode, slack), obs)
        assert r["relation_counts"].sum() == r["n_out"] > 200
        assert (r["relation_counts"] >= 0.02 * r["n_out"]).all(), (which, mode, r["relation_counts"])
    assert set(vw.SCENE_SIZES) == {n for call in vw.SCENE_CALLS for n in call}
    # the clouds of 63 .. 257 points, which carry the wave-edge and block-edge comparisons, under each pose they are used with: what can hold
    # of so few points does -- rows, points outside and invalid points at every cell, hidden points at the coarsest cell in both modes
    for call in vw.SCENE_CALLS:
        for k, n in enumerate(call):
            if not 63 <= n <= 257:
                continue
            for cell, mode, slack in ((1, vw.FRONT, 0.0), (16, vw.FRONT, 0.0), (16, vw.SURFACE, 0.05)):
                r = vw.view_reading(S["clouds"][n], S["poses"][k], S["camera"], vw.params(*S["size"], cell, mode, slack))
                assert r["n_out"] >= 10 and (r["map"] == -2).sum() >= 0.05 * n and (r["map"] == -3).sum() >= 2, (which, k, n, cell, mode)
                assert cell == 1 or (r["map"] == -1).sum() >= 5, (which, k, n, cell, mode)


def test_the_edge_cloud_sits_on_the_edges_it_names():
    """view_reading.edge_cloud, which the GPU tests compare on: each point's code in the reading is what its name says"""
    x, f, names = vw.edge_cloud()
    eye = np.eye(4, dtype=f32)
    code = lambda pose, **kw: vw.view_reading((x, f), pose, vw.EDGE_CAM, vw.params(*vw.EDGE_SIZE, **kw))
    front = code(eye)
    seen = lambda m: ["in" if c >= 0 else {-1: "hidden", -2: "out", -3: "invalid"}[c] for c in m.tolist()]
    want = ["in", "out", "out", "in", "in", "out", "out", "in", "in", "out", "in", "out", "in", "hidden", "hidden", "hidden", "out", "out",
            "invalid", "invalid", "out", "in"]
    assert len(names) == len(want) == x.shape[0] and seen(front["map"]) == want
    assert front["pixel"].tolist() == [24 * 64 + 0, 24 * 64 + 63, 0 * 64 + 48, 47 * 64 + 48, 24 * 64 + 32, 24 * 64 + 40, 27 * 64 + 35, 18 * 64 + 48]
    assert front["index"][27, 35] == 12 and front["depth"][27, 35] == 2.0   # of the twins the lower index
    s0 = seen(code(eye, mode=vw.SURFACE)["map"])
    assert s0 == want[:13] + ["in"] + want[14:]                        # slack 0: the twin of the front, nothing else
    s5 = seen(code(eye, mode=vw.SURFACE, slack=0.05)["map"])
    assert s5 == want[:13] + ["in", "hidden", "in"] + want[16:]        # 2.05 <= 2 + 0.05 * 2 (2.1), 2.5 is not
    tiny = code(eye, z_near=1e-6)
    assert seen(tiny["map"]) == want[:8] + ["hidden", "hidden"] + want[10:16] + ["out", "in"] + want[18:]   # |u| past 2^20; the axis point hides z_near's
    assert tiny["index"][24, 32] == 17
    far = seen(code(vw.EDGE_FAR_MOVE)["map"])
    assert far[20] == "invalid" and far[21] == "out" and far[16] == "invalid" and far[0] == "out" and "in" not in far
