"""Loop-closure batches built from RGB-D images (cvo_batch_set_pairs_images): every distinct image generated once by the batched GPU
generator, makeMaps decided per image on the device.  The clouds must be IDENTICAL to the oracle's pcd_generate and to the handle path's
(cvo_set_pcd_images), and everything after the hand-over must behave as with clouds handed in by cvo_batch_set_pairs."""
import ctypes as C

import numpy as np
import pytest

from helpers import make_tf, rot_trans_err

pytestmark = pytest.mark.gpu

FIXED, MOVING = 0, 1


def camera(shape):
    from cvo_slam_amd import synth
    return synth.TUM1 if shape == "tum" else synth.ETH3D


def frame_images(indices, cam):
    from cvo_slam_amd import synth
    out = []
    for i in indices:
        (fa, da), (fb, db), _ = synth.make_frames(i, cam=cam)
        out += [(fa, da), (fb, db)]
    return out


def assert_cloud(B, p, slot, want):
    xyz, feat = B.get_cloud(p, slot)
    px = B.get_selected_points(p, slot)
    assert xyz.shape[0] == want["n"], (p, slot)
    np.testing.assert_array_equal(px, want["px"])
    np.testing.assert_array_equal(xyz, want["xyz"])
    np.testing.assert_array_equal(feat, want["feat"])


def result_key(r):
    return (r["transform"].tobytes(), r["R"].tobytes(), r["T"].tobytes(), r["ell"], r["iter"], r["A_nonzero"], r["iterations_run"], r["status"],
            r["rebuilds"], r["dense_fallbacks"])


@pytest.mark.parametrize("num_want", [300, 3000, 12000])
@pytest.mark.parametrize("shape", ["tum", "eth3d"])
def test_clouds_identical_to_oracle_and_handle_path(hiplib, oracle, shape, num_want):
    from cvo_slam_amd import synth
    cam = camera(shape); camt = synth.camera_tuple(cam)
    images = frame_images([0, 2, 3] if shape == "tum" else [1, 2, 3], cam)     # 6 different images of one size
    B = hiplib.CvoBatch(4); B.set_num_want(num_want)
    fixed, moving = [0, 2, 4, 5], [1, 3, 5, 0]
    pts = B.set_pairs_images(images, fixed, moving, camt)
    want = [oracle.pcd_generate(b, d, camt, num_want=num_want, cap=40000) for b, d in images]
    assert list(pts) == [w["n"] for w in want]
    for p in range(4):
        assert_cloud(B, p, FIXED, want[fixed[p]]); assert_cloud(B, p, MOVING, want[moving[p]])
    g = hiplib.Cvo(); g.set_num_want(num_want)                      # the handle path, image by image (first call: FIXED, later ones: MOVING)
    for k, (b, d) in enumerate(images):
        g.set_pcd_images(b, d, camt)
        slot = FIXED if k == 0 else MOVING
        p = fixed.index(k) if k in fixed else moving.index(k)
        got = B.get_cloud(p, FIXED if k in fixed else MOVING)
        hx, hf = g.get_cloud(slot)
        np.testing.assert_array_equal(got[0], hx); np.testing.assert_array_equal(got[1], hf)
        np.testing.assert_array_equal(B.get_selected_points(p, FIXED if k in fixed else MOVING), g.get_selected_points(slot))
    g.close(); B.close()


def test_each_image_takes_its_own_makemaps_decisions(hiplib, oracle):
    """One call mixes every branch of makeMaps: a frame that keeps its first selection, frames that select again, a flat image (nothing
    selected: empty cloud) and a textured frame without depth (pixels selected, no points)."""
    from cvo_slam_amd import synth
    camt = synth.camera_tuple(synth.TUM1); num_want = 12000
    (t0, d0), _, _ = synth.make_frames(0, cam=synth.TUM1)
    (t3, d3), (t3b, d3b), _ = synth.make_frames(3, cam=synth.TUM1)
    flat = np.full_like(t0, 90); flat_d = np.full_like(d0, 5000)
    images = [(t0, d0), (t3, d3), (flat, flat_d), (t3b, np.zeros_like(d3b)), (t3b, d3b)]
    want = [oracle.pcd_generate(b, d, camt, num_want=num_want, cap=40000, debug=True) for b, d in images]
    pots = [int(w["info"][0]) for w in want]
    assert pots[0] != 3 and pots[1] == 3 and pots[2] == 1, pots      # the premise: re-selection, none, the empty image's re-selection
    assert want[2]["n"] == 0 and want[3]["n"] == 0 and int(want[3]["info"][1]) > 0
    fixed, moving = [0, 1, 2, 0, 3, 4], [1, 0, 1, 3, 3, 1]
    B = hiplib.CvoBatch(len(fixed)); B.set_num_want(num_want); B.set_workgroups(2)
    pts = B.set_pairs_images(images, fixed, moving, camt)
    assert list(pts) == [w["n"] for w in want]
    for p in range(len(fixed)):
        assert_cloud(B, p, FIXED, want[fixed[p]]); assert_cloud(B, p, MOVING, want[moving[p]])
    res = B.align(len(fixed))
    empty = [want[fixed[p]]["n"] == 0 or want[moving[p]]["n"] == 0 for p in range(len(fixed))]
    assert empty == [False, False, True, True, True, False]
    for p, r in enumerate(res):
        assert (r["status"] == hiplib.api.CVO_ERR_EMPTY_CLOUD) == empty[p], (p, r["status"])
    # the pairs with points align exactly as the same clouds handed in by cvo_batch_set_pairs, in a launch of the same shape
    B2 = hiplib.CvoBatch(len(fixed)); B2.set_workgroups(2)
    B2.set_pairs([(want[f]["xyz"], want[f]["feat"], want[m]["xyz"], want[m]["feat"]) for f, m in zip(fixed, moving)])
    res2 = B2.align(len(fixed))
    for p in range(len(fixed)):
        assert result_key(res[p]) == result_key(res2[p]), p
    B.close(); B2.close()


def test_loop_closure_from_images_end_to_end(hiplib, oracle):
    """keyframe_graph.cpp:693-717 from images: one reference frame listed once, 8 candidates of the same scene with known motions, priors
    within ~2 degrees / 3 cm of the truth (reset_initial), one align launch, one score launch; against oracle objects fed the oracle's clouds,
    and bit for bit against the same pairs handed over by cvo_batch_set_pairs with the handle path's clouds."""
    from cvo_slam_amd import synth
    camt = synth.camera_tuple(synth.TUM1)
    frames, poses = synth.make_sequence(4, n_frames=9, max_deg=1.2, max_trans=0.02)
    n = len(frames) - 1
    rng = np.random.default_rng(7)
    lc_priors = []
    for k in range(1, n + 1):
        d = np.eye(4); d[:3] = make_tf(rng.normal(size=3), np.deg2rad(rng.uniform(0.5, 2.0)), rng.normal(size=3) * 0.012)
        lc_priors.append((poses[k] @ d)[:3].astype(np.float32))
    lc_priors = np.stack(lc_priors)
    priors = np.stack([np.eye(3, 4, dtype=np.float32)] * n)
    clouds = [oracle.pcd_generate(b, d, camt) for b, d in frames]
    B = hiplib.CvoBatch(n)
    pts = B.set_pairs_images(frames, [0] * n, list(range(1, n + 1)), camt)
    assert list(pts) == [c["n"] for c in clouds]
    single = []
    for i in range(n):
        o = oracle.OracleCvo(search=oracle.SEARCH_KDTREE, threads=8)
        o.reset_initial(lc_priors[i])
        o.set_pcd(clouds[0]["xyz"], clouds[0]["feat"]); o.set_pcd(clouds[i + 1]["xyz"], clouds[i + 1]["feat"])
        st0 = o.get_state(); B.set_state(i, st0["R"], st0["T"], st0["ell"])
        single.append((o, st0))
    res = B.align(n)
    got = B.compute_innerproduct_lc(priors, lc_priors, lc_priors)
    for i, ((o, _), r, g) in enumerate(zip(single, res, got)):
        rc, _ = o.align(); assert rc == 0
        st = o.get_state()
        re, te = rot_trans_err(r["transform"], st["transform"])
        assert re <= 1e-6 and te <= 1e-6, (i, re, te)
        assert r["iter"] == st["iter"], (i, r["iter"], st["iter"])
        rc, want = o.compute_innerproduct_lc(priors[i], lc_priors[i], lc_priors[i], st["transform"]); assert rc == 0
        for key in ("inn_prior", "inn_lc_prior", "inn_lc_pre", "inn_lc_post", "inn_fixed_pcd", "inn_moving_pcd"):
            assert g[key][1] == want[key][1], (i, key)
            assert g[key][0] == pytest.approx(want[key][0], rel=1e-5), (i, key)
        assert (g["inliers_svd"], g["inliers_pnpransac"]) == (want["inliers_svd"], want["inliers_pnpransac"]), i
        post = want["inn_lc_post"][0]                                   # the reference's rule, keyframe_graph.cpp:711-712
        want_accept = not (post <= want["inn_lc_pre"][0] or post <= want["inn_lc_prior"][0] or post <= want["inn_prior"][0] or want["cos_angle"] < 0.1)
        assert g["accept"] == want_accept, i
    # the handle path: each frame through cvo_set_pcd_images and back to the host, then one cvo_batch_set_pairs
    g = hiplib.Cvo()
    host = []
    for k, (b, d) in enumerate(frames):
        g.set_pcd_images(b, d, camt)
        host.append(g.get_cloud(FIXED if k == 0 else MOVING))
    g.close()
    B2 = hiplib.CvoBatch(n)
    B2.set_pairs([(host[0][0], host[0][1], host[i][0], host[i][1]) for i in range(1, n + 1)])
    for i, (_, st0) in enumerate(single):
        B2.set_state(i, st0["R"], st0["T"], st0["ell"])
    res2 = B2.align(n)
    got2 = B2.compute_innerproduct_lc(priors, lc_priors, lc_priors)
    for i in range(n):
        assert result_key(res[i]) == result_key(res2[i]), i
        for key in ("inn_prior", "inn_lc_prior", "inn_lc_pre", "inn_lc_post", "inn_fixed_pcd", "inn_moving_pcd", "inliers_svd", "inliers_pnpransac",
                    "cos_angle", "accept"):
            assert got[i][key] == got2[i][key], (i, key)
        np.testing.assert_array_equal(got[i]["post_hessian"], got2[i]["post_hessian"])
    B.close(); B2.close()


def test_reuse_range_and_errors(hiplib, oracle):
    from cvo_slam_amd import synth
    camt = synth.camera_tuple(synth.TUM1)
    first = frame_images([0, 1, 2], synth.TUM1)
    B = hiplib.CvoBatch(6); B.set_workgroups(2)
    B.set_pairs_images(first, [0, 2, 4, 0, 2, 4], [1, 3, 5, 3, 5, 1], camt)
    before = [(B.get_cloud(p, FIXED), B.get_cloud(p, MOVING)) for p in range(6)]
    r1 = B.align(6)
    # a second call with fewer images on pairs 2..3: the others keep their clouds and align as before
    second = frame_images([5], synth.TUM1)
    want = [oracle.pcd_generate(b, d, camt) for b, d in second]
    pts = B.set_pairs_images(second, [1, 0], [0, 1], camt, first=2)
    assert list(pts) == [w["n"] for w in want]
    for p in (0, 1, 4, 5):
        for slot in (FIXED, MOVING):
            xyz, feat = B.get_cloud(p, slot)
            np.testing.assert_array_equal(xyz, before[p][slot][0]); np.testing.assert_array_equal(feat, before[p][slot][1])
    assert_cloud(B, 2, FIXED, want[1]); assert_cloud(B, 2, MOVING, want[0]); assert_cloud(B, 3, FIXED, want[0]); assert_cloud(B, 3, MOVING, want[1])
    r2 = B.align(6)
    for p in (0, 1, 4, 5):
        assert result_key(r1[p]) == result_key(r2[p]), p
    # calls that fail change nothing
    CE = hiplib.CvoError
    with pytest.raises(CE) as e:
        B.set_pairs_images(second, [0, 2], [1, 0], camt, first=0)                        # image index out of range
    assert e.value.code == hiplib.api.CVO_ERR_INVALID
    small = [(b[:32, :32], d[:32, :32]) for b, d in second]
    with pytest.raises(CE) as e:
        B.set_pairs_images(small, [0], [1], camt, first=0)                               # smaller than the selector's blocks
    assert e.value.code == hiplib.api.CVO_ERR_INVALID
    L = hiplib.load_library()
    bgr = np.ascontiguousarray(second[0][0]); dep = np.ascontiguousarray(second[0][1])
    h, w = dep.shape
    cam = hiplib.api.Camera(*camt); ip = C.POINTER(C.c_int)
    fi = np.array([0], np.int32); mi = np.array([1], np.int32)
    rc = L.cvo_batch_set_pairs_images(B.h, 0, 1, 2, (C.c_void_p * 2)(bgr.ctypes.data, None), (C.c_void_p * 2)(dep.ctypes.data, dep.ctypes.data), w, h, C.byref(cam),
                                      fi.ctypes.data_as(ip), mi.ctypes.data_as(ip), None)
    assert rc == hiplib.api.CVO_ERR_INVALID                                                # a null image
    rc = L.cvo_batch_set_pairs_images(B.h, 5, 2, 1, (C.c_void_p * 1)(bgr.ctypes.data), (C.c_void_p * 1)(dep.ctypes.data), w, h, C.byref(cam),
                                      fi.ctypes.data_as(ip), fi.ctypes.data_as(ip), None)
    assert rc == hiplib.api.CVO_ERR_INVALID                                                # pairs past max_pairs
    for p in (0, 1, 4, 5):
        xyz, _ = B.get_cloud(p, FIXED)
        np.testing.assert_array_equal(xyz, before[p][FIXED][0])
    B.reset_states()
    r3 = B.align(6)
    for p in range(6):
        assert result_key(r2[p]) == result_key(r3[p]), p
    B.close()
