"""K-stream frame-to-frame odometry on a batch (cvo_batch_advance_images, cvo_batch_align_pairs_async, cvo_batch_reset_stream,
cvo_batch_get_prev_accum_transform): every slot is one cvo::cvo odometry object that takes a frame per call, and everything it gives
must be bit-identical to a handle given the same frames (cvo_set_pcd_images, cvo_match_odometry_images, cvo_update_fixed_pcd)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXED, MOVING = 0, 1
LENGTHS = [6, 4, 1, 5, 3, 6]
CAM2 = (5000.0, 535.4, 539.2, 320.1, 247.6)      # a second camera of the same image size (TUM freiburg3-like intrinsics)


@pytest.fixture(scope="module")
def seqs():
    from cvo_slam_amd import synth
    frames = [synth.make_sequence(40 + i, n_frames=n)[0] for i, n in enumerate(LENGTHS)]
    cams = [synth.camera_tuple(synth.TUM1) if i % 2 == 0 else CAM2 for i in range(len(LENGTHS))]
    return frames, cams


def handle_steps(hiplib, frames, cam, arith="base", scores=False):
    """A handle replaying `frames` like cvo_main: per frame k >= 1 {status, transform, iter, nnz, prev, accum[, scores]}; None for frame 0."""
    g = hiplib.Cvo(); g.set_arith_mode(arith)
    out = [None]
    g.set_pcd_images(*frames[0], cam)
    for b, d in frames[1:]:
        try:
            g.match_odometry_images(b, d, cam); st = 0
        except hiplib.CvoError as e:
            st = e.code
        r = dict(status=st, transform=g.transform.copy(), iter=g.get_iteration_number(), nnz=g.get_A_nonzero(), pa=g.prev_accum_transform())
        if scores and st == 0:
            r["scores"] = g.compute_innerproduct(g.transform)
        out.append(r)
        g.update_fixed_pcd()
    g.close()
    return out


def assert_same(res, want):
    assert res["status"] == want["status"]
    if want["status"] == 0:
        np.testing.assert_array_equal(res["transform"], want["transform"])
        assert (res["iter"], res["A_nonzero"]) == (want["iter"], want["nnz"])


@pytest.mark.parametrize("slots", [3, 6])
def test_many_sequences_equal_one_handle_each(hiplib, seqs, slots):
    from cvo_slam_amd import replay
    frames, cams = seqs
    starts = [0, 0, 0, 2, 0, 0]                                     # sequence 3 starts two steps late; sequence 2 has a single frame
    got = replay.replay_odometry_many(frames, cams, slots=slots, starts=starts)
    for i, (fr, cam) in enumerate(zip(frames, cams)):
        poses, info = replay.replay_odometry(fr, cam)
        assert len(got[i][0]) == len(poses) == LENGTHS[i]
        for a, b in zip(got[i][0], poses):
            assert np.array_equal(a, b), i
        assert got[i][1] == info, i


def test_many_sequences_eigen337(hiplib, seqs):
    from cvo_slam_amd import replay
    frames, cams = seqs
    got = replay.replay_odometry_many(frames, cams, slots=4, arith="eigen337")
    for i, (fr, cam) in enumerate(zip(frames, cams)):
        poses, info = replay.replay_odometry(fr, cam, arith="eigen337")
        assert all(np.array_equal(a, b) for a, b in zip(got[i][0], poses)) and got[i][1] == info, i


def test_clouds_move_from_moving_to_fixed(hiplib, seqs):
    frames, cams = seqs
    B = hiplib.CvoBatch(2)
    use = [0, 1]                                                    # two cameras in every call
    prev_moving = [None, None]
    for k in range(4):
        pts = B.advance_images([0, 1], [frames[i][k] for i in use], [cams[i] for i in use], [0, 1])
        for p, i in enumerate(use):
            g = hiplib.Cvo(); g.set_pcd_images(*frames[i][k], cams[i])
            want_xyz, want_feat = g.get_cloud(FIXED); want_px = g.get_selected_points(FIXED); g.close()
            slot = FIXED if k == 0 else MOVING
            xyz, feat = B.get_cloud(p, slot)
            assert pts[p] == xyz.shape[0]
            np.testing.assert_array_equal(xyz, want_xyz); np.testing.assert_array_equal(feat, want_feat)
            np.testing.assert_array_equal(B.get_selected_points(p, slot), want_px)
            if k >= 2:
                fx, ff = B.get_cloud(p, FIXED)
                np.testing.assert_array_equal(fx, prev_moving[p][0]); np.testing.assert_array_equal(ff, prev_moving[p][1])
            if k >= 1:
                prev_moving[p] = (xyz, feat)
        if k >= 1:
            B.align_pairs([0, 1])
    B.close()


def test_subset_launches_and_pauses(hiplib, seqs):
    frames, cams = seqs
    use = [0, 1, 3, 5]                                              # four sequences of at least 4 frames
    want = {i: handle_steps(hiplib, frames[i][:4], cams[i]) for i in use}
    A, F = hiplib.CvoBatch(4), hiplib.CvoBatch(4)
    for B in (A, F):
        B.advance_images(range(4), [frames[i][0] for i in use], [cams[i] for i in use], range(4))
    # a listed slot with only its first frame: CVO_ERR_NOT_INITIALIZED, nothing run
    r = A.align_pairs([2, 1])
    assert [x["status"] for x in r] == [1, 1]
    for B in (A, F):
        B.advance_images(range(4), [frames[i][1] for i in use], [cams[i] for i in use], range(4))
    full = F.align_pairs([0, 1, 2, 3])
    sub = A.align_pairs([3, 0])                                     # list order
    for a, b in zip(sub, [full[3], full[0]]):
        assert a["transform"].tobytes() == b["transform"].tobytes() and (a["iter"], a["A_nonzero"], a["status"]) == (b["iter"], b["A_nonzero"], b["status"])
    for pos, p in enumerate([3, 0]):
        assert_same(sub[pos], want[use[p]][1])
    r = A.align_pairs([1, 2])                                       # slots 1 and 2 a step later, from their own states
    for pos, p in enumerate([1, 2]):
        assert_same(r[pos], want[use[p]][1])
    # slot 2 pauses for a step (neither advanced nor listed), then carries on
    A.advance_images([0, 1, 3], [frames[use[p]][2] for p in (0, 1, 3)], [cams[use[p]] for p in (0, 1, 3)], [0, 1, 2])
    r = A.align_pairs([0, 1, 3])
    for pos, p in enumerate([0, 1, 3]):
        assert_same(r[pos], want[use[p]][2])
    A.advance_images([2], [frames[use[2]][2]], [cams[use[2]]])
    r = A.align_pairs([2])
    assert_same(r[0], want[use[2]][2])
    for p in range(4):                                              # 5. prev / accum transforms of the matching handle
        if p != 2:
            pa = A.prev_accum_transform(p)
            np.testing.assert_array_equal(pa[0], want[use[p]][2]["pa"][0]); np.testing.assert_array_equal(pa[1], want[use[p]][2]["pa"][1])
    A.close(); F.close()


def test_plain_pairs_and_restarts_leave_streams_alone(hiplib, seqs):
    from cvo_slam_amd import synth
    frames, cams = seqs
    want0 = handle_steps(hiplib, frames[0], cams[0])
    want5 = handle_steps(hiplib, frames[5], cams[5])
    want4 = handle_steps(hiplib, frames[4], cams[4])
    B = hiplib.CvoBatch(3)
    pair = synth.make_small_pair(3, n=500)
    for k in range(6):
        B.advance_images([0, 1], [frames[0][k], frames[5][k]], [cams[0], cams[5]], [0, 1])
        B.set_pair(2, pair.fixed.xyz, pair.fixed.feat, pair.moving.xyz, pair.moving.feat)   # a plain pair restarted between the steps
        if k == 0:
            continue
        B.reset_states()
        r = B.align_pairs([0, 2, 1])
        assert_same(r[0], want0[k]); assert_same(r[2], want5[k])
        assert r[1]["status"] == 0
        pa = B.prev_accum_transform(1)
        np.testing.assert_array_equal(pa[1], want5[k]["pa"][1])
    B.reset_stream(0)                                               # slot 0 takes the next sequence: as a fresh handle would
    for k in range(3):
        B.advance_images([0], [frames[4][k]], [cams[4]])
        if k:
            assert_same(B.align_pairs([0])[0], want4[k])
    B.close()


def _check(got, want, rel):                                         # the tolerances of tests/test_gpu_tail_scores.py
    for key in ("inn_pre", "inn_post", "inn_fixed_pcd", "inn_moving_pcd"):
        assert got[key][1] == want[key][1], key
        assert got[key][0] == pytest.approx(want[key][0], rel=rel), key
    assert got["inliers"] == want["inliers"]
    assert got["cos_angle"] == pytest.approx(want["cos_angle"], rel=rel)
    np.testing.assert_allclose(got["post_hessian"], want["post_hessian"], rtol=1e-3, atol=1e-3 * np.abs(want["post_hessian"]).max())


def test_tail_scores_and_launch_modes(hiplib, seqs):
    frames, cams = seqs
    use = [0, 5]
    want = {i: handle_steps(hiplib, frames[i][:3], cams[i], scores=True) for i in use}
    for mode in ("tail", "adopt", "auto"):
        B = hiplib.CvoBatch(4)
        if mode == "tail":
            B.set_tail_scores(True)
        if mode == "adopt":
            B.set_adoption(True); B.set_workgroups(1)
        for k in range(3):
            B.advance_images([3, 1], [frames[i][k] for i in use], [cams[i] for i in use], [0, 1])
            if k == 0:
                continue
            r = B.align_pairs([1, 3])                               # list order: sequence 5, then sequence 0
            assert_same(r[0], want[5][k]); assert_same(r[1], want[0][k])
            if mode == "tail":
                sc = B.innerproduct_results(2)
                _check(sc[0], want[5][k]["scores"], 1e-6); _check(sc[1], want[0][k]["scores"], 1e-6)
        B.close()


def test_empty_frame_and_bad_arguments(hiplib, seqs):
    frames, cams = seqs
    fr = [(b, d.copy()) for b, d in frames[0]]
    fr[2] = (fr[2][0], np.zeros_like(fr[2][1]))                     # all-zero depth: an empty cloud
    want = handle_steps(hiplib, fr, cams[0])
    assert want[1]["status"] == 0 and want[2]["status"] != 0 and want[4]["status"] == 0
    B = hiplib.CvoBatch(2)
    bad = [
        dict(slots=[0, 0]), dict(slots=[2]), dict(slots=[-1]), dict(cam_index=[-1]),
    ]
    for k in range(len(fr)):
        before = [B.get_cloud(0, s)[0].copy() for s in (FIXED, MOVING)]
        for kw in bad:
            slots = kw.get("slots", [0])
            ims = [fr[k]] * len(slots)
            with pytest.raises((hiplib.CvoError, ValueError)) as e:
                if "cam_index" in kw:
                    import ctypes as C
                    from cvo_slam_amd import api
                    b, d, w, h = api.Cvo._images(*fr[k]); cam = api.Camera(*cams[0]); ci = (C.c_int * 1)(-1); sl = (C.c_int * 1)(0)
                    api._check(B.L.cvo_batch_advance_images(B.h, 1, sl, (C.c_void_p * 1)(b.ctypes.data), (C.c_void_p * 1)(d.ctypes.data), w, h,
                                                            C.byref(cam), ci, None))
                else:
                    import ctypes as C
                    from cvo_slam_amd import api
                    b, d, w, h = api.Cvo._images(*fr[k]); cam = api.Camera(*cams[0]); n = len(slots)
                    sl = (C.c_int * n)(*slots)
                    api._check(B.L.cvo_batch_advance_images(B.h, n, sl, (C.c_void_p * n)(*[b.ctypes.data] * n), (C.c_void_p * n)(*[d.ctypes.data] * n), w, h,
                                                            C.byref(cam), None, None))
            assert getattr(e.value, "code", 4) == 4
        import ctypes as C
        from cvo_slam_amd import api
        b, d, w, h = api.Cvo._images(*fr[k]); cam = api.Camera(*cams[0]); sl = (C.c_int * 1)(0)
        for args in ((1, sl, None, (C.c_void_p * 1)(d.ctypes.data), w, h, C.byref(cam)), (1, sl, (C.c_void_p * 1)(b.ctypes.data), (C.c_void_p * 1)(d.ctypes.data), 32, h, C.byref(cam)),
                     (1, sl, (C.c_void_p * 1)(b.ctypes.data), (C.c_void_p * 1)(d.ctypes.data), w, h, None), (0, sl, (C.c_void_p * 1)(b.ctypes.data), (C.c_void_p * 1)(d.ctypes.data), w, h, C.byref(cam))):
            assert B.L.cvo_batch_advance_images(B.h, *args, None, None) == api.CVO_ERR_INVALID
        for bad_list in ([0, 0], [5]):
            assert B.L.cvo_batch_align_pairs_async(B.h, len(bad_list), (C.c_int * len(bad_list))(*bad_list), None) == api.CVO_ERR_INVALID
        assert B.L.cvo_batch_reset_stream(B.h, 7) == api.CVO_ERR_INVALID
        after = [B.get_cloud(0, s)[0] for s in (FIXED, MOVING)]
        assert all(np.array_equal(x, y) for x, y in zip(before, after))     # no slot changed
        B.advance_images([0], [fr[k]], [cams[0]])
        if k:
            assert_same(B.align_pairs([0])[0], want[k])
    B.close()
