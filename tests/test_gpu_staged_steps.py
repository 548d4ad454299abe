"""Frames staged ahead of a K-stream step (cvo_tracks_stage_async / cvo_tracks_step_staged_async, cvo_batch_stage_images /
cvo_batch_advance_staged): the frames of step f + 1 are handed over while step f is in flight, and everything the consuming step gives must be
what the unstaged call gives for the same frames -- bits for transforms, states, iteration counts, clouds and selected pixels; the project's score
rule for score blocks (the tail may answer a score on one route and the score kernel on the other)."""
import ctypes as C

import numpy as np
import pytest

from tracks_cases import bits

pytestmark = pytest.mark.gpu

FIXED, MOVING, PREVIOUS = 0, 1, 2
ODO, KEY = 0, 1
LENGTHS = [6, 4, 1, 5, 3, 6]                                        # the fixture of tests/test_gpu_tracks.py
CAM2 = (5000.0, 535.4, 539.2, 320.1, 247.6)
A, R = True, False
# the decision on every phase-2 frame (frame 2, 3, ...) of every sequence (tests/test_gpu_tracks.py)
DECISIONS = [[A, A, R, A], [R, A], [], [A, R, R], [R], [R, R, A, R]]
INVALID, EMPTY_CLOUD, NOT_INITIALIZED = 4, 2, 1


@pytest.fixture(scope="module")
def seqs():
    from cvo_slam_amd import synth
    frames = [synth.make_sequence(40 + i, n_frames=n)[0] for i, n in enumerate(LENGTHS)]
    cams = [synth.camera_tuple(synth.TUM1) if i % 2 == 0 else CAM2 for i in range(len(LENGTHS))]
    return frames, cams


def check_scores(got, want, rel):                                    # the rule of tests/test_gpu_batch_odometry.py:159-165
    for key in ("inn_pre", "inn_post", "inn_fixed_pcd", "inn_moving_pcd"):
        assert got[key][1] == want[key][1], key
        assert got[key][0] == pytest.approx(want[key][0], rel=rel), key
    assert got["inliers"] == want["inliers"]
    assert got["cos_angle"] == pytest.approx(want["cos_angle"], rel=rel)
    np.testing.assert_allclose(got["post_hessian"], want["post_hessian"], rtol=1e-3, atol=1e-3 * np.abs(want["post_hessian"]).max())


def same_step(got, want, where):
    """the rule of tests/test_gpu_tracks.py::same_step between two cvo_track_step: bits for transforms, states, counts; the score rule for score blocks"""
    assert got["phase"] == want["phase"] and got["points"] == want["points"], where
    for obj in ("odometry", "keyframe"):
        g, w = got[obj], want[obj]
        assert g["status"] == w["status"], (where, obj, g["status"], w["status"])
        for key in ("transform", "R", "T", "ell"):
            assert np.array_equal(bits(g[key]), bits(w[key])), (where, obj, key)
        assert (g["iter"], g["A_nonzero"]) == (w["iter"], w["A_nonzero"]), (where, obj)
        if w["status"] == 0:
            check_scores(got[obj + "_scores"], want[obj + "_scores"], 1e-6)
    assert np.array_equal(bits(got["initial_guess"]), bits(want["initial_guess"])), where


def final_state(T, n):
    """every cloud, selected pixel list and state of streams 0 .. n-1, as bytes"""
    out = []
    for p in range(n):
        for obj in (ODO, KEY):
            st = T.get_state(p, obj)
            out.append(((p, obj, "state"), st["R"].tobytes() + st["T"].tobytes() + np.float32(st["ell"]).tobytes() + st["transform"].tobytes()))
            for slot in (FIXED, MOVING, PREVIOUS):
                xyz, feat = T.get_cloud(p, obj, slot)
                out.append(((p, obj, slot), xyz.tobytes() + feat.tobytes() + T.get_selected_points(p, obj, slot).tobytes()))
    return out


def staged_images(images):
    """copies of the images for a stage call, and the function that overwrites them with zeros once the call has returned"""
    own = [(np.ascontiguousarray(b).copy(), np.ascontiguousarray(d).copy()) for b, d in images]

    def wipe():
        for b, d in own:
            b[...] = 0; d[...] = 0
    return own, wipe


def run_tracks(T, frames, cams, table, staged):
    """Sequence i on stream i, every stream that still has a frame in every step.  staged: step k + 1's frames are handed over between step k's
    step call and its wait, the caller's arrays zeroed right after the stage call, and consumed by step_staged_async.  Returns steps[i][k]."""
    n = len(frames)
    steps = [[] for _ in range(n)]
    depth = max(len(f) for f in frames)
    lists = [[i for i in range(n) if len(frames[i]) > k] for k in range(depth)]
    for k in range(depth):
        ids = lists[k]
        if staged and k > 0:
            assert T.staged_count()[0] == len(ids)
            T.step_staged_async()
        else:
            T.step_async(ids, [frames[i][k] for i in ids], cams, ids)
        if staged and k + 1 < depth:
            nxt = lists[k + 1]
            own, wipe = staged_images([frames[i][k + 1] for i in nxt])
            T.stage_async(nxt, own, cams, nxt)                      # while step k is in flight
            wipe()
        res = T.wait()
        who, what = [], []
        for i, r in zip(ids, res):
            steps[i].append(r)
            if r["phase"] == 2 and r["odometry"]["status"] == 0:
                who.append(i); what.append(table[i][k - 2])
        if who:
            T.commit(who, what)
    return steps


@pytest.fixture(scope="module")
def reference(hiplib, seqs):
    """the unstaged run of all six sequences on one CvoTracks (step_async), made once: (steps, final clouds and states)"""
    frames, cams = seqs
    T = hiplib.CvoTracks(len(frames))
    steps = run_tracks(T, frames, cams, DECISIONS, staged=False)
    assert T.staged_count() == (0, 0)
    fin = final_state(T, len(frames))
    T.close()
    return steps, fin


# ---- 1. tracker streams (and 7: the caller's arrays are zeroed right after every stage call)
def test_staged_tracker_steps_equal_unstaged(hiplib, seqs, reference):
    frames, cams = seqs
    want, want_fin = reference
    T = hiplib.CvoTracks(len(frames))
    got = run_tracks(T, frames, cams, DECISIONS, staged=True)
    for i in range(len(frames)):
        assert len(got[i]) == LENGTHS[i]
        for k, (a, b) in enumerate(zip(got[i], want[i])):
            same_step(a, b, (i, k))
    assert all(s["odometry"]["status"] == 0 for st in got for s in st[1:]) and all(s["keyframe"]["status"] == 0 for st in got for s in st[2:])
    fin = final_state(T, len(frames))
    for (what, a), (_, b) in zip(fin, want_fin):
        assert a == b, what
    assert T.staged_count() == (0, sum(LENGTHS) - len(LENGTHS))     # every frame but the first step's came through the stage
    T.close()


# ---- 2. batch streams
def run_batch(B, frames, cams, staged):
    n = len(frames)
    depth = max(len(f) for f in frames)
    lists = [[i for i in range(n) if len(frames[i]) > k] for k in range(depth)]
    out = [[] for _ in range(n)]
    pts = B.advance_images(lists[0], [frames[i][0] for i in lists[0]], cams, lists[0])
    for k in range(depth):
        ids = lists[k]
        nl = B.align_pairs_async(ids) if k else 0
        if staged and k + 1 < depth:
            nxt = lists[k + 1]
            own, wipe = staged_images([frames[i][k + 1] for i in nxt])
            B.stage_images(nxt, own, cams, nxt)                     # while the launch runs
            wipe()
        res = B.wait(nl) if k else [None] * len(ids)
        for i, r, p in zip(ids, res, pts):
            out[i].append((int(p), r, None if r is None else B.prev_accum_transform(i)))
        if k + 1 < depth:
            nxt = lists[k + 1]
            if staged:
                assert B.staged_count()[0] == len(nxt)
                pts = B.advance_staged()
            else:
                pts = B.advance_images(nxt, [frames[i][k + 1] for i in nxt], cams, nxt)
    return out


def test_staged_batch_streams_equal_unstaged(hiplib, seqs):
    frames, cams = seqs                                             # two cameras in every call
    U, S = hiplib.CvoBatch(len(frames)), hiplib.CvoBatch(len(frames))
    want, got = run_batch(U, frames, cams, False), run_batch(S, frames, cams, True)
    for i in range(len(frames)):
        assert len(got[i]) == LENGTHS[i]
        for k, ((gp, g, gpa), (wp, w, wpa)) in enumerate(zip(got[i], want[i])):
            assert gp == wp and gp > 2000, (i, k)
            if k == 0:
                continue
            assert g["status"] == w["status"] == 0, (i, k)
            for key in ("transform", "R", "T"):
                assert g[key].tobytes() == w[key].tobytes(), (i, k, key)
            assert (g["iter"], g["A_nonzero"], g["iterations_run"]) == (w["iter"], w["A_nonzero"], w["iterations_run"]), (i, k)
            assert np.float32(g["ell"]).tobytes() == np.float32(w["ell"]).tobytes()
            assert gpa[0].tobytes() == wpa[0].tobytes() and gpa[1].tobytes() == wpa[1].tobytes(), (i, k)
    for p in range(len(frames)):
        for slot in (FIXED, MOVING):
            (gx, gf), (wx, wf) = S.get_cloud(p, slot), U.get_cloud(p, slot)
            assert gx.tobytes() == wx.tobytes() and gf.tobytes() == wf.tobytes(), (p, slot)
            assert S.get_selected_points(p, slot).tobytes() == U.get_selected_points(p, slot).tobytes(), (p, slot)
    assert S.staged_count() == (0, sum(LENGTHS) - len(LENGTHS)) and U.staged_count() == (0, 0)
    U.close(); S.close()


# ---- 3. a frame with no valid depth, staged
def test_staged_empty_frame_gives_the_unstaged_statuses(hiplib, seqs):
    frames, cams = seqs
    fr = [(b, d.copy()) for b, d in frames[5]]
    fr[3] = (fr[3][0], np.zeros_like(fr[3][1]))                     # all-zero depth: an empty cloud
    table = [[A, None, None, R]]                                    # frames 3 and 4 ask for no decision
    U, S = hiplib.CvoTracks(1), hiplib.CvoTracks(1)
    want = run_tracks(U, [fr], [cams[5]], table, staged=False)[0]
    key_of = lambda fin: [x for x in fin if x[0][1] == KEY]

    # the staged run step by step: the keyframe object is left as it was by the empty frame and the one after it
    got = []
    for k in range(6):
        before = key_of(final_state(S, 1))
        if k == 0:
            S.step_async([0], [fr[0]], cams[5])
        else:
            S.step_staged_async()
        if k + 1 < 6:
            S.stage_async([0], [fr[k + 1]], cams[5])
        r = S.wait()[0]
        got.append(r)
        same_step(r, want[k], k)
        if k in (3, 4):
            assert r["odometry"]["status"] == EMPTY_CLOUD and r["keyframe"]["status"] == NOT_INITIALIZED
            assert key_of(final_state(S, 1)) == before
        elif k >= 2:
            S.commit([0], [table[0][k - 2]])
    assert got[3]["points"] == 0 and [s["odometry"]["status"] for s in got[1:]] == [0, 0, EMPTY_CLOUD, EMPTY_CLOUD, 0]
    assert final_state(S, 1) == final_state(U, 1)
    U.close(); S.close()


# ---- 4. stage bookkeeping
def test_replaced_dropped_and_kept_stages(hiplib, seqs, reference):
    frames, cams = seqs
    want, _ = reference
    T = hiplib.CvoTracks(2)
    T.step_async([0], [frames[0][0]], cams[0])
    T.stage_async([0, 1], [frames[0][1], frames[1][0]], [cams[0], cams[1]], [0, 1])
    assert T.staged_count() == (2, 0)
    T.stage_async([0], [frames[0][1]], cams[0])                     # replaces the first stage, which is dropped
    assert T.staged_count() == (1, 0)
    T.wait()
    res = T.step_staged()                                           # only the second list
    assert len(res) == 1
    same_step(res[0], want[0][1], "after a replaced stage")
    assert T.get_cloud(1, ODO, FIXED)[0].shape[0] == 0 and T.staged_count() == (0, 1)
    # set_num_want drops the stage
    T.stage_async([0], [frames[0][2]], cams[0])
    T.set_num_want(3000)
    assert T.staged_count() == (0, 1)
    assert T.L.cvo_tracks_step_staged_async(T.h, None) == INVALID
    # reset of a staged stream keeps the stage: the frame arrives as the fresh stream's first
    T.stage_async([0], [frames[3][0]], cams[3])
    T.reset(0)
    assert T.staged_count() == (1, 1)
    r = T.step_staged()[0]
    same_step(r, want[3][0], "after a reset")
    assert r["phase"] == 0
    T.stage_async([0], [frames[3][1]], cams[3])
    same_step(T.step_staged()[0], want[3][1], "the reset stream's second frame")
    assert T.staged_count() == (0, 3)
    T.close()
    # the same on a batch: a replaced stage, set_num_want, a plain-pair call on a staged slot, reset_stream
    from cvo_slam_amd import synth
    B = hiplib.CvoBatch(3)
    B.stage_images([0, 1], [frames[0][0], frames[1][0]], [cams[0], cams[1]], [0, 1])
    B.stage_images([1], [frames[1][0]], cams[1])
    assert B.staged_count() == (1, 0)
    pts = B.advance_staged()
    assert len(pts) == 1 and pts[0] == want[1][0]["points"] == B.get_cloud(1, FIXED)[0].shape[0] and B.get_cloud(0, FIXED)[0].shape[0] == 0
    B.stage_images([1], [frames[1][1]], cams[1]); B.set_num_want(3000)
    assert B.staged_count() == (0, 1) and B.L.cvo_batch_advance_staged(B.h, None) == INVALID
    pair = synth.make_small_pair(3, n=500)
    B.stage_images([1, 2], [frames[1][1], frames[2][0]], [cams[1], cams[2]], [0, 1])
    B.set_pair(0, pair.fixed.xyz, pair.fixed.feat, pair.moving.xyz, pair.moving.feat)   # not a staged slot: the stage stays
    assert B.staged_count()[0] == 2
    B.set_pair(2, pair.fixed.xyz, pair.fixed.feat, pair.moving.xyz, pair.moving.feat)   # a staged slot: dropped
    assert B.staged_count() == (0, 1)
    B.stage_images([1], [frames[3][0]], cams[3]); B.reset_stream(1)
    assert B.staged_count() == (1, 1)
    assert B.advance_staged()[0] == want[3][0]["points"] == B.get_cloud(1, FIXED)[0].shape[0] and B.get_cloud(1, MOVING)[0].shape[0] == 0
    B.close()


# ---- 5. consume failures
def test_consume_failures_keep_streams_and_stage(hiplib, seqs, reference):
    frames, cams = seqs
    want, _ = reference
    T = hiplib.CvoTracks(2)
    assert T.L.cvo_tracks_step_staged_async(T.h, None) == INVALID    # nothing staged
    B = hiplib.CvoBatch(1)
    assert B.L.cvo_batch_advance_staged(B.h, None) == INVALID
    B.close()
    for k in range(3):
        T.step_async([0], [frames[0][k]], cams[0])
        if k == 2:
            T.stage_async([0], [frames[0][3]], cams[0])             # while the phase-2 step is in flight
            assert T.L.cvo_tracks_step_staged_async(T.h, None) == INVALID   # a step is in flight: refused, the stage kept
        same_step(T.wait()[0], want[0][k], k)
    before = final_state(T, 2)
    assert T.L.cvo_tracks_step_staged_async(T.h, None) == INVALID    # stream 0 awaits its decision
    assert final_state(T, 2) == before and T.staged_count() == (1, 0)
    with pytest.raises(hiplib.CvoError) as e:
        T.step_staged()
    assert e.value.code == INVALID and T.staged_count() == (1, 0)
    T.commit([0], [DECISIONS[0][0]])
    same_step(T.step_staged()[0], want[0][3], "after the commit")
    assert T.staged_count() == (0, 1)
    T.close()


# ---- 6. stage argument errors
def test_stage_argument_errors_leave_an_earlier_stage(hiplib, seqs, reference):
    from cvo_slam_amd import api
    frames, cams = seqs
    want, _ = reference
    b, d, w, h = api.Cvo._images(*frames[0][1]); cam = api.Camera(*cams[0])
    one = lambda x: (C.c_void_p * 1)(x.ctypes.data)
    two = lambda x: (C.c_void_p * 2)(x.ctypes.data, x.ctypes.data)
    bad = [(2, (C.c_int * 2)(1, 1), two(b), two(d), w, h, C.byref(cam), None),                  # listed twice
           (1, (C.c_int * 1)(1), (C.c_void_p * 1)(None), one(d), w, h, C.byref(cam), None),     # a null image
           (1, (C.c_int * 1)(1), one(b), one(d), 32, h, C.byref(cam), None),                    # a width below 64
           (1, (C.c_int * 1)(1), one(b), one(d), w, h, C.byref(cam), (C.c_int * 1)(-1))]        # a negative camera index
    T = hiplib.CvoTracks(2)
    T.step([0], [frames[0][0]], cams[0])
    T.stage_async([0], [frames[0][1]], cams[0])
    for args in bad:
        assert T.L.cvo_tracks_stage_async(T.h, *args) == INVALID, args[:2]
    assert T.staged_count() == (1, 0)
    same_step(T.step_staged()[0], want[0][1], "after refused stage calls")
    T.close()
    B = hiplib.CvoBatch(2)
    B.stage_images([0], [frames[0][0]], cams[0])
    for args in bad:
        assert B.L.cvo_batch_stage_images(B.h, *args) == INVALID, args[:2]
    assert B.staged_count() == (1, 0)
    assert B.advance_staged()[0] == want[0][0]["points"]
    B.close()


# ---- 7. the copy-out contract
def test_images_are_the_callers_again_when_the_stage_call_returns(hiplib, seqs, reference):
    """the arrays handed to a stage call are overwritten with zeros (and ones, for the colour image) as soon as it returns: the results are the
    unstaged ones, so every byte had been copied by then"""
    frames, cams = seqs
    want, _ = reference
    T = hiplib.CvoTracks(1)
    T.step([0], [frames[1][0]], cams[1])
    for k in range(1, LENGTHS[1]):
        b, d = np.ascontiguousarray(frames[1][k][0]).copy(), np.ascontiguousarray(frames[1][k][1]).copy()
        T.stage_async([0], [(b, d)], cams[1])
        b[...] = 1; d[...] = 0
        same_step(T.step_staged()[0], want[1][k], k)
        if k >= 2:
            T.commit([0], [DECISIONS[1][k - 2]])
    T.close()


# ---- 8. the replays
def test_replays_with_stage_ahead_equal_without(hiplib, seqs):
    from cvo_slam_amd import replay
    frames, cams = seqs
    decide = lambda seq, frame, odo, key: DECISIONS[seq][frame - 2]
    starts = [0, 0, 0, 2, 0, 0]
    want = replay.replay_tracker_many(frames, cams, decide, slots=3, starts=starts)
    got = replay.replay_tracker_many(frames, cams, decide, slots=3, starts=starts, stage_ahead=True)
    for i in range(len(frames)):                                    # same_run of tests/test_gpu_tracks.py
        (gp, gs, gd), (wp, ws, wd) = got[i], want[i]
        assert gd == wd and len(gs) == len(ws) == LENGTHS[i] and len(gp) == len(wp), i
        for k, (a, b) in enumerate(zip(gs, ws)):
            same_step(a, b, (i, k))
        for k, (a, b) in enumerate(zip(gp, wp)):
            assert np.array_equal(a, b), (i, k)                      # chained poses: the same bits
    want = replay.replay_odometry_many(frames, cams, slots=3, starts=starts)
    got = replay.replay_odometry_many(frames, cams, slots=3, starts=starts, stage_ahead=True)
    for i in range(len(frames)):
        assert all(np.array_equal(a, b) for a, b in zip(got[i][0], want[i][0])) and got[i][1] == want[i][1] and len(got[i][0]) == LENGTHS[i], i
