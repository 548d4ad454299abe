"""K-stream tracker steps (cvo_tracks_*): every stream is the pair of cvo::cvo objects local_tracker owns, a step runs the odometry launch, the
link kernel (reset_initial on the device) and the keyframe launch without a host round trip, and everything a stream gives must be what two handles
give for the same frames and decisions (cvo_slam_amd/replay.py: replay_tracker) -- bit for bit for transforms, iteration counts and poses."""
import numpy as np
import pytest

from helpers import rot_trans_err
import tracks_cases

pytestmark = pytest.mark.gpu

FIXED, MOVING, PREVIOUS = 0, 1, 2
ODO, KEY = 0, 1
LENGTHS = [6, 4, 1, 5, 3, 6]                                        # the fixture of tests/test_gpu_batch_odometry.py
CAM2 = (5000.0, 535.4, 539.2, 320.1, 247.6)
A, R = True, False
# the decision on every phase-2 frame (frame 2, 3, ...) of every sequence: accept runs, a rejection at the first phase-2 frame, consecutive rejections
DECISIONS = [[A, A, R, A], [R, A], [], [A, R, R], [R], [R, R, A, R]]


def decide(table):
    return lambda seq, frame, odo, key: table[seq][frame - 2]


@pytest.fixture(scope="module")
def seqs():
    from cvo_slam_amd import synth
    frames = [synth.make_sequence(40 + i, n_frames=n)[0] for i, n in enumerate(LENGTHS)]
    cams = [synth.camera_tuple(synth.TUM1) if i % 2 == 0 else CAM2 for i in range(len(LENGTHS))]
    return frames, cams


@pytest.fixture(scope="module")
def handle_runs(hiplib, seqs):
    """replay_tracker (two handles) of every sequence, per arithmetic mode, made once"""
    from cvo_slam_amd import replay
    frames, cams = seqs
    cache = {}

    def get(arith):
        if arith not in cache:
            cache[arith] = [replay.replay_tracker(fr, cam, decide(DECISIONS), arith=arith, sequence=i) for i, (fr, cam) in enumerate(zip(frames, cams))]
        return cache[arith]
    return get


def check_scores(got, want, rel):                                    # the rule of tests/test_gpu_batch_odometry.py:159-165
    for key in ("inn_pre", "inn_post", "inn_fixed_pcd", "inn_moving_pcd"):
        assert got[key][1] == want[key][1], key
        assert got[key][0] == pytest.approx(want[key][0], rel=rel), key
    assert got["inliers"] == want["inliers"]
    assert got["cos_angle"] == pytest.approx(want["cos_angle"], rel=rel)
    np.testing.assert_allclose(got["post_hessian"], want["post_hessian"], rtol=1e-3, atol=1e-3 * np.abs(want["post_hessian"]).max())


def same_step(got, want, where):
    """a stream's step against the two handles' step: bits for transforms, iter, A_nonzero and initial_guess; the score rule for score blocks"""
    assert got["phase"] == want["phase"] and got["points"] == want["points"], where
    for obj in ("odometry", "keyframe"):
        g, w = got[obj], want[obj]
        assert g["status"] == w["status"], (where, obj, g["status"], w["status"])
        if w["status"] == 0:
            for key in ("transform", "R", "T"):
                assert np.asarray(g[key], np.float32).tobytes() == np.asarray(w[key], np.float32).tobytes(), (where, obj, key)
            assert (g["iter"], g["A_nonzero"]) == (w["iter"], w["A_nonzero"]), (where, obj)
            assert np.float32(g["ell"]).tobytes() == np.float32(w["ell"]).tobytes(), (where, obj)
            check_scores(got[obj + "_scores"], want[obj + "_scores"], 1e-6)
    if want["initial_guess"] is not None:
        assert got["initial_guess"].tobytes() == np.asarray(want["initial_guess"], np.float32).tobytes(), where


def same_run(got, want, where):
    (gp, gs, gd), (wp, ws, wd) = got, want
    assert gd == wd and len(gs) == len(ws) and len(gp) == len(wp), where
    for k, (a, b) in enumerate(zip(gs, ws)):
        same_step(a, b, (where, k))
    for k, (a, b) in enumerate(zip(gp, wp)):
        assert np.array_equal(a, b), (where, k)                      # chained poses: the same bits


# ---- 1. the link kernel's arithmetic
def test_reset_initial_on_the_device_equals_host_and_oracle(hiplib, oracle):
    from cvo_slam_amd import api
    tr, od = tracks_cases.reset_initial_cases()
    n = tr.shape[0]
    assert n >= 100_000
    R, T, inv = api.selftest_reset_initial(tr, od)
    g = hiplib.Cvo()
    hR = np.zeros_like(R); hT = np.zeros_like(T); hinv = np.zeros_like(inv)
    for i in range(n):
        g.reset_transform(tr[i]); hinv[i] = g.reset_initial(od[i])
        st = g.get_state(); hR[i] = st["R"]; hT[i] = st["T"]
    g.close()
    oR, oT, oinv = tracks_cases.oracle_reset_initial(oracle, tr, od)
    for who, (wR, wT, winv) in (("host", (hR, hT, hinv)), ("oracle", (oR, oT, oinv))):
        for got, want, what in ((R, wR, "R"), (T, wT, "T"), (inv, winv, "init.inverse()")):
            bad = np.nonzero((tracks_cases.bits(got) != tracks_cases.bits(want)).reshape(n, -1).any(axis=1))[0]
            assert bad.size == 0, (who, what, bad.size, bad[:5])


# ---- 2. equality with two handles
@pytest.mark.parametrize("slots", [3, 6])
def test_streams_equal_two_handles_each(hiplib, seqs, handle_runs, slots):
    from cvo_slam_amd import replay
    frames, cams = seqs
    starts = [0, 0, 0, 2, 0, 0]                                     # sequence 3 starts two steps late; sequence 2 has a single frame
    got = replay.replay_tracker_many(frames, cams, decide(DECISIONS), slots=slots, starts=starts)
    want = handle_runs("base")
    seen = set()
    for i in range(len(frames)):
        same_run(got[i], want[i], i)
        assert len(got[i][1]) == LENGTHS[i] and got[i][2][2:] == DECISIONS[i]
        assert all(s["odometry"]["status"] == 0 for s in got[i][1][1:]) and all(s["keyframe"]["status"] == 0 for s in got[i][1][2:])
        roles = replay.keyframe_roles(DECISIONS[i]) if LENGTHS[i] >= 2 else []
        for j, d in enumerate(DECISIONS[i]):
            if not d:
                seen.add("first" if roles[j + 1][2] is None else "later")
    assert seen == {"first", "later"}                               # both branches of cvo.cpp:593-601 were run


def test_streams_equal_two_handles_eigen337(hiplib, seqs, handle_runs):
    from cvo_slam_amd import replay
    frames, cams = seqs
    got = replay.replay_tracker_many(frames, cams, decide(DECISIONS), slots=4, arith="eigen337")
    want = handle_runs("eigen337")
    for i in range(len(frames)):
        same_run(got[i], want[i], i)
    assert any(not np.array_equal(a, b) for a, b in zip(handle_runs("base")[0][0], want[0][0]))   # the mode was on


# ---- 3. clouds
def test_clouds_of_both_objects_equal_the_handles(hiplib, seqs):
    frames, cams = seqs
    use = [0, 5]
    table = {0: [A, R, R, A], 1: [R, R, A, A]}                      # a rejection, a rejection right after a rejection; stream 1 starts with the first-rejection branch
    T = hiplib.CvoTracks(2)
    H = [(hiplib.Cvo(), hiplib.Cvo()) for _ in use]

    def compare(k):
        for p in range(2):
            for obj in (ODO, KEY):
                for slot in (FIXED, MOVING, PREVIOUS):
                    want_xyz, want_feat = H[p][obj].get_cloud(slot); want_px = H[p][obj].get_selected_points(slot)
                    xyz, feat = T.get_cloud(p, obj, slot)
                    np.testing.assert_array_equal(xyz, want_xyz, err_msg=str((k, p, obj, slot)))
                    np.testing.assert_array_equal(feat, want_feat); np.testing.assert_array_equal(T.get_selected_points(p, obj, slot), want_px)

    for k in range(6):
        res = T.step([0, 1], [frames[i][k] for i in use], [cams[i] for i in use], [0, 1])
        for p, i in enumerate(use):
            odo, kf = H[p]
            if k == 0:
                odo.set_pcd_images(*frames[i][k], cams[i]); kf.set_pcd_images(*frames[i][k], cams[i])
                assert res[p]["points"] == T.get_cloud(p, ODO, FIXED)[0].shape[0] == T.get_cloud(p, KEY, FIXED)[0].shape[0] > 2000
                continue
            t = odo.match_odometry_images(*frames[i][k], cams[i]).astype(np.float32)
            assert res[p]["points"] == T.get_cloud(p, ODO, MOVING)[0].shape[0] > 2000
            if k == 1:
                kf.first_frame = False; kf.reset_transform(t)
            else:
                kf.reset_initial(t); kf.match_keyframe_images(*frames[i][k], cams[i])
                np.testing.assert_array_equal(T.get_cloud(p, KEY, MOVING)[0], T.get_cloud(p, ODO, MOVING)[0])   # one generated cloud, held by both objects
        if k >= 2:
            compare((k, "before the decision"))
        for p, i in enumerate(use):
            odo, kf = H[p]
            if k >= 1:
                odo.update_fixed_pcd()
            if k >= 2:
                if table[p][k - 2]:
                    kf.update_previous_pcd()
                else:
                    kf.reset_keyframe(H[p][0].transform)
        if k >= 2:
            T.commit([0, 1], [table[0][k - 2], table[1][k - 2]])
            for p in range(2):                                      # what update_fixed_pcd will make the fixed cloud at the next step
                np.testing.assert_array_equal(T.get_cloud(p, ODO, MOVING)[0], H[p][0].get_cloud(FIXED)[0])
        # the odometry handle has moved on (update_fixed_pcd); the stream's odometry object does so at its next step: compare the keyframe objects, and the
        # odometry object's clouds one step later (its fixed cloud then is the handle's)
        for p in range(2):
            for slot in (FIXED, MOVING, PREVIOUS):
                want_xyz, want_feat = H[p][1].get_cloud(slot)
                xyz, feat = T.get_cloud(p, KEY, slot)
                np.testing.assert_array_equal(xyz, want_xyz, err_msg=str((k, p, slot))); np.testing.assert_array_equal(feat, want_feat)
                np.testing.assert_array_equal(T.get_selected_points(p, KEY, slot), H[p][1].get_selected_points(slot))
            ks, hs = T.get_state(p, KEY), H[p][1].get_state()
            assert ks["R"].tobytes() == hs["R"].tobytes() and ks["T"].tobytes() == hs["T"].tobytes() and ks["transform"].tobytes() == H[p][1].transform.tobytes()
    T.close()
    for odo, kf in H:
        odo.close(); kf.close()


# ---- 4. against the oracle
def test_full_size_tracker_streams_vs_oracle(hiplib, oracle):
    """The sequence of tests/test_gpu_replay.py::test_full_size_tracker_sequence_from_images_vs_oracle (640x480, 5 frames) with one rejection at
    frame 3, on three streams at once, against oracle objects fed with the oracle generator's clouds: every transform within 1e-4 rad / 1e-4 m
    (north_star), every iteration count equal, score counts exact and values to rel 1e-5."""
    from cvo_slam_amd import synth
    frames, _ = synth.make_sequence(2, n_frames=5)
    cam = synth.camera_tuple(synth.TUM1)
    decisions = {2: True, 3: False, 4: True}
    T = hiplib.CvoTracks(3)
    got = [[] for _ in range(3)]
    for k, f in enumerate(frames):
        res = T.step([2, 0, 1], [f, f, f], cam)
        for p, r in zip([2, 0, 1], res):
            got[p].append(r)
        if k >= 2:
            T.commit([0, 1, 2], [decisions[k]] * 3)
    T.close()

    clouds = [oracle.pcd_generate(b, d, cam) for (b, d) in frames]
    oo, ok = oracle.OracleCvo(search=oracle.SEARCH_KDTREE, threads=8), oracle.OracleCvo(search=oracle.SEARCH_KDTREE, threads=8)
    want = [None]
    c = clouds[0]; oo.set_pcd(c["xyz"], c["feat"]); ok.set_pcd(c["xyz"], c["feat"])
    for k in range(1, 5):
        c = clouds[k]
        rc, t = oo.match(c["xyz"], c["feat"]); assert rc == 0
        w = dict(odometry=(t, oo.get_state()["iter"]))
        rc, w["odometry_scores"] = oo.compute_innerproduct(oo.get_state()["transform"]); assert rc == 0
        oo.update_fixed_pcd()
        if k == 1:
            ok.reset_transform(t.astype(np.float32))
        else:
            w["initial_guess"] = ok.reset_initial(t.astype(np.float32))
            rc, tk = ok.match(c["xyz"], c["feat"]); assert rc == 0
            w["keyframe"] = (tk, ok.get_state()["iter"])
            rc, w["keyframe_scores"] = ok.compute_innerproduct(ok.get_state()["transform"]); assert rc == 0
            if decisions[k]:
                ok.update_previous_pcd()
            else:
                ok.reset_keyframe(t.astype(np.float32))
        want.append(w)
    for p in range(3):
        assert [r["phase"] for r in got[p]] == [0, 1, 2, 2, 2]
        assert [r["points"] for r in got[p]] == [c["n"] for c in clouds]
        for k in range(1, 5):
            for obj in ("odometry", "keyframe") if k >= 2 else ("odometry",):
                g, (tw, iw) = got[p][k][obj], want[k][obj]
                assert g["status"] == 0
                re, te = rot_trans_err(g["transform"], tw)
                assert re <= 1e-4 and te <= 1e-4, (p, k, obj, re, te)
                assert g["iter"] == iw, (p, k, obj, g["iter"], iw)
                gs, ws = got[p][k][obj + "_scores"], want[k][obj + "_scores"]
                for key in ("inn_pre", "inn_post", "inn_fixed_pcd", "inn_moving_pcd"):
                    assert gs[key][1] == ws[key][1], (p, k, obj, key)
                    assert gs[key][0] == pytest.approx(ws[key][0], rel=1e-5), (p, k, obj, key)
                assert gs["inliers"] == ws["inliers"], (p, k, obj)
            if k >= 2:
                re, te = rot_trans_err(got[p][k]["initial_guess"], want[k]["initial_guess"])
                assert re <= 1e-4 and te <= 1e-4, (p, k, "initial_guess")
        for k in range(5):                                          # three streams given the same frames: the same bits
            assert got[p][k]["odometry"]["transform"].tobytes() == got[0][k]["odometry"]["transform"].tobytes()
            assert got[p][k]["keyframe"]["transform"].tobytes() == got[0][k]["keyframe"]["transform"].tobytes()


# ---- 5. protocol
def snapshot(T, p):
    return [T.get_state(p, obj)[key].tobytes() for obj in (ODO, KEY) for key in ("R", "T", "transform")] + \
           [T.get_cloud(p, obj, slot)[0].tobytes() for obj in (ODO, KEY) for slot in (FIXED, MOVING, PREVIOUS)]


def test_commit_protocol_and_argument_errors(hiplib, seqs, handle_runs):
    import ctypes as C
    from cvo_slam_amd import api
    frames, cams = seqs
    want = handle_runs("base")[0][1]
    T = hiplib.CvoTracks(3)
    with pytest.raises(hiplib.CvoError) as e:                       # nothing stepped yet
        T.commit([0], [True])
    assert e.value.code == 4
    for k in range(2):
        same_step(T.step([0], [frames[0][k]], cams[0])[0], want[k], k)
        with pytest.raises(hiplib.CvoError) as e:                   # phase 0 / 1: no decision is expected
            T.commit([0], [True])
        assert e.value.code == 4
    same_step(T.step([0], [frames[0][2]], cams[0])[0], want[2], 2)
    before = snapshot(T, 0)
    for streams in ([0], [1, 0]):                                   # a step before the pending decision, alone and beside a stream that could step
        with pytest.raises(hiplib.CvoError) as e:
            T.step(streams, [frames[0][3]] * len(streams), cams[0])
        assert e.value.code == 4
    with pytest.raises(hiplib.CvoError) as e:                       # a decision for a stream that expects none, beside one that does
        T.commit([0, 1], [True, True])
    assert e.value.code == 4
    b, d, w, h = api.Cvo._images(*frames[0][3]); cam = api.Camera(*cams[0])
    one = lambda x: (C.c_void_p * 1)(x.ctypes.data)
    two = lambda x: (C.c_void_p * 2)(x.ctypes.data, x.ctypes.data)
    bad = [(2, (C.c_int * 2)(1, 1), two(b), two(d), w, h, C.byref(cam), None, None),            # a stream listed twice
           (1, (C.c_int * 1)(3), one(b), one(d), w, h, C.byref(cam), None, None), (1, (C.c_int * 1)(-1), one(b), one(d), w, h, C.byref(cam), None, None),
           (1, (C.c_int * 1)(1), None, one(d), w, h, C.byref(cam), None, None), (1, (C.c_int * 1)(1), one(b), one(d), 32, h, C.byref(cam), None, None),
           (1, (C.c_int * 1)(1), one(b), one(d), w, h, None, None, None), (0, (C.c_int * 1)(1), one(b), one(d), w, h, C.byref(cam), None, None),
           (1, (C.c_int * 1)(1), one(b), one(d), w, h, C.byref(cam), (C.c_int * 1)(-1), None), (4, (C.c_int * 4)(0, 1, 2, 0), None, None, w, h, C.byref(cam), None, None)]
    for args in bad:
        assert T.L.cvo_tracks_step_async(T.h, *args) == api.CVO_ERR_INVALID, args[:2]
    assert T.L.cvo_tracks_commit(T.h, 2, (C.c_int * 2)(0, 0), (C.c_int * 2)(1, 1)) == api.CVO_ERR_INVALID
    assert T.L.cvo_tracks_reset(T.h, 3) == api.CVO_ERR_INVALID
    assert T.L.cvo_tracks_wait(T.h, None, 0) == api.CVO_ERR_INVALID   # no step in flight
    assert snapshot(T, 0) == before                                  # nothing changed
    assert T.get_cloud(1, ODO, FIXED)[0].shape[0] == 0               # stream 1 never started
    T.commit([0], [DECISIONS[0][0]])
    for k in range(3, 6):                                            # the same steps succeed after the commit and give the handles' results
        same_step(T.step([0], [frames[0][k]], cams[0])[0], want[k], k)
        T.commit([0], [DECISIONS[0][k - 2]])
    T.close()


def test_empty_frame_leaves_the_keyframe_object_alone(hiplib, seqs):
    from cvo_slam_amd import replay
    frames, cams = seqs
    fr = [(b, d.copy()) for b, d in frames[5]]
    fr[3] = (fr[3][0], np.zeros_like(fr[3][1]))                     # all-zero depth: an empty cloud
    table = [[A, None, None, R]]                                    # frames 3 and 4 ask for no decision
    asked = []

    def accept(seq, frame, odo, key):
        asked.append(frame); return table[0][frame - 2]
    want = replay.replay_tracker(fr, cams[5], accept)
    assert asked == [2, 5]
    assert [s["odometry"]["status"] for s in want[1][1:]] == [0, 0, 2, 2, 0]                     # the frame after the empty one fails too, against an empty fixed cloud
    T = hiplib.CvoTracks(1)
    for k in range(6):
        key_before = snapshot(T, 0)[3:6] + snapshot(T, 0)[9:]
        r = T.step([0], [fr[k]], cams[5])[0]
        same_step(r, want[1][k], k)
        if k in (3, 4):
            assert r["odometry"]["status"] == 2 and r["keyframe"]["status"] == 1 and r["points"] == (0 if k == 3 else r["points"])
            assert snapshot(T, 0)[3:6] + snapshot(T, 0)[9:] == key_before                        # the keyframe object's state and clouds: unchanged
            with pytest.raises(hiplib.CvoError):
                T.commit([0], [True])
        elif k >= 2:
            T.commit([0], [table[0][k - 2]])
    T.close()
    got = replay.replay_tracker_many([fr], [cams[5]], lambda s, f, o, q: table[0][f - 2])
    same_run(got[0], want, "empty frame")


def test_reset_and_subsets(hiplib, seqs, handle_runs):
    frames, cams = seqs
    want = handle_runs("base")
    T = hiplib.CvoTracks(2)

    def advance(p, i, k):
        r = T.step([p], [frames[i][k]], cams[i])[0]
        same_step(r, want[i][1][k], (i, k))
        if k >= 2:
            T.commit([p], [DECISIONS[i][k - 2]])
    # streams stepped one at a time, in changing order, each at its own pace
    for p, i, k in [(1, 3, 0), (0, 1, 0), (0, 1, 1), (1, 3, 1), (1, 3, 2), (1, 3, 3), (0, 1, 2), (1, 3, 4), (0, 1, 3)]:
        advance(p, i, k)
    # both in one step, listed in reverse: results in list order
    T.reset(0); T.reset(1)
    for k in range(3):
        res = T.step([1, 0], [frames[4][k], frames[0][k]], [cams[4], cams[0]], [0, 1])
        same_step(res[0], want[4][1][k], (4, k)); same_step(res[1], want[0][1][k], (0, k))
        if k == 2:
            T.commit([0, 1], [DECISIONS[0][0], DECISIONS[4][0]])
    # a reset stream replays like a fresh one
    T.reset(1)
    for k in range(5):
        advance(1, 3, k)
    T.close()
