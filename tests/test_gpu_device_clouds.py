"""Point clouds in caller-owned device memory (cvo_device_cloud; cvo_batch_set_pairs_device_clouds, cvo_batch_advance_device_clouds,
cvo_tracks_step_device_clouds_async): the ingest kernel alone against the numpy gather of the same tensors, then every entry point against
the same floats handed over from the host or generated from the images -- bits for transforms, states, counts and clouds; the project's
score rule for score blocks -- with the caller's tensors overwritten as early as the ordering rules of include/cvo_hip.h allow, and the
refusals of the validation."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXED, MOVING, PREVIOUS = 0, 1, 2
ODO, KEY = 0, 1
CAM2 = (5000.0, 535.4, 539.2, 320.1, 247.6)
A, R = True, False
INVALID, EMPTY = 4, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the layouts a cloud arrives in.  Each returns (xyz view (n, 3), feat view, feat_layout, the tensors that own the memory).
def lay_tight(torch, x, f, rng):
    tx, tf = up(torch, x), up(torch, f)
    return tx, tf, "channels_first", [tx, tf]


def lay_tight_off4(torch, x, f, rng):
    """tight arrays whose bases lie 4 bytes past a 16-byte boundary (torch allocations are at least 256-byte aligned)"""
    n = x.shape[0]
    bx = rng.normal(size=3 * n + 1).astype(np.float32); bx[1:] = x.reshape(-1)
    bf = rng.normal(size=5 * n + 1).astype(np.float32); bf[1:] = f.reshape(-1)
    tx, tf = up(torch, bx), up(torch, bf)
    assert tx.data_ptr() % 16 == 0 and tf.data_ptr() % 16 == 0
    return tx[1:].view(n, 3), tf[1:].view(5, n), "channels_first", [tx, tf]


def lay_stride(stride_floats, col0):
    def lay(torch, x, f, rng):
        """positions as columns col0 .. col0+2 of an (n, stride) tensor; features points first (20 / 4)"""
        n = x.shape[0]
        big = rng.normal(size=(n, stride_floats)).astype(np.float32); big[:, col0:col0 + 3] = x
        tb, tf = up(torch, big), up(torch, np.ascontiguousarray(f.T))
        return tb[:, col0:col0 + 3], tf, "points_first", [tb, tf]
    return lay


def lay_padded_channels(torch, x, f, rng):
    """channel-major features with a channel stride of 4 (n + 3)"""
    n = x.shape[0]
    big = rng.normal(size=(5, n + 3)).astype(np.float32); big[:, :n] = f
    tx, tb = up(torch, x), up(torch, big)
    return tx, tb[:, :n], "channels_first", [tx, tb]


def lay_point_stride8(torch, x, f, rng):
    """every second float of five channel arrays of 2 n: point stride 8"""
    n = x.shape[0]
    big = rng.normal(size=(5, 2 * n)).astype(np.float32); big[:, ::2] = f
    tx, tb = up(torch, x), up(torch, big)
    return tx, tb[:, ::2], "channels_first", [tx, tb]


LAYOUTS = [lay_tight, lay_tight_off4, lay_stride(4, 0), lay_stride(8, 2), lay_padded_channels, lay_point_stride8]


def random_cloud(rng, n):
    x = rng.normal(size=(n, 3)).astype(np.float32)
    x[:, 2] = rng.uniform(0.4, 6.0, n).astype(np.float32)
    if n:                                                           # sampled points (every 16th) behind, at and barely in front of the camera
        x[0::32, 2] = -x[0::32, 2]
        x[16::64, 2] = np.float32(1e-3)
        x[48::64, 2] = np.float32(0.0)
        x[80::128, 2] = np.nextafter(np.float32(1e-3), np.float32(1))
    return x, rng.uniform(0, 1, (5, n)).astype(np.float32)


def cost_terms(x):
    z = x[0::16, 2]
    z = z[z > np.float32(1e-3)].astype(np.float64)
    return 1.0 / (z * z)


# ---- 1. the ingest kernel alone
def test_ingest_kernel_is_the_gather(hiplib, torch):
    rng = np.random.default_rng(20)
    sizes = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 771, 3072]
    clouds, want, keep = [], [], []
    for k, n in enumerate(sizes + [3072, 771, 257, 65, 17]):        # every layout meets a size with a head, a body and a tail
        x, f = random_cloud(rng, n)
        want.append((x, f))
        if n == 0:
            clouds.append(hiplib.api.DeviceCloud(None, None, 0, 0, 0, 0, 0)); continue
        tx, tf, layout, own = LAYOUTS[k % len(LAYOUTS)](torch, x, f, rng)
        keep += own
        d = hiplib.api.device_cloud(tx, tf, layout)
        if k % len(LAYOUTS) == 0 and k % 2 == 0:                    # the tight layout by its zeros
            d = hiplib.api.DeviceCloud(d.xyz, d.feat, 0, 0, 0, d.n, 0)
        clouds.append(d)
    assert any(cost_terms(x).size < (x.shape[0] + 15) // 16 for x, _ in want)
    torch.cuda.synchronize()
    got, cost, guards = hiplib.api.selftest_ingest_clouds(clouds)
    assert guards, "guard bytes written"
    for k, ((gx, gf), (wx, wf)) in enumerate(zip(got, want)):
        assert gx.tobytes() == wx.tobytes() and gf.tobytes() == wf.tobytes(), (k, wx.shape[0])
        terms = cost_terms(wx)
        assert cost[k, 1] == terms.size, (k, cost[k], terms.size)   # the sample count: exact
        # at most 4096 positive terms: every order of summation errs by at most (m - 1) 2^-53 < 4.5e-13 relative; the terms themselves are
        # the same doubles (z * z is exact in double, the division is correctly rounded on both sides)
        print(f"cloud {k}: n {wx.shape[0]} samples {terms.size} sum {cost[k, 0]!r} numpy {float(terms.sum())!r}")
        np.testing.assert_allclose(cost[k, 0], terms.sum(), rtol=1e-12, atol=0)
    got2, cost2, guards2 = hiplib.api.selftest_ingest_clouds(clouds)
    assert guards2 and cost2.tobytes() == cost.tobytes()
    assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(got, got2))


# ---- 2. plain pairs (+ 5. ordering on the side-stream leg)
@pytest.fixture(scope="module")
def pair_clouds():
    g = [np.load(os.path.join(GOLDEN, f"small_pair_{i}.npz")) for i in (11, 12, 13)]
    cat = lambda a, b, key: np.concatenate([a[key], b[key]], axis=0 if key.endswith("xyz") else 1)
    clouds = [(g[0]["fixed_xyz"], g[0]["fixed_feat"]),                                                  # 0: 300, the fixed cloud of pairs 0 and 1
              (g[0]["moving_xyz"], g[0]["moving_feat"]),                                                # 1: 300
              (np.concatenate([g[0]["moving_xyz"], g[0]["moving_xyz"][:150] + np.float32(0.01)]),
               np.concatenate([g[0]["moving_feat"], g[0]["moving_feat"][:, :150]], axis=1)),            # 2: 450
              (cat(g[1], g[2], "fixed_xyz"), cat(g[1], g[2], "fixed_feat")),                            # 3: 600
              (cat(g[1], g[2], "moving_xyz"), cat(g[1], g[2], "moving_feat")),                          # 4: 600
              (g[2]["fixed_xyz"], g[2]["fixed_feat"]),                                                  # 5: 300
              (np.zeros((0, 3), np.float32), np.zeros((5, 0), np.float32))]                             # 6: empty
    clouds = [(np.ascontiguousarray(x, np.float32), np.ascontiguousarray(f, np.float32)) for x, f in clouds]
    return clouds, [0, 0, 3, 5], [1, 2, 4, 6]


@pytest.fixture(scope="module")
def pair_reference(hiplib, pair_clouds):
    clouds, fi, mi = pair_clouds
    B = hiplib.CvoBatch(4)
    B.set_pairs([clouds[a] + clouds[b] for a, b in zip(fi, mi)])
    res = B.align(4)
    got = [(B.get_cloud(p, FIXED), B.get_cloud(p, MOVING)) for p in range(4)]
    B.close()
    assert [r["status"] for r in res] == [0, 0, 0, EMPTY]
    return res, got


def same_pair_result(g, w, where):
    assert g["status"] == w["status"], (where, g["status"], w["status"])
    if w["status"] == 0:
        for key in ("transform", "R", "T"):
            assert np.asarray(g[key], np.float32).tobytes() == np.asarray(w[key], np.float32).tobytes(), (where, key)
        assert np.float32(g["ell"]).tobytes() == np.float32(w["ell"]).tobytes(), where
        assert (g["iter"], g["A_nonzero"]) == (w["iter"], w["A_nonzero"]), where


@pytest.mark.parametrize("side_stream", [False, True])
def test_set_pairs_clouds_equal_set_pairs(hiplib, torch, pair_clouds, pair_reference, side_stream):
    clouds, fi, mi = pair_clouds
    want, want_clouds = pair_reference
    rng = np.random.default_rng(3)
    side = torch.cuda.Stream() if side_stream else None
    B = hiplib.CvoBatch(4)
    for rep in range(2):                                            # the second hand-over reuses the objects the first one let go of
        with torch.cuda.stream(side if side is not None else torch.cuda.current_stream()):
            ups = [LAYOUTS[(k + rep) % len(LAYOUTS)](torch, x, f, rng) if x.shape[0] else (up(torch, x), up(torch, f), None, []) for k, (x, f) in enumerate(clouds)]
        B.set_pairs_clouds([(u[0], u[1], u[2]) for u in ups], fi, mi, cloud_stream=side)
        with torch.cuda.stream(side if side is not None else torch.cuda.current_stream()):
            for u in ups:                                           # the caller's memory is the caller's again: overwritten at once
                for t in u[3]:
                    t.fill_(float("nan"))
        res = B.align(4)
        for p in range(4):
            same_pair_result(res[p], want[p], (rep, p))
            for slot in (FIXED, MOVING):
                gx, gf = B.get_cloud(p, slot)
                assert gx.tobytes() == want_clouds[p][slot][0].tobytes() and gf.tobytes() == want_clouds[p][slot][1].tobytes(), (rep, p, slot)
                assert B.get_selected_points(p, slot).shape[0] == 0
        assert B.get_cloud(0, FIXED)[0].tobytes() == B.get_cloud(1, FIXED)[0].tobytes() == clouds[0][0].tobytes()
    # a pair of the shared cloud handed over from the host again: its neighbour keeps the shared cloud
    B.set_pair(0, *clouds[5], *clouds[1])
    assert B.get_cloud(1, FIXED)[0].tobytes() == clouds[0][0].tobytes() and B.get_cloud(0, FIXED)[0].tobytes() == clouds[5][0].tobytes()
    same_pair_result(B.align(2)[1], want[1], "after set_pair on the neighbour")
    torch.cuda.synchronize()
    B.close()


# ---- 3. stream slots
LENGTHS = [6, 6, 5]


@pytest.fixture(scope="module")
def seqs():
    from cvo_slam_amd import synth
    frames = [synth.make_sequence(40 + i, n_frames=n)[0] for i, n in enumerate(LENGTHS)]
    cams = [synth.camera_tuple(synth.TUM1) if i % 2 == 0 else CAM2 for i in range(len(LENGTHS))]
    return frames, cams


@pytest.fixture(scope="module")
def frame_clouds(hiplib, seqs):
    """the cloud of every frame, taken once from the image path through get_cloud"""
    frames, cams = seqs
    B = hiplib.CvoBatch(3)
    out = [[] for _ in frames]
    for k in range(max(LENGTHS)):
        ids = [i for i in range(3) if k < LENGTHS[i]]
        B.advance_images(ids, [frames[i][k] for i in ids], [cams[i] for i in ids], range(len(ids)))
        for i in ids:
            out[i].append(B.get_cloud(i, FIXED))
            B.reset_stream(i)                                       # (every frame is a fresh slot's first frame)
    B.close()
    assert all(2000 < c[0].shape[0] < 4000 for s in out for c in s)
    return out


def handle_steps(hiplib, clouds):
    """a handle fed host clouds like cvo_main: per cloud k >= 1 the result fields, plus prev / accum transforms"""
    g = hiplib.Cvo()
    g.set_pcd(*clouds[0])
    out = [None]
    for x, f in clouds[1:]:
        g.match_odometry(x, f)
        st = g.get_state()
        out.append(dict(status=0, transform=g.transform.copy(), R=np.asarray(st["R"], np.float32).reshape(3, 3), T=np.asarray(st["T"], np.float32),
                        ell=st["ell"], iter=g.get_iteration_number(), A_nonzero=g.get_A_nonzero(), pa=g.prev_accum_transform()))
        g.update_fixed_pcd()
    g.close()
    return out


def test_advance_clouds_equal_a_handle_per_sequence(hiplib, torch, frame_clouds):
    rng = np.random.default_rng(4)
    use = 4                                                         # four clouds per sequence
    want = [handle_steps(hiplib, frame_clouds[i][:use]) for i in range(3)]
    B = hiplib.CvoBatch(4)
    slot_of = [2, 0, 3]                                             # sequence i runs in slot slot_of[i]

    def hand(seq_ids, k):
        ups = [LAYOUTS[(i + k) % len(LAYOUTS)](torch, *frame_clouds[i][k], rng) for i in seq_ids]
        B.advance_clouds([slot_of[i] for i in seq_ids], [(u[0], u[1], u[2]) for u in ups])
        for u in ups:
            for t in u[3]:
                t.zero_()

    def check(seq_ids, k, res):
        for r, i in zip(res, seq_ids):
            same_pair_result(r, want[i][k], (i, k))
            pa = B.prev_accum_transform(slot_of[i])
            assert pa[0].tobytes() == want[i][k]["pa"][0].tobytes() and pa[1].tobytes() == want[i][k]["pa"][1].tobytes(), (i, k)
            for slot, kk in ((FIXED, k - 1), (MOVING, k)):
                gx, gf = B.get_cloud(slot_of[i], slot)
                assert gx.tobytes() == frame_clouds[i][kk][0].tobytes() and gf.tobytes() == frame_clouds[i][kk][1].tobytes(), (i, k, slot)
            assert B.get_selected_points(slot_of[i], MOVING).shape[0] == 0

    hand([0, 1, 2], 0)
    assert [r["status"] for r in B.align_pairs([slot_of[0], slot_of[1]])] == [1, 1]   # only the first cloud is in: CVO_ERR_NOT_INITIALIZED
    hand([0, 1, 2], 1)
    check([0, 1, 2], 1, B.align_pairs([slot_of[i] for i in (0, 1, 2)]))
    hand([2, 0], 2)                                                 # a subset step, in another order; sequence 1 pauses
    check([0, 2], 2, B.align_pairs([slot_of[0], slot_of[2]]))
    hand([1], 2)
    check([1], 2, B.align_pairs([slot_of[1]]))
    hand([0, 1, 2], 3)
    check([2, 1, 0], 3, B.align_pairs([slot_of[i] for i in (2, 1, 0)]))
    # the slot of sequence 1 starts over with sequence 0's clouds; the others are not disturbed
    B.reset_stream(slot_of[1])
    assert B.get_cloud(slot_of[1], FIXED)[0].shape[0] == 0
    for k in range(3):
        ups = LAYOUTS[k](torch, *frame_clouds[0][k], rng)
        B.advance_clouds([slot_of[1]], [(ups[0], ups[1], ups[2])])
        if k >= 1:
            same_pair_result(B.align_pairs([slot_of[1]])[0], want[0][k], ("after reset", k))
    pa = B.prev_accum_transform(slot_of[0])
    assert pa[1].tobytes() == want[0][3]["pa"][1].tobytes()
    torch.cuda.synchronize()
    B.close()


# ---- 4. tracker streams (+ 5. ordering on the side-stream leg)
DECISIONS = [{2: R, 5: A}, {2: A, 3: R, 4: R, 5: A}, {2: R, 3: R, 4: A}]   # a first-frame rejection, consecutive rejections, accepts; sequence 0 has an empty frame 3


def check_scores(got, want, rel):                                    # the rule of tests/test_gpu_tracks.py (tests/test_gpu_batch_odometry.py:159-165)
    for key in ("inn_pre", "inn_post", "inn_fixed_pcd", "inn_moving_pcd"):
        assert got[key][1] == want[key][1], key
        assert got[key][0] == pytest.approx(want[key][0], rel=rel), key
    assert got["inliers"] == want["inliers"]
    assert got["cos_angle"] == pytest.approx(want["cos_angle"], rel=rel)
    np.testing.assert_allclose(got["post_hessian"], want["post_hessian"], rtol=1e-3, atol=1e-3 * np.abs(want["post_hessian"]).max())


def same_step(got, want, where):
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
    assert got["initial_guess"].tobytes() == want["initial_guess"].tobytes(), where


def key_object(T, s):
    st = T.get_state(s, KEY)
    return [np.asarray(st[k], np.float32).tobytes() for k in ("R", "T", "transform")] + [np.float32(st["ell"]).tobytes()] + \
           [a.tobytes() for slot in (FIXED, MOVING, PREVIOUS) for a in T.get_cloud(s, KEY, slot)]


@pytest.fixture(scope="module")
def tracker_frames(seqs):
    frames, cams = seqs
    fr = [list(f) for f in frames]
    fr[0][3] = (fr[0][3][0], np.zeros_like(fr[0][3][1]))           # all-zero depth: an empty cloud
    return fr, cams


@pytest.mark.parametrize("side_stream", [False, True])
def test_tracker_steps_on_clouds_equal_steps_on_images(hiplib, torch, tracker_frames, side_stream):
    frames, cams = tracker_frames
    rng = np.random.default_rng(5)
    side = torch.cuda.Stream() if side_stream else None
    ctx = lambda: torch.cuda.stream(side if side is not None else torch.cuda.current_stream())
    TI, TC = hiplib.CvoTracks(3), hiplib.CvoTracks(3)
    seen_empty = False
    for k in range(max(LENGTHS)):
        ids = [i for i in range(3) if k < LENGTHS[i]]
        want = TI.step(ids, [frames[i][k] for i in ids], [cams[i] for i in ids], range(len(ids)))
        host = [TI.get_cloud(i, ODO, FIXED if k == 0 else MOVING) for i in ids]   # the frames' clouds, from the image path
        with ctx():
            ups = [LAYOUTS[(i + k) % len(LAYOUTS)](torch, x, f, rng) if x.shape[0] else (up(torch, x), up(torch, f), None, []) for i, (x, f) in zip(ids, host)]
        before = [key_object(TC, i) for i in ids]
        got = TC.step_clouds(ids, [(u[0], u[1], u[2]) for u in ups], cloud_stream=side)
        with ctx():
            for u in ups:
                for t in u[3]:
                    t.fill_(float("nan"))
        decide_ids, decide = [], []
        for pos, i in enumerate(ids):
            same_step(got[pos], want[pos], (i, k))
            assert got[pos]["points"] == host[pos][0].shape[0]
            if want[pos]["phase"] >= 1 and want[pos]["odometry"]["status"] != 0:                  # the empty frame and the frame after it
                seen_empty = True
                assert got[pos]["odometry"]["status"] == EMPTY and got[pos]["keyframe"]["status"] == 1
                assert key_object(TC, i) == before[pos]                                          # the keyframe object: left alone
                with pytest.raises(hiplib.CvoError):
                    TC.commit([i], [True])
            elif want[pos]["phase"] == 2:
                decide_ids.append(i); decide.append(DECISIONS[i][k])
        for T in (TI, TC):
            if decide_ids:
                T.commit(decide_ids, decide)
        for i in ids:                                               # the clouds of both objects in all three slots, after the decision
            for obj in (ODO, KEY):
                for slot in (FIXED, MOVING, PREVIOUS):
                    (wx, wf), (gx, gf) = TI.get_cloud(i, obj, slot), TC.get_cloud(i, obj, slot)
                    assert gx.tobytes() == wx.tobytes() and gf.tobytes() == wf.tobytes(), (i, k, obj, slot)
                    assert TC.get_selected_points(i, obj, slot).shape[0] == 0
            assert key_object(TC, i)[:4] == key_object(TI, i)[:4], (i, k)
    assert seen_empty
    torch.cuda.synchronize()
    TI.close(); TC.close()


# ---- 6. refusals: through cvo_check_device_clouds, nothing is launched
def loaded_hip():
    """the HIP runtime this process already has (torch's copy: tests/conftest.py)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise AssertionError("no HIP runtime loaded")


def refused(hiplib, desc, word, index=0, before=()):
    D = hiplib.api.DeviceCloud
    arr = (D * (len(before) + 1))(*before, desc)
    L = hiplib.api.load_library()
    rc = L.cvo_check_device_clouds(0, len(before) + 1, arr)
    msg = L.cvo_last_error().decode()
    assert rc == INVALID, (rc, msg, word)
    assert word in msg and f"cloud {index + len(before)}" in msg, msg


def test_refusals_name_cloud_and_field(hiplib, torch):
    n = 1024
    D = hiplib.api.DeviceCloud
    L = hiplib.api.load_library()
    tx = torch.zeros((n, 3), dtype=torch.float32, device="cuda"); tf = torch.zeros((5, n), dtype=torch.float32, device="cuda")
    px, pf = tx.data_ptr(), tf.data_ptr()
    good = D(px, pf, 0, 0, 0, n, 0)
    assert L.cvo_check_device_clouds(0, 2, (D * 2)(good, D(None, None, 0, 0, 0, 0, 0))) == 0       # n == 0 needs no pointers
    assert L.cvo_check_device_clouds(0, 1, (D * 1)(D(px, pf, 12, 4, 4 * n, n, 0))) == 0
    host_x = np.zeros((n, 3), np.float32); host_f = np.zeros((5, n), np.float32)
    refused(hiplib, D(host_x.ctypes.data, pf, 0, 0, 0, n, 0), "xyz", before=(good,))                # pageable host memory, second of two
    refused(hiplib, D(px, host_f.ctypes.data, 0, 0, 0, n, 0), "feat")
    refused(hiplib, D(px + 2, pf, 0, 0, 0, n, 0), "xyz")                                            # misaligned bases
    refused(hiplib, D(px, pf + 1, 0, 0, 0, n, 0), "feat")
    refused(hiplib, D(None, pf, 0, 0, 0, n, 0), "xyz")                                              # null with n > 0
    refused(hiplib, D(px, None, 0, 0, 0, n, 0), "feat")
    refused(hiplib, D(px, pf, -12, 0, 0, n, 0), "xyz_stride")                                       # each bad stride
    refused(hiplib, D(px, pf, 14, 0, 0, n, 0), "xyz_stride")
    for s in (4, 8):
        refused(hiplib, D(px, pf, s, 0, 0, n, 0), "xyz_stride")                                     # 1 .. 11
    refused(hiplib, D(px, pf, 0, -4, 4 * n, n, 0), "feat_point_stride")
    refused(hiplib, D(px, pf, 0, 6, 4 * n, n, 0), "feat_point_stride")
    refused(hiplib, D(px, pf, 0, 4, -4 * n, n, 0), "feat_channel_stride")
    refused(hiplib, D(px, pf, 0, 4, 4 * n + 2, n, 0), "feat_channel_stride")
    refused(hiplib, D(px, pf, 0, 4, 0, n, 0), "exactly one")                                        # exactly one of the two is 0
    refused(hiplib, D(px, pf, 0, 0, 4 * n, n, 0), "exactly one")
    refused(hiplib, D(px, pf, 0, 0, 0, 65536, 0), "65535")
    refused(hiplib, D(px, pf, 0, 0, 0, -1, 0), "65535")
    # an extent one float past its allocation: allocations of the runtime's own, so that their ends are known
    hip = loaded_hip()
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; hip.hipFree.argtypes = [C.c_void_p]
    ax, af = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(ax), 12 * n) == 0 and hip.hipMalloc(C.byref(af), 20 * n) == 0
    try:
        assert L.cvo_check_device_clouds(0, 1, (D * 1)(D(ax.value, af.value, 0, 0, 0, n, 0))) == 0, L.cvo_last_error().decode()   # both end where the allocations end
        assert L.cvo_check_device_clouds(0, 1, (D * 1)(D(ax.value + 12, af.value + 4, 0, 0, 0, n - 1, 0))) == 0
        refused(hiplib, D(ax.value + 4, af.value, 0, 0, 0, n, 0), "xyz")
        refused(hiplib, D(ax.value, af.value + 4, 0, 0, 0, n, 0), "feat")
        refused(hiplib, D(ax.value, af.value, 16, 0, 0, n, 0), "xyz")                               # a stride that walks out
        refused(hiplib, D(ax.value, af.value, 0, 4, 4 * n + 4, n, 0), "feat")
        refused(hiplib, D(ax.value, af.value, 0, 20, 4, n + 1, 0), "xyz")
    finally:
        hip.hipFree(ax); hip.hipFree(af)
    torch.zeros(1, device="cuda").sum().item()                                                      # the device still answers: no sticky error left behind


def test_a_refused_call_changes_nothing(hiplib, torch, frame_clouds):
    D = hiplib.api.DeviceCloud
    L = hiplib.api.load_library()
    ip = C.POINTER(C.c_int)
    dev = lambda i, k: (up(torch, frame_clouds[i][k][0]), up(torch, frame_clouds[i][k][1]))
    ids = np.array([0, 1], np.int32)

    def bad_descs(k):
        good = dev(0, k)
        host = np.ascontiguousarray(frame_clouds[1][k][0])
        return (D * 2)(hiplib.api.device_cloud(*good), D(host.ctypes.data, good[1].data_ptr(), 0, 0, 0, host.shape[0], 0)), (good, host)

    # tracker streams: a refused third step between two good ones; an undisturbed object gives the same results
    T, U = hiplib.CvoTracks(2), hiplib.CvoTracks(2)
    for k in range(2):
        for X in (T, U):
            X.step_clouds([0, 1], [dev(0, k), dev(1, k)])
    descs, keep = bad_descs(2)
    torch.cuda.synchronize()
    rc = L.cvo_tracks_step_device_clouds_async(T.h, 2, ids.ctypes.data_as(ip), descs, None, None)
    assert rc == INVALID and "cloud 1" in L.cvo_last_error().decode()
    got, want = T.step_clouds([0, 1], [dev(0, 2), dev(1, 2)]), U.step_clouds([0, 1], [dev(0, 2), dev(1, 2)])
    for p in range(2):
        assert got[p]["phase"] == 2
        same_step(got[p], want[p], p)
    T.close(); U.close()
    # batch slots
    Bt, Bu = hiplib.CvoBatch(2), hiplib.CvoBatch(2)
    for B in (Bt, Bu):
        B.advance_clouds([0, 1], [dev(0, 0), dev(1, 0)])
    rc = L.cvo_batch_advance_device_clouds(Bt.h, 2, ids.ctypes.data_as(ip), descs, None)
    assert rc == INVALID and "cloud 1" in L.cvo_last_error().decode()
    twice = np.array([1, 1], np.int32)
    gd = (D * 2)(hiplib.api.device_cloud(*keep[0]), hiplib.api.device_cloud(*keep[0]))
    assert L.cvo_batch_advance_device_clouds(Bt.h, 2, twice.ctypes.data_as(ip), gd, None) == INVALID   # a slot listed twice
    for B in (Bt, Bu):
        B.advance_clouds([0, 1], [dev(0, 1), dev(1, 1)])
    got, want = Bt.align_pairs([0, 1]), Bu.align_pairs([0, 1])
    for p in range(2):
        assert want[p]["status"] == 0
        same_pair_result(got[p], want[p], p)
    Bt.close(); Bu.close()
