"""Frames in caller-owned device memory (cvo_device_image; cvo_batch_*_device_images, cvo_tracks_step_device_async / _stage_device_async): the
ingest kernel alone against its byte-for-byte definition, then every device entry point against its host twin given the same pixel values --
bits for transforms, states, counts, clouds and selected pixels; the project's score rule for score blocks -- with the caller's tensors
zeroed as early as the ordering rules of include/cvo_hip.h allow, and the refusals of the validation."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tracks_cases import bits

pytestmark = pytest.mark.gpu

FIXED, MOVING, PREVIOUS = 0, 1, 2
ODO, KEY = 0, 1
LENGTHS = [6, 4, 1, 5, 3, 6]                                        # the fixture of tests/test_gpu_staged_steps.py
CAM2 = (5000.0, 535.4, 539.2, 320.1, 247.6)
A, R = True, False
DECISIONS = [[A, A, R, A], [R, A], [], [A, R, R], [R], [R, R, A, R]]
INVALID = 4
FILL = 0x5C                                                         # what lies between and behind the rows of a pitched source


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def seqs():
    from cvo_slam_amd import synth
    frames = [synth.make_sequence(40 + i, n_frames=n)[0] for i, n in enumerate(LENGTHS)]
    cams = [synth.camera_tuple(synth.TUM1) if i % 2 == 0 else CAM2 for i in range(len(LENGTHS))]
    return frames, cams


# ---- 1. the ingest kernel alone
def pitched(pixels, base, pitch, tail=7):
    """a flat uint8 buffer of FILL with the rows of `pixels` (h, row bytes) at base + y * pitch; returns the buffer"""
    h, rb = pixels.shape
    buf = np.full(base + (h - 1) * pitch + rb + tail, FILL, np.uint8)
    for y in range(h):
        buf[base + y * pitch: base + y * pitch + rb] = pixels[y]
    return buf


@pytest.mark.parametrize("w,h", [(64, 64), (67, 65), (100, 66)])
def test_ingest_kernel_is_the_byte_gather(hiplib, torch, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    colour = list(itertools.product((0, 1, 2, 3), (3, 4), (0, 1), (0, 1, 5, 64)))   # base offset, pixel_bytes, swap_rb, pitch - row bytes
    depth = list(itertools.product((0, 2), (0, 2, 6)))                              # base offset, pitch - 2 w
    while len(colour) % 3:
        colour.append(colour[len(colour) % 7])
    for call in range(len(colour) // 3):
        descs, want_b, want_d, keep = [], [], [], []
        for j in range(3):                                          # three images per call, each with another layout
            off, pb, swap, extra = colour[3 * call + j]
            doff, dextra = depth[(3 * call + j) % len(depth)]
            bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)   # the pixel values as the stacks must hold them: B, G, R
            src = np.full((h, w, pb), 0xEE, np.uint8)               # (a fourth byte is ignored)
            src[..., :3] = bgr[..., ::-1] if swap else bgr
            d16 = rng.integers(0, 65536, (h, w), dtype=np.uint16)
            pitch, dpitch = w * pb + extra, 2 * w + dextra
            tb = torch.from_numpy(pitched(src.reshape(h, w * pb), off, pitch)).cuda()
            td = torch.from_numpy(pitched(d16.view(np.uint8).reshape(h, 2 * w), doff, dpitch)).cuda()
            keep += [tb, td]
            descs.append(hiplib.api.DeviceImage(tb.data_ptr() + off, td.data_ptr() + doff, pitch, dpitch, pb, swap))
            want_b.append(bgr); want_d.append(d16)
        torch.cuda.synchronize()
        got_b, got_d, guards = hiplib.api.selftest_ingest_images(descs, w, h)
        assert guards, (call, "guard bytes written")
        for j in range(3):
            assert np.array_equal(got_b[j], want_b[j]), (call, j, colour[3 * call + j])
            assert np.array_equal(got_d[j], want_d[j]), (call, j, depth[(3 * call + j) % len(depth)])


def test_ingest_tight_descriptor_with_pitch_zero(hiplib, torch):
    rng = np.random.default_rng(5)
    w, h = 65, 64
    bgr = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8); d16 = rng.integers(0, 65536, (2, h, w), dtype=np.uint16)
    tb, td = torch.from_numpy(bgr).cuda(), torch.from_numpy(d16.view(np.int16)).cuda()
    descs = [hiplib.api.DeviceImage(tb[k].data_ptr(), td[k].data_ptr(), 0, 0, 3, 0) for k in range(2)]   # image 1: odd 3 n, a base that is no multiple of 4
    torch.cuda.synchronize()
    got_b, got_d, guards = hiplib.api.selftest_ingest_images(descs, w, h)
    assert guards and np.array_equal(got_b, bgr) and np.array_equal(got_d, d16)


# ---- the layouts a stream's frames arrive in (sequence i: layout i mod 3)
def to_device(torch, b, d, layout, rng):
    """(bgr tensor, depth tensor, swap_rb, the tensors to zero afterwards) for one frame"""
    h, w = d.shape
    d = np.ascontiguousarray(d).view(np.int16)
    if layout == 0:                                                 # tight BGR
        tb, td = torch.from_numpy(np.ascontiguousarray(b)).cuda(), torch.from_numpy(d).cuda()
        return tb, td, False, [tb, td]
    if layout == 1:                                                 # a crop of a larger BGRA tensor, first three channels; depth a crop too
        big = rng.integers(0, 256, (h + 5, w + 9, 4), dtype=np.uint8); big[2:2 + h, 3:3 + w, :3] = b
        bigd = rng.integers(0, 30000, (h + 3, w + 5)).astype(np.int16); bigd[1:1 + h, 2:2 + w] = d
        tb, td = torch.from_numpy(big).cuda(), torch.from_numpy(bigd).cuda()
        return tb[2:2 + h, 3:3 + w, :3], td[1:1 + h, 2:2 + w], False, [tb, td]
    tb, td = torch.from_numpy(np.ascontiguousarray(b[..., ::-1])).cuda(), torch.from_numpy(d).cuda()   # RGB
    return tb, td, True, [tb, td]


class Feeder:
    """Uploads the frames of a call in their streams' layouts and zeroes them once the call has returned: on `side` (the image_stream) when
    there is one, else on torch's current stream."""
    def __init__(self, torch, side):
        self.torch, self.side, self.rng = torch, side, np.random.default_rng(11)

    def _ctx(self):
        return self.torch.cuda.stream(self.side) if self.side is not None else self.torch.cuda.stream(self.torch.cuda.current_stream())

    def upload(self, ids, images):
        with self._ctx():
            ups = [to_device(self.torch, b, d, i % 3, self.rng) for i, (b, d) in zip(ids, images)]
        self.own = [t for u in ups for t in u[3]]
        return [(u[0], u[1]) for u in ups], [u[2] for u in ups]

    def wipe(self):
        with self._ctx():
            for t in self.own:
                t.zero_()

    @property
    def image_stream(self):
        return self.side


def check_scores(got, want, rel):                                    # the rule of tests/test_gpu_batch_odometry.py:159-165
    for key in ("inn_pre", "inn_post", "inn_fixed_pcd", "inn_moving_pcd"):
        assert got[key][1] == want[key][1], key
        assert got[key][0] == pytest.approx(want[key][0], rel=rel), key
    assert got["inliers"] == want["inliers"]
    assert got["cos_angle"] == pytest.approx(want["cos_angle"], rel=rel)
    np.testing.assert_allclose(got["post_hessian"], want["post_hessian"], rtol=1e-3, atol=1e-3 * np.abs(want["post_hessian"]).max())


def same_step(got, want, where):
    """the rule of tests/test_gpu_staged_steps.py::same_step: bits for transforms, states, counts; the score rule for score blocks"""
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
    out = []
    for p in range(n):
        for obj in (ODO, KEY):
            st = T.get_state(p, obj)
            out.append(((p, obj, "state"), st["R"].tobytes() + st["T"].tobytes() + np.float32(st["ell"]).tobytes() + st["transform"].tobytes()))
            for slot in (FIXED, MOVING, PREVIOUS):
                xyz, feat = T.get_cloud(p, obj, slot)
                out.append(((p, obj, slot), xyz.tobytes() + feat.tobytes() + T.get_selected_points(p, obj, slot).tobytes()))
    return out


def run_tracks(T, frames, cams, table, feeder=None, staged=False):
    """Sequence i on stream i, every stream that still has a frame in every step.  feeder None: host images through step_async.  Else the
    frames go up in their layouts, through step_async, or (staged) through stage_async between a step's call and its wait and
    step_staged_async, and are zeroed right after the call that took them."""
    n = len(frames)
    steps = [[] for _ in range(n)]
    depth = max(len(f) for f in frames)
    lists = [[i for i in range(n) if len(frames[i]) > k] for k in range(depth)]
    for k in range(depth):
        ids = lists[k]
        if feeder is None:
            T.step_async(ids, [frames[i][k] for i in ids], cams, ids)
        elif staged and k > 0:
            assert T.staged_count()[0] == len(ids)
            T.step_staged_async()
        else:
            ims, sw = feeder.upload(ids, [frames[i][k] for i in ids])
            T.step_async(ids, ims, cams, ids, swap_rb=sw, image_stream=feeder.image_stream)
            feeder.wipe()
        if staged and k + 1 < depth:
            nxt = lists[k + 1]
            ims, sw = feeder.upload(nxt, [frames[i][k + 1] for i in nxt])
            T.stage_async(nxt, ims, cams, nxt, swap_rb=sw, image_stream=feeder.image_stream)   # while step k is in flight
            feeder.wipe()
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
    """the host run of all six sequences on one CvoTracks (step_async), made once: (steps, final clouds and states)"""
    frames, cams = seqs
    T = hiplib.CvoTracks(len(frames))
    steps = run_tracks(T, frames, cams, DECISIONS)
    fin = final_state(T, len(frames))
    T.close()
    return steps, fin


# ---- 2. tracker streams
@pytest.mark.parametrize("side_stream", [True, False])
@pytest.mark.parametrize("staged", [False, True])
def test_tracker_steps_on_device_images_equal_host_images(hiplib, torch, seqs, reference, staged, side_stream):
    frames, cams = seqs
    want, want_fin = reference
    feeder = Feeder(torch, torch.cuda.Stream() if side_stream else None)
    T = hiplib.CvoTracks(len(frames))
    got = run_tracks(T, frames, cams, DECISIONS, feeder, staged)
    for i in range(len(frames)):
        assert len(got[i]) == LENGTHS[i]
        for k, (a, b) in enumerate(zip(got[i], want[i])):
            same_step(a, b, (i, k))
    fin = final_state(T, len(frames))
    for (what, a), (_, b) in zip(fin, want_fin):
        assert a == b, what
    assert T.staged_count() == (0, sum(LENGTHS) - len(LENGTHS) if staged else 0)
    T.close()
    torch.cuda.synchronize()


# ---- 3. batch slots
def run_batch(B, frames, cams, feeder=None, staged=False):
    n = len(frames)
    depth = max(len(f) for f in frames)
    lists = [[i for i in range(n) if len(frames[i]) > k] for k in range(depth)]
    out = [[] for _ in range(n)]

    def advance(ids, k):
        if feeder is None:
            return B.advance_images(ids, [frames[i][k] for i in ids], cams, ids)
        ims, sw = feeder.upload(ids, [frames[i][k] for i in ids])
        pts = B.advance_images(ids, ims, cams, ids, swap_rb=sw, image_stream=feeder.image_stream)
        feeder.wipe()
        return pts
    pts = advance(lists[0], 0)
    for k in range(depth):
        ids = lists[k]
        nl = B.align_pairs_async(ids) if k else 0
        if staged and k + 1 < depth:
            nxt = lists[k + 1]
            ims, sw = feeder.upload(nxt, [frames[i][k + 1] for i in nxt])
            B.stage_images(nxt, ims, cams, nxt, swap_rb=sw, image_stream=feeder.image_stream)   # while the launch runs
            feeder.wipe()
        res = B.wait(nl) if k else [None] * len(ids)
        for i, r, p in zip(ids, res, pts):
            out[i].append((int(p), r, None if r is None else B.prev_accum_transform(i)))
        if k + 1 < depth:
            nxt = lists[k + 1]
            if staged:
                assert B.staged_count()[0] == len(nxt)
                pts = B.advance_staged()
            else:
                pts = advance(nxt, k + 1)
    return out


@pytest.mark.parametrize("staged", [False, True])
def test_batch_slots_on_device_images_equal_host_images(hiplib, torch, seqs, staged):
    frames, cams = seqs[0][:3], seqs[1][:3]                          # three slots, two cameras, one sequence of a single frame
    U, S = hiplib.CvoBatch(3), hiplib.CvoBatch(3)
    want = run_batch(U, frames, cams)
    got = run_batch(S, frames, cams, Feeder(torch, torch.cuda.Stream()), staged)
    for i in range(3):
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
    for p in range(3):
        for slot in (FIXED, MOVING):
            (gx, gf), (wx, wf) = S.get_cloud(p, slot), U.get_cloud(p, slot)
            assert gx.tobytes() == wx.tobytes() and gf.tobytes() == wf.tobytes(), (p, slot)
            assert S.get_selected_points(p, slot).tobytes() == U.get_selected_points(p, slot).tobytes(), (p, slot)
    assert S.staged_count() == (0, sum(LENGTHS[:3]) - 3 if staged else 0)
    U.close(); S.close()
    torch.cuda.synchronize()


def test_set_pairs_on_device_images_equal_host_images(hiplib, torch):
    from cvo_slam_amd import synth
    cam = synth.camera_tuple(synth.ETH3D)
    images = []
    for i in (1, 2):
        (fa, da), (fb, db), _ = synth.make_frames(i, cam=synth.ETH3D)
        images += [(fa, da), (fb, db)]
    assert images[0][1].shape == (456, 736)
    fixed, moving = [0, 2, 3], [1, 3, 0]                             # 4 images, 3 pairs
    U, S = hiplib.CvoBatch(3), hiplib.CvoBatch(3)
    wp = U.set_pairs_images(images, fixed, moving, cam)
    feeder = Feeder(torch, None)
    ims, sw = feeder.upload([0, 1, 2, 3], images)                    # (layouts 0, 1, 2, 0)
    gp = S.set_pairs_images(ims, fixed, moving, cam, swap_rb=sw)
    feeder.wipe()
    assert list(gp) == list(wp)
    for p in range(3):
        for slot in (FIXED, MOVING):
            (gx, gf), (wx, wf) = S.get_cloud(p, slot), U.get_cloud(p, slot)
            assert gx.tobytes() == wx.tobytes() and gf.tobytes() == wf.tobytes(), (p, slot)
            assert S.get_selected_points(p, slot).tobytes() == U.get_selected_points(p, slot).tobytes(), (p, slot)
    for g, w in zip(S.align(3), U.align(3)):
        assert g["status"] == w["status"]
        for key in ("transform", "R", "T"):
            assert g[key].tobytes() == w[key].tobytes(), key
        assert (g["iter"], g["A_nonzero"], g["iterations_run"]) == (w["iter"], w["A_nonzero"], w["iterations_run"])
    U.close(); S.close()
    torch.cuda.synchronize()


# ---- 4. refusals: through cvo_check_device_images only, nothing is launched
def refused(hiplib, desc, w, h, word):
    arr = (hiplib.api.DeviceImage * 1)(desc)
    rc = hiplib.api.load_library().cvo_check_device_images(0, 1, arr, w, h)
    msg = hiplib.api.load_library().cvo_last_error().decode()
    assert rc == INVALID, (rc, msg)
    assert word in msg and "image 0" in msg, msg


def test_refusals_name_the_field(hiplib, torch):
    w, h = 64, 64
    tb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda"); td = torch.zeros((h, w), dtype=torch.int16, device="cuda")
    D = hiplib.api.DeviceImage
    pb, pd = tb.data_ptr(), td.data_ptr()
    assert hiplib.api.load_library().cvo_check_device_images(0, 1, (D * 1)(D(pb, pd, 0, 0, 3, 0)), w, h) == 0
    host = np.zeros((h, w, 3), np.uint8)
    refused(hiplib, D(host.ctypes.data, pd, 0, 0, 3, 0), w, h, "bgr8")          # pageable host memory
    refused(hiplib, D(pb, pd, 0, 0, 5, 0), w, h, "pixel_bytes")
    refused(hiplib, D(pb, pd, 3 * w - 1, 0, 3, 0), w, h, "bgr_pitch")            # one byte short
    refused(hiplib, D(pb, pd, 0, 2 * w - 1, 3, 0), w, h, "depth_pitch")
    refused(hiplib, D(pb, pd + 1, 0, 0, 3, 0), w, h, "depth16")                  # an odd depth pointer
    refused(hiplib, D(None, pd, 0, 0, 3, 0), w, h, "bgr8")                       # null
    refused(hiplib, D(pb, None, 0, 0, 3, 0), w, h, "depth16")
    refused(hiplib, D(pb, pd, 0, 0, 3, 2), w, h, "swap_rb")
    torch.zeros(1, device="cuda").sum().item()                                   # the device still answers: no sticky error left behind


def test_a_refused_step_changes_nothing(hiplib, torch, seqs):
    frames, cams = seqs
    T = hiplib.CvoTracks(2)
    ids = [0, 1]
    T.step(ids, [frames[i][0] for i in ids], cams, ids)
    up = lambda k: [(torch.from_numpy(np.ascontiguousarray(frames[i][k][0])).cuda(), torch.from_numpy(frames[i][k][1].view(np.int16)).cuda()) for i in ids]
    T.step(ids, up(1), cams, ids)
    T.stage_async(ids, up(2), cams, ids)
    before = final_state(T, 2)
    good = up(2)
    h, w = frames[0][2][1].shape
    D = hiplib.api.DeviceImage
    host = np.ascontiguousarray(frames[1][2][0])
    descs = (D * 2)(hiplib.api.device_image(*good[0])[0], D(host.ctypes.data, good[1][1].data_ptr(), 0, 0, 3, 0))
    sl = np.array(ids, np.int32); cam = (hiplib.api.Camera * 2)(*[hiplib.api.Camera(*[float(v) for v in c]) for c in cams[:2]])
    L = hiplib.api.load_library()
    rc = L.cvo_tracks_step_device_async(T.h, 2, sl.ctypes.data_as(C.POINTER(C.c_int)), descs, w, h, cam, sl.ctypes.data_as(C.POINTER(C.c_int)), None, None)
    assert rc == INVALID and "image 1" in L.cvo_last_error().decode()
    assert T.staged_count()[0] == 2                                  # the stage is kept
    after = final_state(T, 2)
    for (what, a), (_, b) in zip(after, before):
        assert a == b, what
    res = T.step_staged()                                            # ... and the streams go on from where they were
    assert [r["phase"] for r in res] == [2, 2] and all(r["odometry"]["status"] == 0 for r in res)
    T.close()
