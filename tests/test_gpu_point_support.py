"""Per-point support (cvo_point_support, cvo_batch_point_support(_device), cvo_tracks_point_support(_device)): the terms
function_inner_product sums over two clouds, kept per point.  The yardstick is tests/support_reading.py, a dense numpy reading that
tests/test_support_reading.py holds against the C++ oracle; count arrays must be EQUAL to it, sums agree to rtol 1e-6 (atol 0: the terms
are positive, a point's relative error is bounded by a term's), and every other form must give the handle form's bits."""
import ctypes as C

import numpy as np
import pytest

import support_reading
from helpers import make_tf

pytestmark = pytest.mark.gpu

FIXED, MOVING, PREVIOUS = 0, 1, 2
ODO, KEY = 0, 1
ERR_EMPTY, ERR_INVALID = 2, 4
CASES = [(77, 800), (31, 700), (5, 200)]
ELLS = [0.15, 0.03]
RTOL = 1e-6
KEYS = ("sum_moving", "count_moving", "sum_fixed", "count_fixed")


def small_tf():
    return make_tf([0.2, 1, 0.1], 0.01, [0.004, -0.002, 0.003])


@pytest.fixture(scope="module")
def pairs():
    from cvo_slam_amd import synth
    return {c: synth.make_small_pair(*c) for c in CASES}


def handle_for(hiplib, fixed, moving, ell):
    """a handle with (fixed, moving) in its slots and the given ell; each a (xyz, feat) tuple"""
    g = hiplib.Cvo(); g.set_pcd(*fixed); g.set_pcd(*moving); g.set_state(np.eye(3), np.zeros(3), ell)
    return g


def check_against_reading(got, a, b, ell, tf, where):
    """got = (sum_a, count_a, sum_b, count_b) of clouds a (rows) and b (columns), each (xyz, feat)"""
    want = support_reading.point_support(a[0], a[1], b[0], b[1], ell, tf)
    for side in (0, 2):
        print(where, "ab"[side // 2], "pairs", int(want[side + 1].sum()), "points with support", int((want[side + 1] > 0).sum()),
              "max rel", float(np.max(np.abs(got[side] - want[side]) / np.maximum(want[side], 1e-300))))
        np.testing.assert_array_equal(got[side + 1], want[side + 1], err_msg=str((where, side)))
        np.testing.assert_allclose(got[side].astype(np.float64), want[side], rtol=RTOL, atol=0, err_msg=str((where, side)))
        assert got[side].dtype == np.float32 and got[side + 1].dtype == np.int32
    return want


def same_bits(x, y, where=""):
    assert len(x) == len(y), where
    for k, (u, v) in enumerate(zip(x, y)):
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), (where, k)


# ---- 1, 2. the handle form against the reading and against cvo_function_inner_product
@pytest.mark.parametrize("moved", [False, True], ids=["as_stored", "moved"])
@pytest.mark.parametrize("ell", ELLS)
@pytest.mark.parametrize("case", CASES)
def test_handle_form_against_the_reading_and_the_total(hiplib, pairs, case, ell, moved):
    p = pairs[case]
    tf = small_tf() if moved else None
    g = handle_for(hiplib, (p.fixed.xyz, p.fixed.feat), (p.moving.xyz, p.moving.feat), ell)
    got = g.point_support(MOVING, tf, FIXED)
    want = check_against_reading(got, (p.moving.xyz, p.moving.feat), (p.fixed.xyz, p.fixed.feat), ell, tf, (case, ell, moved))
    assert int(want[1].sum()) > 0
    # the existing entry point, same arguments: counts add up to num (0 where it reads 1), sums to value
    value, num, _ = g.function_inner_product(MOVING, tf, FIXED)
    total_a, total_b = int(got[1].sum(dtype=np.int64)), int(got[3].sum(dtype=np.int64))
    assert total_a == total_b and (total_a if total_a else 1) == num
    assert float(got[0].sum(dtype=np.float64)) == pytest.approx(value, rel=1e-6)
    assert float(got[2].sum(dtype=np.float64)) == pytest.approx(value, rel=1e-6)
    # one direction alone gives the same bits (the other is not computed: its arrays are not there to write)
    n = case[1]
    sa = np.zeros(n, np.float32); ca = np.zeros(n, np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    t = None if tf is None else np.ascontiguousarray(tf, np.float32).reshape(12)
    rc = g.L.cvo_point_support(g.h, MOVING, None if t is None else t.ctypes.data_as(fp), FIXED, sa.ctypes.data_as(fp), ca.ctypes.data_as(ip), n, None, None, 0)
    assert rc == 0
    same_bits((sa, ca), got[:2])
    g.close()


def test_empty_overlap_gives_zeros(hiplib, pairs):
    p = pairs[(5, 200)]
    far = p.moving.xyz + np.array([10, 0, 0], np.float32)
    g = handle_for(hiplib, (p.fixed.xyz, p.fixed.feat), (far, p.moving.feat), 0.15)
    got = g.point_support(MOVING, None, FIXED)
    assert g.function_inner_product(MOVING, None, FIXED)[1] == 1       # cvo.cpp:455-456: the total's rule ...
    for a in got:
        assert not a.any()                                             # ... is not a point's
    g.close()


# ---- 3. the cull's edge cases (tests/test_gpu_parity.py::test_score_box_cull_edge_cases)
@pytest.mark.parametrize("case", ["shuffled", "behind_camera", "tiny", "ragged_33", "wide_ell"])
def test_support_box_cull_edge_cases(hiplib, pairs, case):
    """These clouds exercise ordering and padding but not skipping (in random order every group's box spans the scene);
    tests/test_gpu_sweep_cases.py runs the clouds on which groups are skipped."""
    rng = np.random.default_rng(5)
    p = pairs[(31, 700)]
    fx, ff, mx, mf = p.fixed.xyz.copy(), p.fixed.feat.copy(), p.moving.xyz.copy(), p.moving.feat.copy()
    ell = 0.03
    if case == "shuffled":
        a, b = rng.permutation(fx.shape[0]), rng.permutation(mx.shape[0])
        fx, ff, mx, mf = fx[a], ff[:, a], mx[b], mf[:, b]
    elif case == "behind_camera":
        fx[:, 2] -= 1.2; mx[:, 2] -= 1.2
        assert (fx[:, 2] < 0).any() and (fx[:, 2] > 0).any()
    elif case == "tiny":
        fx, ff, mx, mf = fx[:7], ff[:, :7], mx[:5], mf[:, :5]
        mx[:] = fx[:5] + 0.002
    elif case == "ragged_33":
        fx, ff, mx, mf = fx[:97], ff[:, :97], mx[:33], mf[:, :33]
        mx[:] = fx[:33] + np.float32(0.003)
    elif case == "wide_ell":
        ell = 0.15
    fx, ff, mx, mf = (np.ascontiguousarray(v) for v in (fx, ff, mx, mf))
    tf = small_tf()
    g = handle_for(hiplib, (fx, ff), (mx, mf), ell)
    clouds = {FIXED: (fx, ff), MOVING: (mx, mf)}
    hits = 0
    for (sa, t, sb) in ((MOVING, None, FIXED), (MOVING, tf, FIXED), (FIXED, None, FIXED), (MOVING, None, MOVING), (FIXED, tf, MOVING)):
        got = g.point_support(sa, t, sb)
        want = check_against_reading(got, clouds[sa], clouds[sb], ell, t, (case, sa, sb, t is not None))
        hits += int(want[1].sum())
    assert hits > 0
    g.close()


@pytest.mark.parametrize("rows", [1, 31, 32, 33, 63, 64, 65])
def test_support_row_counts_around_a_wave(hiplib, pairs, rows):
    """rows of one wave, one short of it, one past it, around half a wave (a 32-point group) -- against 129 columns (four groups and one point),
    and the roles swapped"""
    p = pairs[(31, 700)]
    bx, bf = np.ascontiguousarray(p.fixed.xyz[:129]), np.ascontiguousarray(p.fixed.feat[:, :129])
    ax = np.ascontiguousarray(p.fixed.xyz[:rows] + np.float32(0.003)); af = np.ascontiguousarray(p.moving.feat[:, :rows])
    tf = small_tf()
    g = handle_for(hiplib, (bx, bf), (ax, af), 0.15)
    for (sa, a, sb, b) in ((MOVING, (ax, af), FIXED, (bx, bf)), (FIXED, (bx, bf), MOVING, (ax, af))):
        for t in (None, tf):
            want = check_against_reading(g.point_support(sa, t, sb), a, b, 0.15, t, (rows, sa, t is not None))
            assert int(want[1].sum()) >= rows
    g.close()


def test_support_past_one_ballot_round(hiplib):
    """2049 columns are 65 groups: a wave tests 64 group boxes per ballot, so the 65th -- one point -- is reached only in the sweep's second round.
    65 rows (a wave and one row) sit on columns 1984..2048; then the roles swapped, 2049 rows against 65 columns.  The same arguments through
    function_inner_product: two row blocks make the host deal 16 column chunks of 5 groups, so the score kernel runs ranges that end before, at
    and after group 65, empty ones included."""
    from cvo_slam_amd import synth
    p = synth.make_small_pair(31, 2100)
    bx, bf = np.ascontiguousarray(p.fixed.xyz[:2049]), np.ascontiguousarray(p.fixed.feat[:, :2049])
    ax = np.ascontiguousarray(p.fixed.xyz[1984:2049] + np.float32(0.003)); af = np.ascontiguousarray(p.moving.feat[:, 1984:2049])
    assert bx.shape[0] == 2049 and ax.shape[0] == 65
    ell = 0.15
    g = handle_for(hiplib, (bx, bf), (ax, af), ell)
    for t in (None, small_tf()):
        # the precondition, on the reading: the 65th group's only column is hit, and so is a column of every other group
        want = support_reading.point_support(ax, af, bx, bf, ell, t)
        assert want[3][2048] >= 1
        assert all(want[3][32 * k:32 * k + 32].any() for k in range(65))
        for (sa, a, sb, b) in ((MOVING, (ax, af), FIXED, (bx, bf)), (FIXED, (bx, bf), MOVING, (ax, af))):
            got = g.point_support(sa, t, sb)
            check_against_reading(got, a, b, ell, t, ("second round", sa, t is not None))
            value, num, _ = g.function_inner_product(sa, t, sb)
            total_a, total_b = int(got[1].sum(dtype=np.int64)), int(got[3].sum(dtype=np.int64))
            assert total_a > 0 and total_a == total_b == num
            assert float(got[0].sum(dtype=np.float64)) == pytest.approx(value, rel=1e-6)
            assert float(got[2].sum(dtype=np.float64)) == pytest.approx(value, rel=1e-6)
    g.close()


# ---- 4. a cloud against itself
def test_a_cloud_against_itself_is_symmetric(hiplib, pairs):
    p = pairs[(77, 800)]
    for ell in ELLS:
        g = handle_for(hiplib, (p.fixed.xyz, p.fixed.feat), (p.moving.xyz, p.moving.feat), ell)
        sa, ca, sb, cb = g.point_support(FIXED, None, FIXED)
        assert (ca >= 1).all()                                          # every point is inside with itself
        same_bits((sa, ca), (sb, cb), ell)
        check_against_reading((sa, ca, sb, cb), (p.fixed.xyz, p.fixed.feat), (p.fixed.xyz, p.fixed.feat), ell, None, ("self", ell))
        g.close()


# ---- 5, 6. the batch form: the handle form's bits, whoever shares the launch
SIZES = [200, 300, 400, 500, 600, 700, 800, 650]


@pytest.fixture(scope="module")
def aligned_batch(hiplib):
    """eight pairs of 200 ... 800 points, aligned once; what the handle form gives for every pair at its result transform and ell"""
    from cvo_slam_amd import synth
    ps = [synth.make_small_pair(100 + i, n) for i, n in enumerate(SIZES)]
    b = hiplib.CvoBatch(8)
    for i, p in enumerate(ps):
        b.set_pair(i, p.fixed.xyz, p.fixed.feat, p.moving.xyz, p.moving.feat)
    res = b.align(8)
    assert all(r["status"] == 0 for r in res)
    want = []
    for p, r in zip(ps, res):
        g = handle_for(hiplib, (p.fixed.xyz, p.fixed.feat), (p.moving.xyz, p.moving.feat), r["ell"])
        want.append(g.point_support(MOVING, r["transform"], FIXED))
        assert want[-1][1].sum() > 0
        g.close()
    yield b, ps, res, want
    b.close()


def test_the_same_call_twice_gives_the_same_bits(hiplib, pairs):
    p = pairs[(77, 800)]
    g = handle_for(hiplib, (p.fixed.xyz, p.fixed.feat), (p.moving.xyz, p.moving.feat), 0.15)
    first = g.point_support(MOVING, small_tf(), FIXED)
    for _ in range(2):
        same_bits(g.point_support(MOVING, small_tf(), FIXED), first)
    g.close()


def test_batch_form_equals_the_handle_form(aligned_batch):
    b, ps, res, want = aligned_batch
    got = b.point_support()
    assert len(got) == 8
    for i in range(8):
        same_bits([got[i][k] for k in KEYS], want[i], i)
    same_bits([b.point_support()[3][k] for k in KEYS], want[3], "again")
    # one pair asked alone, and among the eight requests of one launch
    for i in (0, 3, 7):
        alone = b.point_support([i])
        assert len(alone) == 1
        same_bits([alone[0][k] for k in KEYS], want[i], ("alone", i))
    # a permuted subset: the results are those pairs'
    sub = [5, 2, 7, 0]
    got = b.point_support(sub)
    for k, i in enumerate(sub):
        same_bits([got[k][key] for key in KEYS], want[i], ("subset", i))


# ---- 7. the device form
def guarded(torch, n, dtype, pad=64):
    """an n-entry array sliced out of a larger 0xA5-filled allocation"""
    big = torch.full((4 * (n + 2 * pad),), 0xA5, dtype=torch.uint8, device="cuda")
    return big, big.view(dtype)[pad:pad + n]


def guards_intact(big, n, pad=64):
    raw = big.cpu().numpy()
    return (raw[:4 * pad] == 0xA5).all() and (raw[4 * (pad + n):] == 0xA5).all()


@pytest.mark.parametrize("side_stream", [True, False], ids=["out_stream", "host_wait"])
def test_device_form_equals_the_host_form(aligned_batch, side_stream):
    import torch
    b, ps, res, want = aligned_batch
    sub = [6, 1, 4]
    out, bigs = [], []
    for i in sub:
        n = SIZES[i]
        rec = {}
        for key in KEYS:
            big, arr = guarded(torch, n, torch.float32 if key.startswith("sum") else torch.int32)
            rec[key] = arr; bigs.append((big, n))
        out.append(rec)
    if side_stream:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())                    # the fills above
        b.point_support(sub, out=out, out_stream=s)
        s.synchronize()
    else:
        b.point_support(sub, out=out)
    for k, i in enumerate(sub):
        same_bits([out[k][key].cpu().numpy() for key in KEYS], want[i], ("device", i))
    assert all(guards_intact(big, n) for big, n in bigs)
    # one direction only: the other pair's arrays are not there to write
    big_s, sm = guarded(torch, SIZES[2], torch.float32); big_c, cm = guarded(torch, SIZES[2], torch.int32)
    b.point_support([2], out=[dict(sum_moving=sm, count_moving=cm)])
    same_bits((sm.cpu().numpy(), cm.cpu().numpy()), want[2][:2])
    assert guards_intact(big_s, SIZES[2]) and guards_intact(big_c, SIZES[2])


def test_device_form_refuses_what_it_cannot_write(hiplib, aligned_batch):
    import torch
    b, ps, res, want = aligned_batch
    n = SIZES[0]
    good = lambda: dict(sum_moving=guarded(torch, n, torch.float32)[1], count_moving=guarded(torch, n, torch.int32)[1],
                        sum_fixed=guarded(torch, n, torch.float32)[1], count_fixed=guarded(torch, n, torch.int32)[1])
    # a short tensor, a wrong dtype, a strided view, host memory: refused before the library is called
    for key, bad in (("sum_moving", torch.zeros(n - 1, dtype=torch.float32, device="cuda")), ("count_fixed", torch.zeros(n, dtype=torch.int64, device="cuda")),
                     ("sum_fixed", torch.zeros(n, dtype=torch.int32, device="cuda")), ("count_moving", torch.zeros(2 * n, dtype=torch.int32, device="cuda")[::2]),
                     ("sum_moving", np.zeros(n, np.float32))):
        rec = good(); rec[key] = bad
        with pytest.raises(ValueError):
            b.point_support([0], out=[rec])
    # the library's own check: pageable host memory, a misaligned array -- CVO_ERR_INVALID, nothing written
    from cvo_slam_amd.api import PointSupportDst
    L = b.L
    host = [np.full(n, 7, np.float32), np.full(n, 7, np.int32), np.full(n, 7, np.float32), np.full(n, 7, np.int32)]
    rec = (PointSupportDst * 1)(); idx = (C.c_int * 1)(0)
    for key, a in zip(KEYS, host):
        setattr(rec[0], key, a.ctypes.data)
    assert L.cvo_batch_point_support_device(b.h, 1, idx, rec, None) == ERR_INVALID
    assert all((a == 7).all() for a in host)
    dev = good()
    for key in KEYS:
        setattr(rec[0], key, dev[key].data_ptr())
    rec[0].sum_fixed = dev["sum_fixed"].data_ptr() + 2
    assert L.cvo_batch_point_support_device(b.h, 1, idx, rec, None) == ERR_INVALID
    torch.cuda.synchronize()
    for key in KEYS:
        assert (dev[key].cpu().numpy().view(np.uint8) == 0xA5).all(), key       # nothing was queued
    # and the batch still answers
    same_bits([b.point_support([0])[0][k] for k in KEYS], want[0])


# ---- 8. a score block in flight is not disturbed
def test_score_block_in_flight_is_undisturbed(aligned_batch):
    b, ps, res, want = aligned_batch
    b.enqueue_innerproduct(8)
    plain = bytes(b.innerproduct_results_raw(8))
    b.enqueue_innerproduct(8)
    got = b.point_support()
    between = bytes(b.innerproduct_results_raw(8))
    assert between == plain
    for i in range(8):
        same_bits([got[i][k] for k in KEYS], want[i], i)


# ---- 9. tracker streams
def test_tracker_streams_equal_the_two_handle_loop(hiplib):
    """Streams 0, 2, 3 stepped to a step in which they are in phase 2, 1 and 0; stream 1 sits the step out.  Support of both objects equals, bit for
    bit, what the two-handle loop's objects give at the same frame for (MOVING, their transform, FIXED); everything else is refused."""
    from cvo_slam_amd import synth
    NUM_WANT = 500
    frames = [synth.make_sequence(40 + i, n_frames=3)[0] for i in range(2)]
    cam = synth.camera_tuple(synth.TUM1)
    seq_of = {0: 0, 1: 0, 2: 1, 3: 1}
    T = hiplib.CvoTracks(4); T.set_num_want(NUM_WANT)
    T.step([0, 1], [frames[0][0], frames[0][0]], cam)
    T.step([0, 1, 2], [frames[0][1], frames[0][1], frames[1][0]], cam)
    with pytest.raises(hiplib.CvoError) as e:                          # a phase-1 step was waited for: object 1 has nothing
        T.point_support(KEY, [0])
    assert e.value.code == ERR_INVALID
    res = T.step([0, 2, 3], [frames[0][2], frames[1][1], frames[1][0]], cam)
    assert [r["phase"] for r in res] == [2, 1, 0]
    assert res[0]["odometry"]["status"] == 0 and res[0]["keyframe"]["status"] == 0 and res[1]["odometry"]["status"] == 0
    assert all(0 < r["points"] <= 800 for r in res)

    # the two-handle loop of streams 0 and 2 (tests/test_gpu_tracks.py::test_clouds_of_both_objects_equal_the_handles)
    want = {}
    for s, last in ((0, 2), (2, 1)):
        fr = frames[seq_of[s]]
        odo, kf = hiplib.Cvo(), hiplib.Cvo()
        odo.set_num_want(NUM_WANT); kf.set_num_want(NUM_WANT)
        odo.set_pcd_images(*fr[0], cam); kf.set_pcd_images(*fr[0], cam)
        for k in range(1, last + 1):
            t = odo.match_odometry_images(*fr[k], cam).astype(np.float32)
            if k == 1:
                kf.first_frame = False; kf.reset_transform(t)
            else:
                kf.reset_initial(t); kf.match_keyframe_images(*fr[k], cam)
            if k == last:
                want[(s, ODO)] = odo.point_support(MOVING, odo.transform, FIXED)
                if k >= 2:
                    want[(s, KEY)] = kf.point_support(MOVING, kf.transform, FIXED)
            odo.update_fixed_pcd()
        odo.close(); kf.close()

    def refused(obj, streams):
        with pytest.raises(hiplib.CvoError) as e:
            T.point_support(obj, streams)
        assert e.value.code == ERR_INVALID

    before = [T.get_state(s, o) for s in range(4) for o in (ODO, KEY)]
    refused(ODO, [1])                                                  # not in the step
    refused(ODO, [0, 1])                                               # ... whoever else is listed
    refused(ODO, [3]); refused(KEY, [3])                               # phase 0: nothing aligned
    refused(KEY, [2])                                                  # phase 1: the keyframe object did not align
    refused(2, [0])                                                    # no such object
    after = [T.get_state(s, o) for s in range(4) for o in (ODO, KEY)]
    for x, y in zip(before, after):
        assert all(np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes() for k in x)

    got = T.point_support(ODO, [2, 0])
    same_bits([got[0][k] for k in KEYS], want[(2, ODO)], "odometry of stream 2")
    same_bits([got[1][k] for k in KEYS], want[(0, ODO)], "odometry of stream 0")
    got = T.point_support(KEY, [0])
    same_bits([got[0][k] for k in KEYS], want[(0, KEY)], "keyframe of stream 0")
    assert want[(0, KEY)][1].sum() > 0 and want[(0, ODO)][1].sum() > 0

    import torch                                                       # the device form, for the keyframe object
    n_m, n_f = want[(0, KEY)][0].shape[0], want[(0, KEY)][2].shape[0]
    out = [dict(sum_moving=torch.zeros(n_m, dtype=torch.float32, device="cuda"), count_moving=torch.zeros(n_m, dtype=torch.int32, device="cuda"),
                sum_fixed=torch.zeros(n_f, dtype=torch.float32, device="cuda"), count_fixed=torch.zeros(n_f, dtype=torch.int32, device="cuda"))]
    T.point_support(KEY, [0], out=out)
    same_bits([out[0][k].cpu().numpy() for k in KEYS], want[(0, KEY)], "keyframe of stream 0, device form")

    T.commit([0], [True])
    refused(ODO, [0]); refused(KEY, [0]); refused(ODO, [2])            # after the decision the objects' clouds have moved on
    T.close()


# ---- 10. argument errors
def test_argument_errors_leave_the_outputs_alone(hiplib, pairs, aligned_batch):
    p = pairs[(5, 200)]
    n = 200
    g = handle_for(hiplib, (p.fixed.xyz, p.fixed.feat), (p.moving.xyz, p.moving.feat), 0.15)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    arr = [np.full(n, 7, np.float32), np.full(n, 7, np.int32), np.full(n, 7, np.float32), np.full(n, 7, np.int32)]
    ptr = [arr[0].ctypes.data_as(fp), arr[1].ctypes.data_as(ip), arr[2].ctypes.data_as(fp), arr[3].ctypes.data_as(ip)]
    call = lambda sa, sb, a, ca, cap_a, bb, cb, cap_b: g.L.cvo_point_support(g.h, sa, None, sb, a, ca, cap_a, bb, cb, cap_b)
    assert call(MOVING, FIXED, ptr[0], ptr[1], n - 1, ptr[2], ptr[3], n) == ERR_INVALID        # a cap below the cloud's size
    assert call(MOVING, FIXED, ptr[0], ptr[1], n, ptr[2], ptr[3], n - 1) == ERR_INVALID
    assert call(MOVING, PREVIOUS, ptr[0], ptr[1], n, ptr[2], ptr[3], n) == ERR_EMPTY           # an empty slot
    assert call(PREVIOUS, FIXED, ptr[0], ptr[1], n, ptr[2], ptr[3], n) == ERR_EMPTY
    assert call(MOVING, 7, ptr[0], ptr[1], n, ptr[2], ptr[3], n) == ERR_EMPTY                  # no such slot (as cvo_function_inner_product answers)
    assert call(MOVING, FIXED, None, None, 0, None, None, 0) == ERR_INVALID                    # nothing to compute
    assert call(MOVING, FIXED, ptr[0], None, n, ptr[2], ptr[3], n) == ERR_INVALID              # half a direction
    assert g.L.cvo_point_support(None, MOVING, None, FIXED, ptr[0], ptr[1], n, ptr[2], ptr[3], n) == ERR_INVALID
    assert all((a == 7).all() for a in arr)
    assert call(MOVING, FIXED, ptr[0], ptr[1], n, ptr[2], ptr[3], n) == 0                      # and then it computes
    assert arr[1].sum() > 0 and arr[1].sum() == arr[3].sum()
    g.close()

    from cvo_slam_amd.api import PointSupportDst
    b, ps, res, want = aligned_batch
    L = b.L
    big = [np.full(800, 7, np.float32), np.full(800, 7, np.int32), np.full(800, 7, np.float32), np.full(800, 7, np.int32)]
    rec = (PointSupportDst * 2)()
    for r in rec:
        for key, a in zip(KEYS, big):
            setattr(r, key, a.ctypes.data)
    idx = lambda *v: (C.c_int * len(v))(*v)
    assert L.cvo_batch_point_support(b.h, 1, idx(0), None) == ERR_INVALID                      # NULL dst
    assert L.cvo_batch_point_support(None, 1, idx(0), rec) == ERR_INVALID
    assert L.cvo_batch_point_support(b.h, 1, idx(8), rec) == ERR_INVALID                       # pair index out of range
    assert L.cvo_batch_point_support(b.h, 1, idx(-1), rec) == ERR_INVALID
    assert L.cvo_batch_point_support(b.h, 0, idx(0), rec) == ERR_INVALID
    assert L.cvo_batch_point_support(b.h, 9, None, rec) == ERR_INVALID                         # more pairs than the launch aligned
    assert L.cvo_batch_point_support(b.h, 2, idx(1, 1), rec) == ERR_INVALID                    # listed twice
    rec[0].count_fixed = None
    assert L.cvo_batch_point_support(b.h, 1, idx(0), rec) == ERR_INVALID                       # half a direction
    assert all((a == 7).all() for a in big)
    fresh = hiplib.CvoBatch(2)
    with pytest.raises(hiplib.CvoError) as e:                                                  # nothing was aligned yet
        fresh.point_support([0])
    assert e.value.code == ERR_INVALID
    fresh.close()
