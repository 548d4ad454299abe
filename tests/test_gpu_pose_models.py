"""Pose models (cvo_pose_models, cvo_batch_pose_models, cvo_batch_result_models): value, se(3) gradient and Hessian of the inner product at K poses
per pair in one launch.  The yardstick is tests/pose_model_reading.py, a dense numpy reading that tests/test_pose_model_reading.py holds against
central differences of the energy: num must be EQUAL to it, value agree to rtol 1e-6 (the bound of tests/test_gpu_hypotheses.py), and every entry
of grad and hess lie within 1e-6 of its MAGNITUDE (the same sum with every factor replaced by its absolute value): a term carries at most 16 float
roundings of 2^-24, 9.5e-7 of its magnitude, and the double sums add nothing at this scale; the reading's own float32 terms sit within 4e-9 of
float64 ones.  value and num must be the bytes of score_hypotheses, hess symmetric bit for bit, and every other form give the handle form's bytes."""
import ctypes as C

import numpy as np
import pytest

import hypothesis_reading as hr
import pose_model_reading as pm
import support_reading
from helpers import make_tf

pytestmark = pytest.mark.gpu

FIXED, MOVING = 0, 1
ERR_EMPTY, ERR_INVALID = 2, 4
RTOL = 1e-6
MAG_TOL = 1e-6
RESULT_KEYS = ("transform", "R", "T", "ell", "iter", "A_nonzero", "iterations_run", "status")
MIXED = 14                                                               # the "mixed" perturbation's place in hypothesis_set


def small_tf():
    return make_tf([0.2, 1, 0.1], 0.01, [0.004, -0.002, 0.003])


def far_tf(k=0):
    """a pose that moves the cloud 10 m (and k metres more) away: nothing is inside the radius gate"""
    t = np.eye(3, 4, dtype=np.float32); t[0, 3] = 10.0 + k
    return t


@pytest.fixture(scope="module")
def pairs():
    from cvo_slam_amd import synth
    return {c: synth.make_small_pair(*c) for c in hr.CASES}


@pytest.fixture(scope="module")
def sets(pairs):
    """the 15-transform hypothesis set of every case"""
    return {c: hr.hypothesis_set(p.true_transform) for c, p in pairs.items()}


def handle_for(hiplib, fixed, moving, ell=None):
    """a handle with (fixed, moving) in its slots; each a (xyz, feat) tuple"""
    g = hiplib.Cvo(); g.set_pcd(*fixed); g.set_pcd(*moving)
    if ell is not None:
        g.set_state(np.eye(3), np.zeros(3), ell)
    return g


def clouds_of(p):
    return (p.fixed.xyz, p.fixed.feat), (p.moving.xyz, p.moving.feat)


def check_against_reading(got, moving, fixed, trans, ell, where):
    """num equal, value to rtol 1e-6, grad and hess to 1e-6 of their magnitudes; returns the reading"""
    want = pm.models(moving, fixed, trans, ell)
    values, nums, grads, hess = got
    assert values.dtype == np.float32 and nums.dtype == np.int32 and grads.dtype == hess.dtype == np.float64
    assert grads.shape == values.shape + (6,) and hess.shape == values.shape + (6, 6)
    with np.errstate(divide="ignore", invalid="ignore"):
        ug = np.nan_to_num(np.abs(grads - want[2]) / want[4]); uh = np.nan_to_num(np.abs(hess - want[3]) / want[5])
    rel = np.abs(values.astype(np.float64) - want[0]) / np.maximum(want[0].astype(np.float64), 1e-300)
    print(where, "nums", want[1].tolist(), "value max rel", float(rel.max()), "grad, hess max in units of the magnitude", float(ug.max()), float(uh.max()))
    np.testing.assert_array_equal(nums, want[1], err_msg=str(where))
    np.testing.assert_allclose(values.astype(np.float64), want[0].astype(np.float64), rtol=RTOL, atol=0, err_msg=str(where))
    assert (np.abs(grads - want[2]) <= MAG_TOL * want[4]).all(), (where, "grad", float(ug.max()))
    assert (np.abs(hess - want[3]) <= MAG_TOL * want[5]).all(), (where, "hess", float(uh.max()))
    assert np.array_equal(hess, np.swapaxes(hess, -1, -2)), (where, "hess is not symmetric bit for bit")
    return want


def same_bytes(x, y, where=""):
    assert len(x) == len(y) == 4
    for k, (u, v) in enumerate(zip(x, y)):
        u, v = np.asarray(u), np.asarray(v)
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), (where, k, u, v)


def at(m, *idx):
    return tuple(a[idx] for a in m)


def same_results(ra, rb, where=""):
    assert len(ra) == len(rb)
    for i, (a, b) in enumerate(zip(ra, rb)):
        for key in RESULT_KEYS:
            assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (where, i, key, a[key], b[key])


def batch_of(hiplib, pairs, cases, slots=None):
    b = hiplib.CvoBatch(slots or len(cases))
    for i, c in enumerate(cases):
        p = pairs[c]
        b.set_pair(i, p.fixed.xyz, p.fixed.feat, p.moving.xyz, p.moving.feat)
    return b


# ---- 1. the handle form against the reading and against score_hypotheses
@pytest.mark.parametrize("ell", hr.ELLS)
@pytest.mark.parametrize("case", hr.CASES)
def test_handle_form_against_the_reading_and_the_scores(hiplib, pairs, sets, case, ell):
    p = pairs[case]; trans = sets[case]
    fixed, moving = clouds_of(p)
    g = handle_for(hiplib, fixed, moving)
    before = g.get_state()
    got = g.pose_models(MOVING, FIXED, trans, ell)
    assert got[0].shape == (15,)
    want = check_against_reading(got, moving, fixed, trans, ell, (case, ell))
    assert want[1][hr.TRUTH] > 1
    values, nums, _ = g.score_hypotheses(MOVING, FIXED, trans, ell)
    assert got[0].tobytes() == values.tobytes() and got[1].tobytes() == nums.tobytes()
    after = g.get_state()                                               # the handle's R, T, ell are untouched
    assert all(np.asarray(before[k]).tobytes() == np.asarray(after[k]).tobytes() for k in before)
    g.close()


# ---- 2. bits do not depend on the company
def test_bits_do_not_depend_on_k_or_the_position(hiplib, pairs, sets):
    case, ell = (31, 700), 0.06
    trans = sets[case]
    g = handle_for(hiplib, *clouds_of(pairs[case]))
    all15 = g.pose_models(MOVING, FIXED, trans, ell)
    same_bytes(g.pose_models(MOVING, FIXED, trans, ell), all15, "twice")
    for k in range(15):
        same_bytes(g.pose_models(MOVING, FIXED, trans[k:k + 1], ell), at(all15, slice(k, k + 1)), ("K = 1", k))
    many = np.concatenate([trans[(2 + np.arange(63)) % 15], trans[MIXED:MIXED + 1]])
    last_of_64 = g.pose_models(MOVING, FIXED, many, ell)
    assert last_of_64[0].shape == (64,)
    same_bytes(at(last_of_64, slice(63, 64)), at(all15, slice(MIXED, MIXED + 1)), "last of 64")
    g.close()


def test_bits_do_not_depend_on_the_other_pairs_and_equal_the_handle_form(hiplib, pairs, sets):
    ell = 0.06
    order = [(5, 200), (77, 800), (31, 700)]                            # three pairs of different sizes
    trans = np.stack([sets[c][:9] for c in order])                      # K = 9 each
    b = batch_of(hiplib, pairs, order, 4)
    together = b.pose_models(trans, ell=ell)
    assert together[0].shape == together[1].shape == (3, 9) and together[2].shape == (3, 9, 6) and together[3].shape == (3, 9, 6, 6)
    same_bytes(b.pose_models(trans, ell=ell), together, "twice")
    for i, c in enumerate(order):
        alone = b.pose_models(trans[i:i + 1], pairs=[i], ell=ell)
        same_bytes(at(alone, 0), at(together, i), ("alone", c))
        g = handle_for(hiplib, *clouds_of(pairs[c]))
        same_bytes(g.pose_models(MOVING, FIXED, trans[i], ell), at(together, i), ("handle", c))
        g.close()
    swapped = b.pose_models(trans[[2, 0]], pairs=[2, 0], ell=ell)       # a list in another order, a subset: results follow the list
    same_bytes(at(swapped, 0), at(together, 2), "listed first")
    same_bytes(at(swapped, 1), at(together, 0), "listed second")
    b.close()


def test_a_short_and_a_long_pair_in_one_launch(hiplib, pairs, sets):
    """200 and 800 points, K = 9: the row blocks past the short pair's rows write zero records"""
    ell = 0.06
    cases = [(5, 200), (77, 800)]
    trans = np.stack([sets[c][:9] for c in cases])
    handle = []
    for c, t in zip(cases, trans):
        g = handle_for(hiplib, *clouds_of(pairs[c]))
        handle.append(g.pose_models(MOVING, FIXED, t, ell))
        g.close()
    for order in ([0, 1], [1, 0]):
        b = batch_of(hiplib, pairs, [cases[i] for i in order])
        got = b.pose_models(trans[order], ell=ell)
        for slot, i in enumerate(order):
            same_bytes(at(got, slot), handle[i], (order, slot))
            assert got[1][slot][hr.TRUTH] > 1
        b.close()


# ---- 3. the smallest shapes at which the kernel can go wrong
@pytest.mark.parametrize("rows", [1, 63, 64, 65])
def test_row_counts_around_a_wave(hiplib, pairs, rows):
    """rows of one wave, one short of it, one past it -- against 129 columns (four groups and one point)"""
    p = pairs[(31, 700)]
    bx, bf = np.ascontiguousarray(p.fixed.xyz[:129]), np.ascontiguousarray(p.fixed.feat[:, :129])
    ax = np.ascontiguousarray(p.fixed.xyz[:rows] + np.float32(0.003)); af = np.ascontiguousarray(p.moving.feat[:, :rows])
    trans = np.stack([np.eye(3, 4, dtype=np.float32), small_tf(), far_tf()])
    g = handle_for(hiplib, (bx, bf), (ax, af))
    got = g.pose_models(MOVING, FIXED, trans, 0.15)
    want = check_against_reading(got, (ax, af), (bx, bf), trans, 0.15, ("rows", rows))
    assert want[1][0] >= rows and want[1][1] >= rows
    g.close()


def test_past_one_ballot_round(hiplib):
    """2 100 columns are 66 groups: a wave tests 64 group boxes per ballot, so groups 64 and 65 are reached only in the sweep's second round.
    70 rows (a wave and six rows) sit on columns 2030 .. 2099."""
    from cvo_slam_amd import synth
    p = synth.make_small_pair(31, 2100)
    bx, bf = np.ascontiguousarray(p.fixed.xyz), np.ascontiguousarray(p.fixed.feat)
    ax = np.ascontiguousarray(p.fixed.xyz[2030:2100] + np.float32(0.003)); af = np.ascontiguousarray(p.moving.feat[:, 2030:2100])
    assert bx.shape[0] == 2100 and ax.shape[0] == 70
    trans = np.stack([np.eye(3, 4, dtype=np.float32), small_tf()])
    for t in trans:                                                     # the precondition, on the reading: columns of both late groups are hit
        count_b = support_reading.point_support(ax, af, bx, bf, 0.15, t)[3]
        assert count_b[2048:2080].any() and count_b[2080:2100].any()
    g = handle_for(hiplib, (bx, bf), (ax, af))
    got = g.pose_models(MOVING, FIXED, trans, 0.15)
    want = check_against_reading(got, (ax, af), (bx, bf), trans, 0.15, "second round")
    assert want[1].min() >= 70
    g.close()


@pytest.mark.parametrize("case", ["shuffled", "behind_camera"])
def test_box_cull_edge_cases(hiplib, pairs, sets, case):
    """These clouds exercise ordering and padding but not skipping (in random order every group's box spans the scene);
    tests/test_gpu_sweep_cases.py runs the clouds on which groups are skipped."""
    rng = np.random.default_rng(5)
    p = pairs[(31, 700)]
    fx, ff, mx, mf = p.fixed.xyz.copy(), p.fixed.feat.copy(), p.moving.xyz.copy(), p.moving.feat.copy()
    trans = sets[(31, 700)][:9]
    if case == "shuffled":
        a, b = rng.permutation(fx.shape[0]), rng.permutation(mx.shape[0])
        fx, ff, mx, mf = fx[a], ff[:, a], mx[b], mf[:, b]
    else:
        fx[:, 2] -= 1.2; mx[:, 2] -= 1.2                                # clouds partly behind the camera: no slope bound for those points
        assert (fx[:, 2] < 0).any() and (fx[:, 2] > 0).any()
        trans = np.stack([np.eye(3, 4, dtype=np.float32), small_tf(), far_tf()])
    fx, ff, mx, mf = (np.ascontiguousarray(v) for v in (fx, ff, mx, mf))
    g = handle_for(hiplib, (fx, ff), (mx, mf))
    for ell in (0.03, 0.15):
        got = g.pose_models(MOVING, FIXED, trans, ell)
        want = check_against_reading(got, (mx, mf), (fx, ff), trans, ell, (case, ell))
        assert want[1].max() > 1
    g.close()


def test_a_pose_ten_metres_away_gives_nothing(hiplib, pairs):
    p = pairs[(5, 200)]
    g = handle_for(hiplib, *clouds_of(p))
    values, nums, grads, hess = g.pose_models(MOVING, FIXED, np.stack([far_tf(), p.true_transform.astype(np.float32), far_tf(3)]), 0.15)
    for k in (0, 2):
        assert values[k] == 0 and nums[k] == 1                          # cvo.cpp:455-456
        assert grads[k].tobytes() == np.zeros(6).tobytes() and hess[k].tobytes() == np.zeros((6, 6)).tobytes()
    assert values[1] > 0 and nums[1] > 1 and grads[1].any() and hess[1].any()
    g.close()


# ---- 4. the models of an align launch's results
SIZES = [200, 300, 400, 500, 600, 700, 800, 650]


@pytest.fixture(scope="module")
def eight():
    from cvo_slam_amd import synth
    return [synth.make_small_pair(100 + i, n) for i, n in enumerate(SIZES)]


def batch_of_eight(hiplib, eight):
    b = hiplib.CvoBatch(8)
    for i, p in enumerate(eight):
        b.set_pair(i, p.fixed.xyz, p.fixed.feat, p.moving.xyz, p.moving.feat)
    return b


def test_result_models_equal_the_handle_form_and_leave_the_results_alone(hiplib, eight):
    plain = batch_of_eight(hiplib, eight)
    res_plain = plain.align(8); res_plain_warm = plain.align(8)
    b = batch_of_eight(hiplib, eight)
    b.align_async(8)
    got = b.result_models()                                             # queued behind the launch, before anyone has waited for it
    res = b.wait(8)
    assert all(r["status"] == 0 for r in res)
    same_results(res, res_plain, "result_models behind the launch")
    assert got[0].shape == got[1].shape == (8,) and got[2].shape == (8, 6) and got[3].shape == (8, 6, 6)
    support = b.point_support()
    for i, (p, r) in enumerate(zip(eight, res)):
        g = handle_for(hiplib, *clouds_of(p))
        same_bytes(g.pose_models(MOVING, FIXED, np.asarray(r["transform"], np.float32).reshape(1, 3, 4), float(r["ell"])), at(got, slice(i, i + 1)), i)
        g.close()
        assert got[1][i] == int(support[i]["count_moving"].sum()) > 1
        assert np.array_equal(got[3][i], got[3][i].T)
    same_bytes(b.result_models(), got, "again")
    sub = [5, 2, 7, 0]                                                  # a permuted subset, and one pair alone
    part = b.result_models(sub)
    for k, i in enumerate(sub):
        same_bytes(at(part, k), at(got, i), ("subset", i))
    same_bytes(b.result_models([3]), at(got, slice(3, 4)), "alone")
    same_results(b.align(8), res_plain_warm, "a warm launch after result_models")
    plain.close(); b.close()


def test_pose_models_before_an_align_launch_leave_it_alone(hiplib, pairs, sets):
    cases = list(hr.CASES)
    plain = batch_of(hiplib, pairs, cases)
    res_plain = plain.align(3); res_plain_warm = plain.align(3)
    b = batch_of(hiplib, pairs, cases)
    trans = np.stack([sets[c][:9] for c in cases])
    b.pose_models(trans, ell=0.06)
    same_results(b.align(3), res_plain, "pose_models before the first launch")
    b.pose_models(trans, ell=0.15)                                      # and with the device states carried: a warm second launch either way
    same_results(b.align(3), res_plain_warm, "pose_models before a warm launch")
    plain.close(); b.close()


# ---- 5. what a model is for
@pytest.mark.parametrize("ell", hr.ELLS)
@pytest.mark.parametrize("case", hr.CASES)
def test_a_newton_step_raises_the_inner_product(hiplib, pairs, sets, case, ell):
    from cvo_slam_amd import pose_model
    T = sets[case][MIXED]
    g = handle_for(hiplib, *clouds_of(pairs[case]), ell)                # the handle's ell = the model's, for function_inner_product below
    values, nums, grads, hess = g.pose_models(MOVING, FIXED, T[None], ell)
    assert np.linalg.eigvalsh(hess[0]).max() < 0                        # negative definite
    T1 = pose_model.retract(pose_model.newton_step(grads[0], hess[0]), T)
    v0 = g.function_inner_product(MOVING, T, FIXED)[0]; v1 = g.function_inner_product(MOVING, T1.astype(np.float32), FIXED)[0]
    print(case, ell, "value", v0, "->", v1, "x", v1 / v0)
    assert v0 == pytest.approx(float(values[0]), rel=1e-6)
    assert v1 > v0
    g.close()


# ---- 6. argument errors, one by one, change nothing
BAD_CALLS = [
    ("null_trans", dict(trans=None), ERR_INVALID),
    ("k_0", dict(k=0), ERR_INVALID),
    ("k_65", dict(k=65, trans=np.tile(np.eye(3, 4, dtype=np.float32), (2 * 65, 1, 1))), ERR_INVALID),
    ("ell_0", dict(ell=0.0), ERR_INVALID),
    ("ell_negative", dict(ell=-0.06), ERR_INVALID),
    ("ell_nan", dict(ell=float("nan")), ERR_INVALID),
    ("ell_inf", dict(ell=float("inf")), ERR_INVALID),
    ("trans_nan", dict(poison=float("nan")), ERR_INVALID),
    ("trans_inf", dict(poison=float("inf")), ERR_INVALID),
    ("count_0", dict(count=0), ERR_INVALID),
    ("count_5", dict(count=5), ERR_INVALID),
    ("slot_out_of_range", dict(pairs=[0, 4]), ERR_INVALID),
    ("slot_negative", dict(pairs=[-1, 0]), ERR_INVALID),
    ("slot_twice", dict(pairs=[1, 1]), ERR_INVALID),
    ("stream_slot", dict(pairs=[0, 2]), ERR_INVALID),
    ("empty_cloud", dict(pairs=[0, 3]), ERR_EMPTY),
    ("null_out", dict(out=None), ERR_INVALID),
]


def filled_models(hiplib, n):
    recs = (hiplib.api.PoseModel * n)()
    C.memset(recs, 0x5a, C.sizeof(recs))
    return recs, bytes(recs)


def test_batch_argument_errors_change_nothing(hiplib, pairs, sets):
    import torch
    cases = [(31, 700), (5, 200), (77, 800)]
    ell = 0.06
    plain = batch_of(hiplib, pairs, cases[:2])
    undisturbed = plain.align(2)
    plain.close()
    b = batch_of(hiplib, pairs, cases[:2], 4)
    p = pairs[cases[2]]                                                 # slot 2: a stream slot; slot 3: never filled
    b.advance_clouds([2], [(torch.from_numpy(p.fixed.xyz).cuda(), torch.from_numpy(p.fixed.feat).cuda(), "channels_first")])
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    recs, fill = filled_models(hiplib, 5 * 65)
    for name, change, code in BAD_CALLS:
        args = dict(count=2, pairs=[0, 1], k=9, trans=np.stack([sets[c][:9] for c in cases[:2]]).copy(), ell=ell, out=recs)
        args.update({k: v for k, v in change.items() if k != "poison"})
        if change.get("poison") is not None:
            args["trans"][1, 8, 2, 3] = change["poison"]                # the last entry but a few of the call's transforms
        pr = np.ascontiguousarray(args["pairs"], np.int32)
        t = None if args["trans"] is None else np.ascontiguousarray(args["trans"], np.float32)
        rc = b.L.cvo_batch_pose_models(b.h, args["count"], pr.ctypes.data_as(ip), args["k"], None if t is None else t.ctypes.data_as(fp),
                                       C.c_float(args["ell"]), args["out"])
        assert rc == code, (name, rc, hiplib.api.load_library().cvo_last_error())
        assert bytes(recs) == fill, name
    assert b.L.cvo_batch_pose_models(None, 2, None, 9, t.ctypes.data_as(fp), C.c_float(ell), recs) == ERR_INVALID
    assert bytes(recs) == fill
    same_results(b.align(2), undisturbed, "after the refused calls")    # the start states are those of an undisturbed batch
    # result_models: the rules of point_support
    idx = lambda *v: (C.c_int * len(v))(*v)
    L = b.L
    assert L.cvo_batch_result_models(b.h, 1, idx(0), None) == ERR_INVALID                      # NULL out
    assert L.cvo_batch_result_models(None, 1, idx(0), recs) == ERR_INVALID
    assert L.cvo_batch_result_models(b.h, 1, idx(2), recs) == ERR_INVALID                      # position out of range: the launch had two
    assert L.cvo_batch_result_models(b.h, 1, idx(-1), recs) == ERR_INVALID
    assert L.cvo_batch_result_models(b.h, 0, idx(0), recs) == ERR_INVALID
    assert L.cvo_batch_result_models(b.h, 3, None, recs) == ERR_INVALID                        # more pairs than the launch aligned
    assert L.cvo_batch_result_models(b.h, 2, idx(1, 1), recs) == ERR_INVALID                   # listed twice
    assert bytes(recs) == fill
    fresh = hiplib.CvoBatch(2)
    with pytest.raises(hiplib.CvoError) as e:                                                  # nothing was aligned yet
        fresh.result_models([0])
    assert e.value.code == ERR_INVALID
    fresh.close()
    assert L.cvo_batch_result_models(b.h, 2, None, recs) == 0                                  # pairs NULL: 0 .. count-1; and then it computes
    assert recs[0].num > 1 and recs[1].num > 1 and bytes(recs)[2 * 344:] == fill[2 * 344:]
    same_results(b.align(2), batch_second_launch(hiplib, pairs, cases[:2]), "a warm launch after the refused calls")
    b.close()


def batch_second_launch(hiplib, pairs, cases):
    plain = batch_of(hiplib, pairs, cases)
    plain.align(len(cases))
    res = plain.align(len(cases))
    plain.close()
    return res


def test_handle_form_errors(hiplib, pairs, sets):
    case, ell = (31, 700), 0.06
    g = handle_for(hiplib, *clouds_of(pairs[case]))
    fp = C.POINTER(C.c_float)
    t = np.ascontiguousarray(sets[case][:9], np.float32)
    recs, fill = filled_models(hiplib, 65)
    L = g.L
    assert L.cvo_pose_models(g.h, MOVING, FIXED, 9, None, C.c_float(ell), recs) == ERR_INVALID
    assert L.cvo_pose_models(g.h, MOVING, FIXED, 9, t.ctypes.data_as(fp), C.c_float(ell), None) == ERR_INVALID
    assert L.cvo_pose_models(None, MOVING, FIXED, 9, t.ctypes.data_as(fp), C.c_float(ell), recs) == ERR_INVALID
    assert L.cvo_pose_models(g.h, MOVING, FIXED, 0, t.ctypes.data_as(fp), C.c_float(ell), recs) == ERR_INVALID
    big = np.tile(np.eye(3, 4, dtype=np.float32), (65, 1, 1))
    assert L.cvo_pose_models(g.h, MOVING, FIXED, 65, big.ctypes.data_as(fp), C.c_float(ell), recs) == ERR_INVALID
    for bad_ell in (0.0, -0.06, float("nan"), float("inf")):
        assert L.cvo_pose_models(g.h, MOVING, FIXED, 9, t.ctypes.data_as(fp), C.c_float(bad_ell), recs) == ERR_INVALID
    bad = t.copy(); bad[4, 1, 1] = np.inf
    assert L.cvo_pose_models(g.h, MOVING, FIXED, 9, bad.ctypes.data_as(fp), C.c_float(ell), recs) == ERR_INVALID
    assert L.cvo_pose_models(g.h, MOVING, 2, 9, t.ctypes.data_as(fp), C.c_float(ell), recs) == ERR_EMPTY   # no PREVIOUS cloud
    assert bytes(recs) == fill
    assert L.cvo_pose_models(g.h, MOVING, FIXED, 9, t.ctypes.data_as(fp), C.c_float(ell), recs) == 0
    assert recs[hr.TRUTH].num > 1 and bytes(recs)[9 * 344:] == fill[9 * 344:]
    g.close()
