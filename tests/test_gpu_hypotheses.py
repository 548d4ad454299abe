"""Pose hypotheses (cvo_score_hypotheses, cvo_batch_score_hypotheses, cvo_batch_seed_hypotheses_async, cvo_batch_hypothesis_results): K start
transforms per pair scored in one launch, the best one written as the pair's start state on the device.  The yardstick is
tests/hypothesis_reading.py, a dense numpy reading that tests/test_hypothesis_reading.py holds against the C++ oracle: nums must be EQUAL to
it, values agree to rtol 1e-6 (atol 0: positive terms, float64 sums -- the bound of tests/test_gpu_point_support.py), best equal (the reading's
best wins by a relative gap of 5e-3 at least, four orders above that tolerance).  Every other form must give the handle form's bytes, and a seeded
alignment the bytes of the same alignment started through cvo_batch_set_state."""
import ctypes as C

import numpy as np
import pytest

import hypothesis_reading as hr
import support_reading
from helpers import make_tf

pytestmark = pytest.mark.gpu

FIXED, MOVING = 0, 1
ERR_EMPTY, ERR_INVALID = 2, 4
RTOL = 1e-6
RESULT_KEYS = ("transform", "R", "T", "ell", "iter", "A_nonzero", "iterations_run", "status")


def small_tf():
    return make_tf([0.2, 1, 0.1], 0.01, [0.004, -0.002, 0.003])


def far_tf(k=0):
    """a hypothesis that moves the cloud 10 m (and k metres more) away: nothing is inside the radius gate"""
    t = np.eye(3, 4, dtype=np.float32); t[0, 3] = 10.0 + k
    return t


@pytest.fixture(scope="module")
def pairs():
    from cvo_slam_amd import synth
    return {c: synth.make_small_pair(*c) for c in hr.CASES}


@pytest.fixture(scope="module")
def readings(pairs):
    """the reading of the full hypothesis set, once per (case, ell): (trans, values, nums, best)"""
    out = {}
    for case, p in pairs.items():
        trans = hr.hypothesis_set(p.true_transform)
        for ell in hr.ELLS:
            out[(case, ell)] = (trans,) + hr.scores((p.moving.xyz, p.moving.feat), (p.fixed.xyz, p.fixed.feat), trans, ell)
    return out


def handle_for(hiplib, fixed, moving, ell=None):
    """a handle with (fixed, moving) in its slots; each a (xyz, feat) tuple"""
    g = hiplib.Cvo(); g.set_pcd(*fixed); g.set_pcd(*moving)
    if ell is not None:
        g.set_state(np.eye(3), np.zeros(3), ell)
    return g


def clouds_of(p):
    return (p.fixed.xyz, p.fixed.feat), (p.moving.xyz, p.moving.feat)


def check_against_reading(got, moving, fixed, trans, ell, where):
    want = hr.scores(moving, fixed, trans, ell)
    rel = np.abs(got[0].astype(np.float64) - want[0]) / np.maximum(want[0].astype(np.float64), 1e-300)
    print(where, "nums", want[1].tolist(), "max rel", float(rel.max()), "best", want[2], "gap", hr.relative_gap(want[0]) if len(want[0]) > 1 else None)
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32
    np.testing.assert_array_equal(got[1], want[1], err_msg=str(where))
    np.testing.assert_allclose(got[0].astype(np.float64), want[0].astype(np.float64), rtol=RTOL, atol=0, err_msg=str(where))
    return want


def same_bytes(x, y, where=""):
    for k, (u, v) in enumerate(zip(x[:2], y[:2])):
        u, v = np.asarray(u), np.asarray(v)
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), (where, k, u, v)
    if len(x) > 2 and len(y) > 2:
        assert np.array_equal(np.asarray(x[2]), np.asarray(y[2])), (where, "best")


def same_results(ra, rb, where=""):
    assert len(ra) == len(rb)
    for i, (a, b) in enumerate(zip(ra, rb)):
        for key in RESULT_KEYS:
            assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (where, i, key, a[key], b[key])


# ---- 1. the handle form against the reading and against cvo_function_inner_product
@pytest.mark.parametrize("ell", hr.ELLS)
@pytest.mark.parametrize("case", hr.CASES)
def test_handle_form_against_the_reading_and_function_inner_product(hiplib, pairs, readings, case, ell):
    p = pairs[case]
    trans, values, nums, best = readings[(case, ell)]
    fixed, moving = clouds_of(p)
    g = handle_for(hiplib, fixed, moving, ell)                          # the handle's ell = the scoring ell, for function_inner_product below
    before = g.get_state()
    got = g.score_hypotheses(MOVING, FIXED, trans, ell)
    rel = np.abs(got[0].astype(np.float64) - values) / np.maximum(values.astype(np.float64), 1e-300)
    print(case, ell, "max rel", float(rel.max()), "best", got[2], "gap", hr.relative_gap(values))
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[0].shape == got[1].shape == (15,)
    np.testing.assert_array_equal(got[1], nums)
    np.testing.assert_allclose(got[0].astype(np.float64), values.astype(np.float64), rtol=RTOL, atol=0)
    assert got[2] == best == hr.TRUTH
    for k in range(trans.shape[0]):
        value, num, _ = g.function_inner_product(MOVING, trans[k], FIXED)
        assert int(got[1][k]) == num, k
        assert float(got[0][k]) == pytest.approx(value, rel=1e-6), k
    after = g.get_state()                                               # the handle's R, T, ell are untouched
    assert all(np.asarray(before[k]).tobytes() == np.asarray(after[k]).tobytes() for k in before)
    g.close()


# ---- 2. bits do not depend on the company
def test_bits_do_not_depend_on_k_or_the_position(hiplib, pairs, readings):
    case, ell = (31, 700), 0.06
    p = pairs[case]; trans = readings[(case, ell)][0]
    g = handle_for(hiplib, *clouds_of(p))
    for k in (hr.TRUTH, 3, 14):
        alone = g.score_hypotheses(MOVING, FIXED, trans[k:k + 1], ell)
        assert alone[1][0] > 1 and alone[2] == 0
        nine = np.concatenate([trans[(k + 1 + np.arange(8)) % 15], trans[k:k + 1]])
        last_of_9 = g.score_hypotheses(MOVING, FIXED, nine, ell)
        many = np.concatenate([trans[(k + 2 + np.arange(63)) % 15], trans[k:k + 1]])
        last_of_64 = g.score_hypotheses(MOVING, FIXED, many, ell)
        assert last_of_64[0].shape == (64,)
        for got in (last_of_9, last_of_64):
            same_bytes((got[0][-1:], got[1][-1:]), alone, k)
        again = g.score_hypotheses(MOVING, FIXED, many, ell)             # the same call twice
        same_bytes(again, last_of_64, "twice")
    g.close()


def test_bits_do_not_depend_on_the_other_pairs_and_equal_the_handle_form(hiplib, pairs, readings):
    ell = 0.06
    order = [(5, 200), (77, 800), (31, 700)]                            # three pairs of different sizes; (31, 700) is pair 2 of 3
    trans = np.stack([readings[(c, ell)][0][:9] for c in order])        # K = 9 each
    b = hiplib.CvoBatch(4)
    for i, c in enumerate(order):
        p = pairs[c]
        b.set_pair(i, p.fixed.xyz, p.fixed.feat, p.moving.xyz, p.moving.feat)
    together = b.score_hypotheses(trans, ell=ell)
    assert together[0].shape == together[1].shape == (3, 9) and together[2].shape == (3,)
    same_bytes(b.score_hypotheses(trans, ell=ell), together, "twice")
    for i, c in enumerate(order):
        alone = b.score_hypotheses(trans[i:i + 1], pairs=[i], ell=ell)
        same_bytes((alone[0][0], alone[1][0], alone[2][0]), (together[0][i], together[1][i], together[2][i]), ("alone", c))
        g = handle_for(hiplib, *clouds_of(pairs[c]))
        h = g.score_hypotheses(MOVING, FIXED, trans[i], ell)
        same_bytes(h, (together[0][i], together[1][i], together[2][i]), ("handle", c))
        np.testing.assert_array_equal(together[1][i], readings[(c, ell)][2][:9])
        assert together[2][i] == hr.TRUTH
        g.close()
    # a list in another order, a subset: results follow the list
    swapped = b.score_hypotheses(trans[[2, 0]], pairs=[2, 0], ell=ell)
    same_bytes((swapped[0][0], swapped[1][0]), (together[0][2], together[1][2]), "listed first")
    same_bytes((swapped[0][1], swapped[1][1]), (together[0][0], together[1][0]), "listed second")


# ---- 3. edges where the kernel can go wrong
@pytest.mark.parametrize("rows", [1, 63, 64, 65])
def test_row_counts_around_a_wave(hiplib, pairs, rows):
    """rows of one wave, one short of it, one past it -- against 129 columns (four groups and one point)"""
    p = pairs[(31, 700)]
    bx, bf = np.ascontiguousarray(p.fixed.xyz[:129]), np.ascontiguousarray(p.fixed.feat[:, :129])
    ax = np.ascontiguousarray(p.fixed.xyz[:rows] + np.float32(0.003)); af = np.ascontiguousarray(p.moving.feat[:, :rows])
    trans = np.stack([np.eye(3, 4, dtype=np.float32), small_tf(), far_tf()])
    g = handle_for(hiplib, (bx, bf), (ax, af))
    got = g.score_hypotheses(MOVING, FIXED, trans, 0.15)
    want = check_against_reading(got, (ax, af), (bx, bf), trans, 0.15, ("rows", rows))
    assert want[1][0] >= rows and want[1][1] >= rows and got[2] == want[2]
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
    got = g.score_hypotheses(MOVING, FIXED, trans, 0.15)
    want = check_against_reading(got, (ax, af), (bx, bf), trans, 0.15, "second round")
    assert want[1].min() >= 70 and got[2] == want[2]
    g.close()


@pytest.mark.parametrize("case", ["shuffled", "behind_camera"])
def test_box_cull_edge_cases(hiplib, pairs, case):
    """These clouds exercise ordering and padding but not skipping (in random order every group's box spans the scene);
    tests/test_gpu_sweep_cases.py runs the clouds on which groups are skipped."""
    rng = np.random.default_rng(5)
    p = pairs[(31, 700)]
    fx, ff, mx, mf = p.fixed.xyz.copy(), p.fixed.feat.copy(), p.moving.xyz.copy(), p.moving.feat.copy()
    trans = hr.hypothesis_set(p.true_transform)[:9]
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
        got = g.score_hypotheses(MOVING, FIXED, trans, ell)
        want = check_against_reading(got, (mx, mf), (fx, ff), trans, ell, (case, ell))
        assert want[1].max() > 1
        if hr.relative_gap(want[0]) >= 1e-4:
            assert got[2] == want[2]
    g.close()


def test_a_hypothesis_ten_metres_away_scores_nothing(hiplib, pairs):
    p = pairs[(5, 200)]
    g = handle_for(hiplib, *clouds_of(p))
    values, nums, best = g.score_hypotheses(MOVING, FIXED, np.stack([far_tf(), p.true_transform.astype(np.float32)]), 0.15)
    assert values[0] == 0 and nums[0] == 1                              # cvo.cpp:455-456
    assert values[1] > 0 and nums[1] > 1 and best == 1
    g.close()


def test_a_short_and_a_long_pair_in_one_launch(hiplib, pairs, readings):
    """200 and 800 points, K = 9: the row blocks past the short pair's rows write zero records"""
    ell = 0.06
    cases = [(5, 200), (77, 800)]
    trans = np.stack([readings[(c, ell)][0][:9] for c in cases])
    for order in ([0, 1], [1, 0]):
        b = hiplib.CvoBatch(2)
        for slot, i in enumerate(order):
            p = pairs[cases[i]]
            b.set_pair(slot, p.fixed.xyz, p.fixed.feat, p.moving.xyz, p.moving.feat)
        got = b.score_hypotheses(trans[order], ell=ell)
        for slot, i in enumerate(order):
            _, values, nums, best = readings[(cases[i], ell)]
            np.testing.assert_array_equal(got[1][slot], nums[:9])
            np.testing.assert_allclose(got[0][slot].astype(np.float64), values[:9].astype(np.float64), rtol=RTOL, atol=0)
            assert got[2][slot] == hr.TRUTH
            g = handle_for(hiplib, *clouds_of(pairs[cases[i]]))
            same_bytes(g.score_hypotheses(MOVING, FIXED, trans[i], ell), (got[0][slot], got[1][slot], got[2][slot]), (order, slot))
            g.close()


# ---- 4. ties
def test_ties_go_to_the_lowest_index(hiplib, pairs, readings):
    case, ell = (31, 700), 0.06
    p = pairs[case]; trans = readings[(case, ell)][0]
    g = handle_for(hiplib, *clouds_of(p))
    six = np.stack([trans[0], trans[3], trans[hr.TRUTH], trans[7], trans[9], trans[hr.TRUTH]])   # the truth at 2 and 5, the others worse
    values, nums, best = g.score_hypotheses(MOVING, FIXED, six, ell)
    assert values[2].tobytes() == values[5].tobytes() and nums[2] == nums[5]
    assert values[2] > np.delete(values, [2, 5]).max()
    assert best == 2
    values, nums, best = g.score_hypotheses(MOVING, FIXED, np.stack([far_tf(k) for k in range(5)]), ell)   # nothing scores anywhere
    assert not values.any() and (nums == 1).all() and best == 0
    g.close()


# ---- 5. seeding
@pytest.fixture(scope="module")
def seed_setup(pairs, readings):
    """three pairs, K = 9, ell 0.06, the truth at a different index per pair"""
    ell = 0.06
    cases = [(31, 700), (5, 200), (77, 800)]
    truth_at = [4, 0, 8]
    trans = []
    for c, at in zip(cases, truth_at):
        t = readings[(c, ell)][0]
        others = [k for k in range(9) if k != hr.TRUTH]                 # identity, six rotated truths, one shifted truth: all worse than the truth
        row = [t[k] for k in others]; row.insert(at, t[hr.TRUTH])
        trans.append(np.stack(row))
    return ell, cases, truth_at, np.stack(trans)


def batch_of(hiplib, pairs, cases):
    b = hiplib.CvoBatch(len(cases))
    for i, c in enumerate(cases):
        p = pairs[c]
        b.set_pair(i, p.fixed.xyz, p.fixed.feat, p.moving.xyz, p.moving.feat)
    return b


def start_from_host(hiplib, b, trans, best):
    """route B: cvo_reset_initial on a fresh handle, its R and T handed to cvo_batch_set_state with the batch's start ell"""
    for i in range(trans.shape[0]):
        g = hiplib.Cvo(); g.reset_initial(trans[i, best[i]]); s = g.get_state(); g.close()
        b.set_state(i, s["R"], s["T"], b.params.ell)


def pose_error(tf, truth):
    D = np.asarray(tf, np.float64)[:, :3].T @ np.asarray(truth, np.float64)[:, :3]
    w = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.arctan2(np.linalg.norm(w), (np.trace(D) - 1) / 2)), float(np.linalg.norm(np.asarray(tf, np.float64)[:, 3] - np.asarray(truth, np.float64)[:, 3]))


def test_seeded_alignment_equals_set_state_alignment(hiplib, pairs, seed_setup):
    ell, cases, truth_at, trans = seed_setup
    a = batch_of(hiplib, pairs, cases)
    a.seed_hypotheses(trans, ell=ell)
    a.align_async(3)
    res_a = a.wait(3)
    seeded = a.hypothesis_results(3)
    b = batch_of(hiplib, pairs, cases)
    scored = b.score_hypotheses(trans, ell=ell)
    same_bytes(seeded, scored, "seed results against score_hypotheses")
    assert scored[2].tolist() == truth_at
    start_from_host(hiplib, b, trans, scored[2])
    b.align_async(3)
    res_b = b.wait(3)
    assert all(r["status"] == 0 for r in res_a)
    same_results(res_a, res_b, "seeded against set_state")
    for i, c in enumerate(cases):
        ang, dt = pose_error(res_a[i]["transform"], pairs[c].true_transform)
        print(c, "iterations", res_a[i]["iterations_run"], "rotation error", ang, "rad, translation error", dt, "m")
    for i, c in enumerate(cases):
        ang, dt = pose_error(res_a[i]["transform"], pairs[c].true_transform)
        assert ang <= 1e-3 and dt <= 1e-3, (c, ang, dt)
    # part of the seeded call's answers, and more than it had
    part = a.hypothesis_results(2)
    same_bytes(part, (scored[0][:2], scored[1][:2], scored[2][:2]), "first two")
    with pytest.raises(hiplib.CvoError) as e:
        a.hypothesis_results(4)
    assert e.value.code == ERR_INVALID


def test_hypothesis_results_before_the_align_launch_is_waited_for(hiplib, pairs, seed_setup):
    ell, cases, truth_at, trans = seed_setup
    a = batch_of(hiplib, pairs, cases)
    scores = (hiplib.api.InnP * 27)(); best = np.full(3, -1, np.int32)
    rc = a.L.cvo_batch_hypothesis_results(a.h, 3, scores, best.ctypes.data_as(C.POINTER(C.c_int)))   # no seeding call yet
    assert rc == ERR_INVALID and (best == -1).all()
    a.seed_hypotheses(trans[[2, 0]], pairs=[2, 0], ell=ell)             # two of the three slots, in another order
    a.align_pairs_async([0, 2])
    got = a.hypothesis_results(2)
    assert got[2].tolist() == [truth_at[2], truth_at[0]]
    res_a = a.wait(2)
    b = batch_of(hiplib, pairs, cases)
    start_from_host(hiplib, b, trans, truth_at)
    res_b = b.wait(b.align_pairs_async([0, 2]))
    same_results(res_a, res_b, "seeded subset")


def test_scores_only_call_leaves_the_alignment_alone(hiplib, pairs, seed_setup):
    ell, cases, truth_at, trans = seed_setup
    b = batch_of(hiplib, pairs, cases)
    start_from_host(hiplib, b, trans, truth_at)
    res_plain = b.align(3)
    c = batch_of(hiplib, pairs, cases)
    start_from_host(hiplib, c, trans, truth_at)
    c.score_hypotheses(trans, ell=ell)                                  # between set_state and the launch
    res_scored = c.align(3)
    same_results(res_scored, res_plain, "scores-only call in between")
    # and with the device states carried (no set_state in between): a warm second launch either way
    c.score_hypotheses(trans, ell=ell)
    same_results(c.align(3), b.align(3), "scores-only call before a warm launch")


def test_set_state_after_a_seed_overrides_it(hiplib, pairs, seed_setup):
    ell, cases, truth_at, trans = seed_setup
    never = batch_of(hiplib, pairs, cases)
    wrong = [(t + 1) % 9 for t in truth_at]                             # the start states of a batch that was never seeded
    start_from_host(hiplib, never, trans, wrong)
    res_never = never.align(3)
    a = batch_of(hiplib, pairs, cases)
    a.seed_hypotheses(trans, ell=ell)
    start_from_host(hiplib, a, trans, wrong)
    same_results(a.align(3), res_never, "set_state after the seed")
    a.seed_hypotheses(trans, ell=ell)                                   # reset_states drops a seed too: back to what set_state gave
    a.reset_states()
    same_results(a.align(3), res_never, "reset_states after the seed")


# ---- 6. argument errors
def raw_batch_call(b, which, count, pairs, k, trans, ell, scores, best):
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    pr = None if pairs is None else np.ascontiguousarray(pairs, np.int32)
    t = None if trans is None else np.ascontiguousarray(trans, np.float32)
    args = [b.h, count, None if pr is None else pr.ctypes.data_as(ip), k, None if t is None else t.ctypes.data_as(fp), C.c_float(ell)]
    if which == "score":
        return b.L.cvo_batch_score_hypotheses(*args, scores, None if best is None else best.ctypes.data_as(ip))
    return b.L.cvo_batch_seed_hypotheses_async(*args)


@pytest.fixture(scope="module")
def undisturbed(hiplib, pairs, seed_setup):
    ell, cases, truth_at, trans = seed_setup
    b = batch_of(hiplib, pairs, cases[:2])
    return b.align(2)


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
    ("slot_out_of_range", dict(pairs=[0, 4]), ERR_INVALID),
    ("slot_negative", dict(pairs=[-1, 0]), ERR_INVALID),
    ("slot_twice", dict(pairs=[1, 1]), ERR_INVALID),
    ("stream_slot", dict(pairs=[0, 2]), ERR_INVALID),
    ("empty_cloud", dict(pairs=[0, 3]), ERR_EMPTY),
]


@pytest.mark.parametrize("which", ["score", "seed"])
@pytest.mark.parametrize("name,change,code", BAD_CALLS, ids=[c[0] for c in BAD_CALLS])
def test_argument_errors_change_nothing(hiplib, pairs, seed_setup, undisturbed, name, change, code, which):
    import torch
    ell, cases, truth_at, trans = seed_setup
    b = hiplib.CvoBatch(4)
    for i, c in enumerate(cases[:2]):
        p = pairs[c]
        b.set_pair(i, p.fixed.xyz, p.fixed.feat, p.moving.xyz, p.moving.feat)
    p = pairs[cases[2]]                                                 # slot 2: a stream slot; slot 3: never filled
    b.advance_clouds([2], [(torch.from_numpy(p.fixed.xyz).cuda(), torch.from_numpy(p.fixed.feat).cuda(), "channels_first")])
    args = dict(count=2, pairs=[0, 1], k=9, trans=trans[:2].copy(), ell=ell)
    poison = change.get("poison")
    args.update({k: v for k, v in change.items() if k != "poison"})
    if poison is not None:
        args["trans"][1, 8, 2, 3] = poison                              # the last entry but a few of the call's transforms
    scores = (hiplib.api.InnP * (2 * 65))()
    for s in scores:
        s.value, s.num, s.num_e = -7.0, -7, -7
    best = np.full(2, -7, np.int32)
    rc = raw_batch_call(b, which, args["count"], args["pairs"], args["k"], args["trans"], args["ell"], scores, best)
    assert rc == code, (name, rc, hiplib.api.load_library().cvo_last_error())
    assert all(s.value == -7.0 and s.num == -7 and s.num_e == -7 for s in scores) and (best == -7).all()
    same_results(b.align(2), undisturbed, name)                         # ... and the start states are those of an undisturbed batch


def test_null_scores_and_handle_form_errors(hiplib, pairs, seed_setup):
    ell, cases, truth_at, trans = seed_setup
    b = batch_of(hiplib, pairs, cases[:2])
    assert raw_batch_call(b, "score", 2, [0, 1], 9, trans[:2], ell, None, None) == ERR_INVALID
    best = np.full(2, -7, np.int32)
    scores = (hiplib.api.InnP * 18)()
    assert raw_batch_call(b, "score", 2, None, 9, trans[:2], ell, scores, None) == 0     # pairs NULL: 0 .. count-1; best NULL: not written
    g = handle_for(hiplib, *clouds_of(pairs[cases[0]]))
    fp = C.POINTER(C.c_float)
    t = np.ascontiguousarray(trans[0], np.float32)
    hs = (hiplib.api.InnP * 65)()
    for s in hs:
        s.value, s.num = -7.0, -7
    L = g.L
    assert L.cvo_score_hypotheses(g.h, MOVING, FIXED, 9, None, C.c_float(ell), hs, None) == ERR_INVALID
    assert L.cvo_score_hypotheses(g.h, MOVING, FIXED, 9, t.ctypes.data_as(fp), C.c_float(ell), None, None) == ERR_INVALID
    assert L.cvo_score_hypotheses(g.h, MOVING, FIXED, 0, t.ctypes.data_as(fp), C.c_float(ell), hs, None) == ERR_INVALID
    big = np.tile(np.eye(3, 4, dtype=np.float32), (65, 1, 1))
    assert L.cvo_score_hypotheses(g.h, MOVING, FIXED, 65, big.ctypes.data_as(fp), C.c_float(ell), hs, None) == ERR_INVALID
    assert L.cvo_score_hypotheses(g.h, MOVING, FIXED, 9, t.ctypes.data_as(fp), C.c_float(float("nan")), hs, None) == ERR_INVALID
    bad = t.copy(); bad[4, 1, 1] = np.inf
    assert L.cvo_score_hypotheses(g.h, MOVING, FIXED, 9, bad.ctypes.data_as(fp), C.c_float(ell), hs, None) == ERR_INVALID
    assert L.cvo_score_hypotheses(g.h, MOVING, 2, 9, t.ctypes.data_as(fp), C.c_float(ell), hs, None) == ERR_EMPTY   # no PREVIOUS cloud
    assert all(s.value == -7.0 and s.num == -7 for s in hs)
    assert L.cvo_score_hypotheses(g.h, MOVING, FIXED, 9, t.ctypes.data_as(fp), C.c_float(ell), hs, None) == 0
    assert hs[truth_at[0]].num > 1
    g.close()
