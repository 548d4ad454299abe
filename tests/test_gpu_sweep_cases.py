"""Every consumer of the box-culled sweep (cvo_sweep.hpp: cvo_score_kernel, cvo_support_kernel, cvo_hyp_score_kernel,
cvo_pose_model_sweep_kernel, cvo_match_kernel, the align launch's tail scores, and the align kernel's own list cull) on clouds whose group
boxes are TIGHT (tests/sweep_cases.py), against the oracle and the dense numpy readings.  tests/test_sweep_cases.py shows on the CPU that
the cull skips 45 to 93 % of its (wave, group) tests on these clouds, loses no hit, and that three wrong slope bounds would lose hits; every
other reading test runs on synth.make_small_pair clouds, where the cull skips nothing.  The second half replaces a cloud through every route
there is after its boxes were made: boxes left over from the cloud before give zero pairs or a wrong count.

The acceptance rules are those of each kernel's own file, imported from it: tests/test_gpu_point_support.py (counts equal, sums rtol 1e-6),
test_gpu_point_matches.py, test_gpu_hypotheses.py, test_gpu_pose_models.py; the inner product to rtol 1e-6 against second_reading (float64
sums) and 2e-6 against the oracle, Hessians to rtol 1e-3 / atol 1e-3 of the largest entry (test_gpu_parity.py::test_score_box_cull_edge_cases),
alignments by test_gpu_parity.py::test_workgroup_counts_tiles_and_overflow_fallback_agree's rule: nnz of every iteration and the iteration
count equal, pose within 1e-6 rad / 1e-6 m."""
import functools

import numpy as np
import pytest

import match_reading
import second_reading as sr
import support_reading
import sweep_cases as sc
from helpers import rot_trans_err
from test_gpu_hypotheses import check_against_reading as check_hypotheses
from test_gpu_parity import env
from test_gpu_point_matches import GAP, RTOL, check_against_reading as check_matches_near_the_origin
from test_gpu_point_support import KEYS as SUPPORT_KEYS, check_against_reading as check_support
from test_gpu_pose_models import check_against_reading as check_models

pytestmark = pytest.mark.gpu

FIXED, MOVING, PREVIOUS = 0, 1, 2
ODO, KEY = 0, 1
EYE = np.eye(3, 4, dtype=np.float32)
CASES = [(name, ell) for name in sc.NAMES for ell in sc.ELLS]
VARIANTS = ("stored", "moved")
SCORE_KEYS = ("inn_pre", "inn_post", "inn_fixed_pcd", "inn_moving_pcd")


@functools.lru_cache(maxsize=None)
def clouds(name, ell, variant="stored"):
    """(fixed, moving, tf): the case's clouds as (xyz, feat) and the transform that goes with them (None: as stored)"""
    c = sc.case(name, ell)
    if variant == "moved":
        c = sc.moved(c)
    return (c[0], c[1]), (c[2], c[3]), (sc.transform() if variant == "moved" else None)


def handle_for(hiplib, fixed, moving, ell):
    g = hiplib.Cvo(); g.set_pcd(*fixed); g.set_pcd(*moving); g.set_state(np.eye(3), np.zeros(3), ell)
    return g


def oracle_for(oracle, fixed, moving, ell):
    o = oracle.OracleCvo(); o.set_pcd(*fixed); o.set_pcd(*moving); o.set_state(np.eye(3), np.zeros(3), ell)
    return o


def reading_inner_product(a, tf, b, ell):
    xa = a[0] if tf is None else support_reading.move(tf, a[0])
    return sr.inner_product(xa, a[1], b[0], b[1], np.float32(ell))


def check_inner_product(g, o, slots, sa, tf, sb, ell, where):
    """function_inner_product and se3_hessian of slots sa (moved by tf), sb against the oracle and the second reading; returns the pair count"""
    rc, want = o.function_inner_product(sa, tf, sb); assert rc == 0
    got = g.function_inner_product(sa, tf, sb)
    val, num = reading_inner_product(slots[sa], tf, slots[sb], ell)
    print(where, "pairs", num, "rel to the oracle", abs(got[0] - want[0]) / max(want[0], 1e-300), "to the reading", abs(got[0] - val) / max(val, 1e-300))
    assert got[1] == want[1] == num, (where, got, want, num)
    assert got[0] == pytest.approx(val, rel=1e-6) and got[0] == pytest.approx(want[0], rel=2e-6), (where, got, want, val)
    rc, Ho, inl_o, _ = o.se3_hessian(sa, tf, sb); assert rc == 0
    Hg, inl_g = g.se3_hessian(sa, tf, sb)
    assert inl_g == inl_o, (where, inl_g, inl_o)
    np.testing.assert_allclose(Hg, Ho, rtol=1e-3, atol=1e-3 * max(np.abs(Ho).max(), 1e-30), err_msg=str(where))
    return num


def check_matches(got, moving, fixed, ell, tf, where):
    """test_gpu_point_matches.check_against_reading; for clouds outside its "within 8 m of the origin" premise (fan_far) the means and the fit
    record's residual, whose tolerances are worked out from that premise, are left out: counts, best, sums and values only, by the same rules"""
    if max(np.abs(moving[0]).max(), np.abs(fixed[0]).max()) < 8.0:
        return check_matches_near_the_origin(got, moving, fixed, ell, tf, where)
    want = match_reading.matches(moving[0], moving[1], fixed[0], fixed[1], ell, tf)
    for side in ("moving", "fixed"):
        A = want["a"] if side == "moving" else want["a"].T
        matched = want[f"count_{side}"] > 0
        decided = want[f"gap_{side}"] > GAP
        open_rows = np.nonzero(matched & ~decided)[0]
        np.testing.assert_array_equal(got[f"count_{side}"], want[f"count_{side}"], err_msg=str((where, side)))
        np.testing.assert_allclose(got[f"sum_{side}"].astype(np.float64), want[f"sum_{side}"], rtol=RTOL, atol=0, err_msg=str((where, side)))
        np.testing.assert_allclose(got[f"best_value_{side}"].astype(np.float64), want[f"best_value_{side}"].astype(np.float64), rtol=RTOL, atol=0, err_msg=str((where, side)))
        np.testing.assert_array_equal(got[f"best_{side}"][decided], want[f"best_{side}"][decided], err_msg=str((where, side)))
        assert open_rows.size <= 0.01 * int(matched.sum()), (where, side, open_rows.size)
        for r in open_rows:
            j = int(got[f"best_{side}"][r])
            assert 0 <= j < A.shape[1] and A[r, j] >= A[r].max() * (1.0 - GAP), (where, side, r, j)
        fit, wfit = got[f"fit_{side}"], want[f"fit_{side}"]
        assert fit["rows"] == wfit["rows"] and fit["matched"] == wfit["matched"], (where, side, fit, wfit)
        assert fit["sum_w"] == pytest.approx(wfit["sum_w"], rel=RTOL, abs=0), (where, side)
    return want


def few_steps(hiplib):
    """parameters for the launches whose RESULT is asked about: three iterations.  Run to the end, these alignments drift until no pair is left
    (half the partners pull one way, half the other), and "equal zeros" would prove nothing; after three steps the pose has left the start and
    the partners are still in reach"""
    prm = hiplib.default_params(); prm.max_iter = 3
    return prm


def check_scores(got, want, where):
    """compute_innerproduct's pair counts and inliers against the oracle's (test_gpu_parity.py::test_score_box_cull_edge_cases)"""
    assert [got[k][1] for k in SCORE_KEYS] == [want[k][1] for k in SCORE_KEYS], (where, [got[k] for k in SCORE_KEYS], [want[k] for k in SCORE_KEYS])
    assert got["inliers"] == want["inliers"], where


# ---- 1. every consumer, handle form, on every case
@pytest.mark.parametrize("name,ell", CASES)
def test_inner_product_hessian_and_score_block_against_the_oracle(hiplib, oracle, name, ell):
    for variant in VARIANTS:
        fixed, moving, tf = clouds(name, ell, variant)
        slots = {FIXED: fixed, MOVING: moving}
        g, o = handle_for(hiplib, fixed, moving, ell), oracle_for(oracle, fixed, moving, ell)
        num = check_inner_product(g, o, slots, MOVING, tf, FIXED, ell, (name, ell, variant, "moving on fixed"))
        assert num > 1
        inv = None if tf is None else np.concatenate([tf[:, :3].T, -(tf[:, :3].T @ tf[:, 3])[:, None]], axis=1).astype(np.float32)
        assert check_inner_product(g, o, slots, FIXED, inv, MOVING, ell, (name, ell, variant, "fixed on moving")) > 1       # the roles swapped: the moving cloud's boxes
        check_inner_product(g, o, slots, FIXED, None, FIXED, ell, (name, ell, variant, "fixed on itself"))
        check_inner_product(g, o, slots, MOVING, tf, MOVING, ell, (name, ell, variant, "moving on itself"))
        t = sc.transform() if tf is None else tf
        rc, want = o.compute_innerproduct(t); assert rc == 0
        got = g.compute_innerproduct(t)
        check_scores(got, want, (name, ell, variant))
        assert max(got[k][1] for k in ("inn_pre", "inn_post")) > 1
        g.close()


@pytest.mark.parametrize("name,ell", CASES)
def test_point_support_against_the_reading(hiplib, name, ell):
    for variant in VARIANTS:
        fixed, moving, tf = clouds(name, ell, variant)
        g = handle_for(hiplib, fixed, moving, ell)
        want = check_support(g.point_support(MOVING, tf, FIXED), moving, fixed, ell, tf, (name, ell, variant))
        assert want[1].sum() > 0
        want = check_support(g.point_support(FIXED, None, MOVING), fixed, moving, ell, None, (name, ell, variant, "swapped"))
        assert variant == "moved" or want[1].sum() > 0
        g.close()


@pytest.mark.parametrize("name,ell", CASES)
def test_point_matches_against_the_reading(hiplib, name, ell):
    for variant in VARIANTS:
        fixed, moving, tf = clouds(name, ell, variant)
        g = handle_for(hiplib, fixed, moving, ell)
        want = check_matches(g.point_matches(MOVING, tf, FIXED), moving, fixed, ell, tf, (name, ell, variant))
        assert want["count_moving"].sum() > 0
        g.close()


def hypothesis_transforms():
    """K = 3: the identity, the moved cases' transform, and one that takes the clouds apart"""
    return np.stack([EYE, sc.transform(), sc.away()])


@pytest.mark.parametrize("name,ell", CASES)
def test_score_hypotheses_against_the_reading(hiplib, name, ell):
    trans = hypothesis_transforms()
    for variant in VARIANTS:
        fixed, moving, tf = clouds(name, ell, variant)
        g = handle_for(hiplib, fixed, moving, ell)
        got = g.score_hypotheses(MOVING, FIXED, trans, ell)
        want = check_hypotheses(got, moving, fixed, trans, ell, (name, ell, variant))
        assert want[1][1 if variant == "moved" else 0] > 1
        assert got[1][2] == 1 and got[0][2] == 0 and want[1][2] == 1        # nothing in reach: count 0 reads 1 (cvo.cpp:455-456)
        assert got[2] == want[2]
        g.close()


@pytest.mark.parametrize("name,ell", CASES)
def test_pose_models_against_the_reading(hiplib, name, ell):
    trans = hypothesis_transforms()
    for variant in VARIANTS:
        fixed, moving, tf = clouds(name, ell, variant)
        g = handle_for(hiplib, fixed, moving, ell)
        want = check_models(g.pose_models(MOVING, FIXED, trans, ell), moving, fixed, trans, ell, (name, ell, variant))
        assert want[1][1 if variant == "moved" else 0] > 1 and want[1][2] == 1
        g.close()


@pytest.mark.parametrize("name,ell", CASES)
def test_alignment_against_the_oracle(hiplib, oracle, name, ell):
    """the align kernel culls its candidate lists with its own copy of the box test; one workgroup and three, and with a list margin of 0,
    which culls at every iteration"""
    for variant in VARIANTS:                                                # (moved: the alignment starts from the identity on the displaced cloud)
        fixed, moving, _ = clouds(name, ell, variant)
        o = oracle_for(oracle, fixed, moving, ell)
        rc, otr = o.align(trace_cap=2000); assert rc == 0
        ost = o.get_state()
        want_nnz = [r["nnz"] for r in otr]
        assert variant == "moved" or want_nnz[0] > 0                            # the partners that carry their column's colours (sweep_cases.case)
        for cfg in (dict(wgs=1), dict(wgs=3), dict(wgs=1, CVO_HIP_SKIN=0.0), dict(wgs=3, CVO_HIP_SKIN=0.0)):
            with env(**{k: v for k, v in cfg.items() if k.startswith("CVO_")}):
                g = hiplib.Cvo(); g.set_workgroups(cfg["wgs"]); g.set_pcd(*fixed); g.set_pcd(*moving); g.set_state(np.eye(3), np.zeros(3), ell)
                gtr = g.align(trace_cap=2000)
            re, te = rot_trans_err(g.transform, ost["transform"])
            print(name, ell, variant, cfg, "iterations", len(gtr), "first nnz", want_nnz[0], "rot err", re, "trans err", te)
            assert [r["nnz"] for r in gtr] == want_nnz, (name, ell, variant, cfg)
            assert re <= 1e-6 and te <= 1e-6, (name, ell, variant, cfg, re, te)
            assert g.get_iteration_number() == ost["iter"], (name, ell, variant, cfg)
            g.close()


# ---- 2. the batch forms: all cases as the pairs of one batch
@pytest.fixture(scope="module")
def batch(hiplib):
    """every (case, ell), as stored, as a pair of one CvoBatch started at that ell and aligned (few_steps) with the score block in the launch's tail"""
    pairs = [clouds(name, ell) for name, ell in CASES]
    b = hiplib.CvoBatch(len(pairs), few_steps(hiplib))
    b.set_pairs([(f[0], f[1], m[0], m[1]) for f, m, _ in pairs])
    for i, (_, ell) in enumerate(CASES):
        b.set_state(i, np.eye(3), np.zeros(3), ell)
    b.set_tail_scores(True)
    res = b.align(len(pairs))
    assert all(r["status"] == 0 for r in res)
    yield b, pairs, res
    b.close()


def test_batch_forms_at_the_results(hiplib, oracle, batch):
    """point_support, point_matches, result_models and the tail's score block answer at each pair's own result transform and ell"""
    b, pairs, res = batch
    n = len(pairs)
    scores = b.innerproduct_results(n)
    support, matches, models = b.point_support(), b.point_matches(), b.result_models()
    for i, ((fixed, moving, _), r) in enumerate(zip(pairs, res)):
        where = ("batch", CASES[i])
        tf, ell = r["transform"], r["ell"]
        want = check_support(tuple(support[i][k] for k in SUPPORT_KEYS), moving, fixed, ell, tf, where)
        assert want[1].sum() > 0
        check_matches(matches[i], moving, fixed, ell, tf, where)
        check_models(tuple(a[i:i + 1] for a in models), moving, fixed, tf[None], ell, where)
        o = oracle.OracleCvo(); o.set_pcd(*fixed); o.set_pcd(*moving); o.set_state(r["R"], r["T"], ell)
        rc, want_scores = o.compute_innerproduct(tf); assert rc == 0
        check_scores(scores[i], want_scores, where)
        assert scores[i]["inn_post"][1] == int(want[1].sum())
    # the score kernel's answer to the same question (no tail): the launch of test_the_score_kernel_sweeps_all_groups_in_one_chunk's kind
    b.set_tail_scores(False)
    plain = b.compute_innerproduct(n)
    for i in range(n):
        check_scores(plain[i], scores[i], ("score kernel", CASES[i]))
    b.set_tail_scores(True)


def test_batch_hypotheses_and_pose_models(hiplib, batch):
    b, pairs, _ = batch
    trans = hypothesis_transforms()
    for ell in sc.ELLS:
        idx = [i for i, c in enumerate(CASES) if c[1] == ell]
        many = np.stack([trans] * len(idx))
        scores = b.score_hypotheses(many, pairs=idx, ell=ell)
        models = b.pose_models(many, pairs=idx, ell=ell)
        for k, i in enumerate(idx):
            fixed, moving, _ = pairs[i]
            want = check_hypotheses((scores[0][k], scores[1][k]), moving, fixed, trans, ell, ("batch", CASES[i]))
            assert want[1][0] > 1 and scores[2][k] == want[2]
            check_models(tuple(a[k] for a in models), moving, fixed, trans, ell, ("batch", CASES[i]))


def test_the_score_kernel_sweeps_all_groups_in_one_chunk(hiplib, oracle):
    """The score kernel deals a cloud's column groups to chunks = min(16, 4 CUs / (row blocks x requests)) workgroups per row block
    (score_enqueue, cvo_capi.hip); only with ONE chunk does a workgroup sweep all 67 groups of the 2 113-point cloud and enter box_sweep's
    second ballot round.  A batch's score block is five requests per pair, the fixed cloud against itself among them (34 row blocks): the
    smallest batch with 4 CUs / (34 x 5 pairs) below 2 -- four pairs, 20 requests, on 256 CUs.  All pairs are the same pair: equal answers,
    the oracle's counts."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ell = 0.15
    fixed, moving, _ = clouds("fan_ragged_2113", ell)
    row_blocks = (fixed[0].shape[0] + 63) // 64
    n = next(k for k in range(1, 64) if 4 * cus // (row_blocks * 5 * k) <= 1)
    print("CUs", cus, "pairs", n, "requests", 5 * n)
    b = hiplib.CvoBatch(n, few_steps(hiplib))
    b.set_pairs([(fixed[0], fixed[1], moving[0], moving[1])] * n)
    for i in range(n):
        b.set_state(i, np.eye(3), np.zeros(3), ell)
    res = b.align(n)
    got = b.compute_innerproduct(n)
    r = res[0]
    o = oracle.OracleCvo(); o.set_pcd(*fixed); o.set_pcd(*moving); o.set_state(r["R"], r["T"], r["ell"])
    rc, want = o.compute_innerproduct(r["transform"]); assert rc == 0
    assert want["inn_post"][1] > 1 and want["inn_fixed_pcd"][1] > fixed[0].shape[0]
    for i in range(n):
        assert res[i]["transform"].tobytes() == r["transform"].tobytes()
        check_scores(got[i], want, ("one chunk", i))
        for k in SCORE_KEYS:
            assert got[i][k] == got[0][k], (i, k)
            assert got[i][k][0] == pytest.approx(want[k][0], rel=2e-6), (i, k)
    b.close()


# ---- 3. boxes left over from the cloud before
# X and Y: two cases more than a metre apart whose clouds have different numbers of 32-point groups (20 and 20 against 4 and 2).  Each route is
# walked from X to Y (Y smaller) and from Y to X (Y larger): ask with the first so that its boxes exist, replace it, ask again, compare with the
# second's reading.
STALE_ELL = 0.15


@functools.lru_cache(maxsize=None)
def stale_pair(which):
    if which == "big":
        fixed, moving, _ = clouds("fan_tum", STALE_ELL)
        return fixed, moving
    fixed, moving, _ = clouds("fan_ragged_97", STALE_ELL)
    shift = np.array([3.0, 0.0, 0.0], np.float32)
    return (fixed[0] + shift, fixed[1]), (moving[0] + shift, moving[1])


ORDERS = [("big", "small"), ("small", "big")]


def test_the_stale_pairs_are_apart():
    (bf, bm), (sf, sm) = stale_pair("big"), stale_pair("small")
    gap = min(np.concatenate([sf[0], sm[0]])[:, 0]) - max(np.concatenate([bf[0], bm[0]])[:, 0])
    assert gap > 1.0
    assert [(c[0].shape[0] + 31) // 32 for c in (bf, bm, sf, sm)] == [20, 20, 4, 2]


def ask_handle(g, o, slots, sa, sb, where, hits=True):
    """function_inner_product, se3_hessian, point_support, point_matches, score_hypotheses and pose_models of slots sa on sb against the readings"""
    a, b = slots[sa], slots[sb]
    num = check_inner_product(g, o, slots, sa, None, sb, STALE_ELL, where)
    want = check_support(g.point_support(sa, None, sb), a, b, STALE_ELL, None, where)
    check_matches(g.point_matches(sa, None, sb), a, b, STALE_ELL, None, where)
    trans = hypothesis_transforms()
    check_hypotheses(g.score_hypotheses(sa, sb, trans, STALE_ELL), a, b, trans, STALE_ELL, where)
    check_models(g.pose_models(sa, sb, trans, STALE_ELL), a, b, trans, STALE_ELL, where)
    assert not hits or (num > 1 and want[1].sum() == num)


def ask_all(g, o, slots, where):
    for sa in slots:
        for sb in slots:
            ask_handle(g, o, slots, sa, sb, where + (sa, sb), hits=False)


@pytest.mark.parametrize("first,second", ORDERS)
def test_stale_boxes_set_pcd_and_update_fixed_pcd(hiplib, oracle, first, second):
    """the third and the fourth set_pcd replace the moving cloud; update_fixed_pcd moves it to the fixed slot"""
    (xf, xm), (yf, ym) = stale_pair(first), stale_pair(second)
    g, o = handle_for(hiplib, xf, xm, STALE_ELL), oracle_for(oracle, xf, xm, STALE_ELL)
    ask_all(g, o, {FIXED: xf, MOVING: xm}, (first, "before"))
    g.set_pcd(*yf); o.set_pcd(*yf)                                          # the third call: MOVING = Y's fixed cloud, next to X's
    ask_all(g, o, {FIXED: xf, MOVING: yf}, (first, "third set_pcd"))
    g.update_fixed_pcd(); o.update_fixed_pcd()
    g.set_pcd(*ym); o.set_pcd(*ym)                                          # the fourth
    ask_all(g, o, {FIXED: yf, MOVING: ym}, (first, "fourth set_pcd"))
    ask_handle(g, o, {FIXED: yf, MOVING: ym}, MOVING, FIXED, (first, "Y"))
    g.close()


@pytest.mark.parametrize("first,second", ORDERS)
def test_stale_boxes_update_previous_pcd_and_reset_keyframe(hiplib, oracle, first, second):
    (xf, xm), (yf, ym) = stale_pair(first), stale_pair(second)
    g, o = handle_for(hiplib, xf, xm, STALE_ELL), oracle_for(oracle, xf, xm, STALE_ELL)
    ask_all(g, o, {FIXED: xf, MOVING: xm}, (first, "before"))
    g.update_previous_pcd(); o.update_previous_pcd()                        # PREVIOUS = X's moving cloud
    g.set_pcd(*yf); o.set_pcd(*yf)
    ask_all(g, o, {FIXED: xf, MOVING: yf, PREVIOUS: xm}, (first, "update_previous_pcd"))
    g.reset_keyframe(EYE); o.reset_keyframe(EYE)                            # FIXED = PREVIOUS (X's moving cloud), PREVIOUS = MOVING (Y's fixed cloud)
    g.set_pcd(*ym); o.set_pcd(*ym)
    g.set_state(np.eye(3), np.zeros(3), STALE_ELL); o.set_state(np.eye(3), np.zeros(3), STALE_ELL)
    ask_all(g, o, {FIXED: xm, MOVING: ym, PREVIOUS: yf}, (first, "reset_keyframe"))
    ask_handle(g, o, {MOVING: ym, PREVIOUS: yf}, MOVING, PREVIOUS, (first, "Y"))
    g.close()


@pytest.mark.parametrize("first,second", ORDERS)
def test_stale_boxes_clouds_handed_in_directly(hiplib, oracle, first, second):
    """function_inner_product_clouds / se3_hessian_clouds keep two scratch clouds in the handle: every call replaces them"""
    (xf, xm), (yf, ym) = stale_pair(first), stale_pair(second)
    g = handle_for(hiplib, xf, xm, STALE_ELL)
    for k, (f, m) in enumerate(((xf, xm), (yf, ym), (ym, yf), (xm, xf), (yf, yf))):
        o = oracle_for(oracle, f, m, STALE_ELL)
        val, num = reading_inner_product(m, None, f, STALE_ELL)
        got = g.function_inner_product_clouds(m[0], m[1], f[0], f[1])
        assert got[1] == num > 1 and got[0] == pytest.approx(val, rel=1e-6), (first, k, got, val, num)
        if k % 2:                                                           # (and the Hessian form first in the same scratch clouds)
            f, m = m, f; o = oracle_for(oracle, f, m, STALE_ELL)
        rc, Ho, inl_o, _ = o.se3_hessian(MOVING, None, FIXED); assert rc == 0
        Hg, inl_g = g.se3_hessian_clouds(m[0], m[1], f[0], f[1])
        assert inl_g == inl_o > 0, (first, k)
        np.testing.assert_allclose(Hg, Ho, rtol=1e-3, atol=1e-3 * np.abs(Ho).max())
    g.close()


def ask_batch(b, oracle, fixed, moving, where, stream_slot=False):
    """slot 0 of the batch: hypotheses and pose models as it stands, then aligned from STALE_ELL: support, matches, model and scores at the result.
    A stream slot (advance_clouds) carries its own state: it offers no hypotheses, and its alignment starts where the slot stands"""
    trans = hypothesis_transforms()
    if not stream_slot:
        got = b.score_hypotheses(trans[None], pairs=[0], ell=STALE_ELL)
        want = check_hypotheses((got[0][0], got[1][0]), moving, fixed, trans, STALE_ELL, where)
        assert want[1][0] > 1
        check_models(tuple(a[0] for a in b.pose_models(trans[None], pairs=[0], ell=STALE_ELL)), moving, fixed, trans, STALE_ELL, where)
        b.set_state(0, np.eye(3), np.zeros(3), STALE_ELL)
    r = b.align_pairs([0])[0]
    assert r["status"] == 0
    tf, ell = r["transform"], r["ell"]
    want = check_support(tuple(b.point_support([0])[0][k] for k in SUPPORT_KEYS), moving, fixed, ell, tf, where)
    assert want[1].sum() > 0
    check_matches(b.point_matches([0])[0], moving, fixed, ell, tf, where)
    check_models(tuple(a[0:1] for a in b.result_models([0])), moving, fixed, tf[None], ell, where)
    o = oracle.OracleCvo(); o.set_pcd(*fixed); o.set_pcd(*moving); o.set_state(r["R"], r["T"], ell)
    rc, want_scores = o.compute_innerproduct(tf); assert rc == 0
    got = b.compute_innerproduct(1)[0]
    check_scores(got, want_scores, where)
    assert got["inn_post"][1] == int(want[1].sum())


def up(torch, cloud):
    return (torch.from_numpy(np.ascontiguousarray(cloud[0])).cuda(), torch.from_numpy(np.ascontiguousarray(cloud[1])).cuda())


@pytest.mark.parametrize("route", ["set_pair", "set_pairs", "set_pairs_clouds", "advance_clouds"])
@pytest.mark.parametrize("first,second", ORDERS)
def test_stale_boxes_batch_routes(hiplib, oracle, first, second, route):
    import torch
    b = hiplib.CvoBatch(2, few_steps(hiplib))
    for which in (first, second, first):
        fixed, moving = stale_pair(which)
        if route == "set_pair":
            b.set_pair(0, fixed[0], fixed[1], moving[0], moving[1])
        elif route == "set_pairs":
            b.set_pairs([(fixed[0], fixed[1], moving[0], moving[1])])
        elif route == "set_pairs_clouds":                                   # device-resident clouds, read where they are
            b.set_pairs_clouds([up(torch, fixed), up(torch, moving)], [0], [1])
        else:                                                               # a slot's next cloud: MOVING -> FIXED, the cloud -> MOVING
            b.advance_clouds([0], [up(torch, fixed)]); b.advance_clouds([0], [up(torch, moving)])
        ask_batch(b, oracle, fixed, moving, (route, first, which), stream_slot=route == "advance_clouds")
    b.close()


@pytest.mark.parametrize("first,second", ORDERS)
def test_stale_boxes_tracker_steps(hiplib, first, second):
    """CvoTracks.step_clouds: a stream's two objects take over the step's cloud; after a reset the stream starts again with other clouds, and a third
    step moves the clouds on (the new frame: the LAST 97 points of the first frame, four groups where the cloud before had 20)"""
    import torch
    T = hiplib.CvoTracks(2, few_steps(hiplib))

    def ask(obj, fixed, moving, r, where):
        tf, ell = r["transform"], r["ell"]
        assert r["status"] == 0
        want = check_support(tuple(T.point_support(obj, [0])[0][k] for k in SUPPORT_KEYS), moving, fixed, ell, tf, where)
        assert want[1].sum() > 0
        check_matches(T.point_matches(obj, [0])[0], moving, fixed, ell, tf, where)
        return int(want[1].sum())

    for which in (first, second):
        fixed, moving = stale_pair(which)
        T.reset(0)
        assert T.step_clouds([0], [up(torch, fixed)])[0]["phase"] == 0
        res = T.step_clouds([0], [up(torch, moving)])[0]
        assert res["phase"] == 1
        pairs = ask(ODO, fixed, moving, res["odometry"], ("tracker", first, which))
        assert res["odometry_scores"]["inn_post"][1] == pairs
    fixed, moving = stale_pair(second)
    tail = (np.ascontiguousarray(fixed[0][-97:]), np.ascontiguousarray(fixed[1][:, -97:]))
    res = T.step_clouds([0], [up(torch, tail)])[0]
    assert res["phase"] == 2
    ask(ODO, moving, tail, res["odometry"], ("tracker", first, "third step, odometry"))
    ask(KEY, fixed, tail, res["keyframe"], ("tracker", first, "third step, keyframe"))
    T.close()
