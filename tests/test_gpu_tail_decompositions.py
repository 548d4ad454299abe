"""The score block answered in the align launch's tail (cvo_batch_set_tail_scores, cvo_set_tail_scores) and the self products answered from a cloud's
four-entry table, under every launch decomposition: the knobs of test_workgroup_counts_tiles_and_overflow_fallback_agree with tails on, several pairs per
workgroup (cvo_batch_set_max_workgroups), several launches in flight, the handle route, and a table driven past its four entries.

Every tail is held to the score-kernel path of the SAME launch configuration (counts and inliers exact, values and cos_angle at rel 1e-6, the Hessian by the
1e-3-of-max rule: _check of tests/test_gpu_tail_scores.py) and, once per pair, to the oracle at rel 1e-5.  The alignment must not notice the tail: pose, iter,
A_nonzero, iterations_run and ell are bit-equal with tails on and off.  The answer masks are held to the models of tests/tail_cases.py (whose inputs
tests/test_tail_cases.py shows to be sharp); the layout a launch gets comes from the host's plan as tests/test_gpu_lopsided_pairs.py restates it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tail_cases as tc
import test_gpu_lopsided_pairs as lp
from test_gpu_lopsided_pairs import env, plan, same_bytes, workgroups
from test_gpu_tail_scores import _check

pytestmark = pytest.mark.gpu

TAIL3 = tc.PRE | tc.POST | tc.HESSIAN
_matrix = {}


def plan_y_mode(cfg, n_pairs=len(tc.PAIRS), nf_max=tc.NF_MAX, nm_max=tc.NM_MAX):
    """the layout of the moving cloud a configuration's launch gets: the forced one, else the plan's -- the same at both ends of sizeof(Shared), and by both
    builds' figures where the three-wave build may run it"""
    if "CVO_HIP_Y_MODE" in cfg:
        return int(cfg["CVO_HIP_Y_MODE"])
    G = workgroups(nf_max, cfg["wgs"], n_pairs=n_pairs)
    builds = (8, 12) if cfg.get("CVO_HIP_WIDE") == 2 else (8,)
    cap = lp.LDS_CAP
    try:
        lp.LDS_CAP = (160 // int(cfg.get("CVO_HIP_WGS_PER_CU", 1)) - 4) * 1024          # plan: lds_cap with two workgroups per CU
        seen = {plan(nf_max, nm_max, G, S, max_waves=mw, tile_request=int(cfg.get("CVO_HIP_TILE", 0)), allow_lds="CVO_HIP_NO_YLDS" not in cfg)[0]
                for S in (0, lp.SHARED_MAX) for mw in builds}
    finally:
        lp.LDS_CAP = cap
    assert len(seen) == 1, (cfg, seen)
    return seen.pop()


def check_masks(cfg, y_mode, cloud, ell, mask, self_bits, where):
    """one pair's answer mask against the model of tests/tail_cases.py"""
    if y_mode != 1:
        assert mask & TAIL3 == 0, where
    else:
        side = tc.pre_class(cloud, ell, tc.capn(cfg))
        assert side is not None, where
        assert bool(mask & tc.PRE) == side, (where, mask)
        if tc.converged(cfg) and not tc.capacities_cut(cfg):
            assert mask & (tc.POST | tc.HESSIAN) == tc.POST | tc.HESSIAN, (where, mask)
    assert bool(mask & tc.POST) == bool(mask & tc.HESSIAN), (where, mask)
    assert mask & (tc.FIXED | tc.MOVING) == self_bits, (where, mask, self_bits)


def run_config(hiplib, oracle, cfg, with_oracle=False):
    """one configuration of the matrix: a batch with tails and one without, three rounds; ([(pair, round, y_mode, mask)], what the mask model objects to).
    Status, alignment and values are asserted on the spot; the mask model's objections are gathered, so that the masks of a configuration that misses it are
    still there for the matrix as a whole."""
    key = tc.config_id(cfg)
    if key in _matrix:
        return _matrix[key]
    objections = []
    clouds = tc.matrix_clouds(); n = len(clouds)
    y_mode = plan_y_mode(cfg)
    prm = hiplib.default_params(); prm.max_iter = tc.max_iter(cfg)
    tables = [(tc.SelfTable(), tc.SelfTable()) for _ in range(n)]
    out = []
    with env(**tc.knobs(cfg)):
        ref = hiplib.CvoBatch(n, prm); B = hiplib.CvoBatch(n, prm)
        try:
            for b in (ref, B):
                b.set_workgroups(cfg["wgs"]); b.set_pairs(clouds)
            B.set_tail_scores(True)
            for rnd in range(tc.ROUNDS):
                ref.align_async(n); ref.enqueue_innerproduct(n); rres = ref.wait(n); want = ref.innerproduct_results(n)
                B.align_async(n); res = B.wait(n); masks = B.last_tail_answers(n); got = B.innerproduct_results(n)
                for i in range(n):
                    where = (key, tc.PAIRS[i], rnd)
                    assert res[i]["status"] == 0 and rres[i]["status"] == 0, (where, res[i]["status"], rres[i]["status"])
                    same_bytes([res[i]], [rres[i]], where)
                    orc = tc.oracle_rounds(oracle, tc.PAIRS[i], tc.max_iter(cfg))[rnd]
                    assert np.float32(res[i]["ell"]) == orc["ell"], where
                    print(f"{where}: mask {masks[i]:05b}, inn_pre {got[i]['inn_pre'][0]:.9g} / {want[i]['inn_pre'][0]:.9g}, inn_post {got[i]['inn_post'][0]:.9g} / {want[i]['inn_post'][0]:.9g}")
                    _check(got[i], want[i], 1e-6)
                    if with_oracle:
                        _check(got[i], orc["scores"], 1e-5)
                    out.append((tc.PAIRS[i], rnd, y_mode, masks[i]))
                    self_bits = tc.tail_round(tables[i], res[i]["ell"])
                    try:
                        check_masks(cfg, y_mode, clouds[i], res[i]["ell"], masks[i], self_bits, where)
                    except AssertionError as e:
                        objections.append(str(e).splitlines()[0])
        finally:
            ref.close(); B.close()
    _matrix[key] = (out, objections)
    return _matrix[key]


# ----------------------------------------------------------------------------- 1. the decomposition matrix with tails on
@pytest.mark.parametrize("cfg", tc.CONFIGS, ids=tc.config_id)
def test_tail_scores_under_a_decomposition(hiplib, oracle, cfg):
    """the oracle once per pair: under the library's own plan at one workgroup, and for the launch cut at ell 0.15.  (The two configurations with
    CVO_HIP_SKIN=0 are the ones whose lists are stale for EVERY transform but their own -- phase T's (r_c + reach) * 1.00001 > Rb with Rb = r_c --: their
    tails answer inn_post and the Hessian from one cull at the final transform, not from the candidate lists.)"""
    _, objections = run_config(hiplib, oracle, cfg, with_oracle=cfg in (tc.CONFIGS[0], dict(wgs=1, CVO_HIP_ROW_CAP=8, max_iter=3)))
    assert not objections, "\n".join(objections)


def test_the_matrix_holds_both_kinds_of_declined_launch(hiplib, oracle):
    """nothing is predicted for inn_post and the Hessian under cut capacities or a cut alignment -- but the matrix as a whole must contain a float4 launch
    that declines them while it answers inn_pre, and one that declines all three (else the assertions above never met a declining workgroup)"""
    runs = [r for cfg in tc.CONFIGS for r in run_config(hiplib, oracle, cfg)[0]]
    f4 = [m for _, _, y, m in runs if y == 1]
    assert any(m & TAIL3 == tc.PRE for m in f4), sorted(set(f4))
    assert any(m & TAIL3 == 0 for m in f4), sorted(set(f4))
    assert any(m & TAIL3 == TAIL3 for m in f4) and any(y != 1 for _, _, y, _ in runs)
    # the two ROW_CAP=8 launches: cut at ell 0.15 the two larger pairs decline inn_pre and the 300-point pair answers it; converged, everybody answers it
    cut = {(p, r): m for p, r, _, m in run_config(hiplib, oracle, dict(wgs=1, CVO_HIP_ROW_CAP=8, max_iter=3))[0]}
    full = {(p, r): m for p, r, _, m in run_config(hiplib, oracle, dict(wgs=1, CVO_HIP_ROW_CAP=8))[0]}
    for r in range(tc.ROUNDS):
        assert [cut[(p, r)] & tc.PRE for p in tc.PAIRS] == [0, 0, tc.PRE] and all(full[(p, r)] & tc.PRE for p in tc.PAIRS)


def test_tail_scores_on_the_three_wave_build(oracle):
    """CVO_HIP_WIDE=2 in a fresh child process, as test_three_wave_build sets it: the float4 layout on the build with three waves per SIMD"""
    code = ("import conftest, pyoracle, tail_cases as tc, test_gpu_tail_decompositions as t\n"
            "import cvo_slam_amd as ca\n"
            "pyoracle.build(); pyoracle.lib(); ca.load_library()\n"
            "for cfg in tc.CHILD_CONFIGS:\n"
            "    assert t.plan_y_mode(cfg) == 1\n"
            "    runs, objections = t.run_config(ca, pyoracle, cfg)\n"
            "    assert not objections, objections\n"
            "    assert all(m & t.TAIL3 == t.TAIL3 for _, _, _, m in runs), runs\n"
            "print('three-wave build: tails equal')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(os.path.abspath(__file__)), env=dict(os.environ, CVO_HIP_WIDE="2"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "three-wave build: tails equal" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ----------------------------------------------------------------------------- 2. several pairs per workgroup
def same_scores(a, b, where):
    for key in ("inn_pre", "inn_post", "inn_fixed_pcd", "inn_moving_pcd", "inliers", "cos_angle"):
        assert a[key] == b[key], (where, key, a[key], b[key])
    np.testing.assert_array_equal(a["post_hessian"], b["post_hessian"], err_msg=str(where))


def test_tails_of_several_pairs_in_a_row_on_one_workgroup(hiplib):
    """the 13 pairs of test_dynamic_pair_queue_gives_the_same_results with tails on: a launch capped to fewer pair slots than pairs runs several pairs, and
    several tails, on each workgroup.  Against the uncapped launch at the same workgroups per pair: align results and masks equal, scores bit-equal (the
    partial sums run in a fixed order); across workgroup counts the alignment is bit-equal and the scores agree at rel 1e-6."""
    clouds = [tc.small_pair(*p) for p in tc.QUEUE_PAIRS]; n = len(clouds)
    B = hiplib.CvoBatch(n); B.set_tail_scores(True); B.set_pairs(clouds)
    try:
        def launch(wgs, cap):
            B.set_workgroups(wgs); B.set_max_workgroups(cap); B.reset_states()
            B.align_async(n); res = B.wait(n)
            assert all(r["status"] == 0 for r in res), (wgs, cap, [r["status"] for r in res])
            return res, B.last_tail_answers(n), B.innerproduct_results(n)
        launch(1, 0)                                                  # (fills the clouds' tables: from here on every launch finds its self products there)
        want = launch(1, 0)
        assert all(m == 31 for m in want[1]), want[1]
        for wgs, cap in tc.QUEUE_LAUNCHES:
            free = launch(wgs, 0)
            same_bytes(want[0], free[0], (wgs, "uncapped"))
            for i in range(n):
                _check(free[2][i], want[2][i], 1e-6)
            for rep in range(2):
                res, masks, got = launch(wgs, cap)
                print(f"wgs {wgs} cap {cap} rep {rep}: masks {masks}")
                same_bytes(want[0], res, (wgs, cap, rep))
                assert masks == free[1], (wgs, cap, rep, masks, free[1])
                for i in range(n):
                    same_scores(got[i], free[2][i], (wgs, cap, rep, i))
    finally:
        B.close()


# ----------------------------------------------------------------------------- 3. several launches in flight
def test_four_tail_launches_in_flight(hiplib):
    """four batches of 8 pairs, adoption and tails on, all queued before any is waited for, three rounds: each batch against its own twin without tails
    (run alone, the score launch behind the align launch), its masks against the model"""
    cfg = dict(wgs=1)
    sets = [[tc.small_pair(*p) for p in b] for b in tc.FLIGHT_PAIRS]; n = len(sets[0])
    y_mode = plan_y_mode(cfg, n_pairs=n, nf_max=max(tc.FLIGHT_SIZES), nm_max=max(tc.FLIGHT_SIZES))
    assert y_mode == 1 and tc.capn(cfg, max(tc.FLIGHT_SIZES)) == 512
    Bs, refs = [], []
    try:
        for cl in sets:
            B = hiplib.CvoBatch(n); B.set_workgroups(1); B.set_adoption(True); B.set_pairs(cl); B.set_tail_scores(True); Bs.append(B)
            r = hiplib.CvoBatch(n); r.set_workgroups(1); r.set_pairs(cl); refs.append(r)
        tables = [[(tc.SelfTable(), tc.SelfTable()) for _ in range(n)] for _ in sets]
        helped = 0
        for rnd in range(tc.ROUNDS):
            for B in Bs:
                B.align_async(n)
            for b, (B, r) in enumerate(zip(Bs, refs)):
                res = B.wait(n); masks = B.last_tail_answers(n); got = B.innerproduct_results(n); helped += B.last_adoptions()
                r.align_async(n); r.enqueue_innerproduct(n); rres = r.wait(n); want = r.innerproduct_results(n)
                for i in range(n):
                    where = ("in flight", b, i, rnd)
                    assert res[i]["status"] == 0 and rres[i]["status"] == 0, (where, res[i]["status"])
                    same_bytes([res[i]], [rres[i]], where)
                    _check(got[i], want[i], 1e-6)
                    check_masks(cfg, y_mode, sets[b][i], res[i]["ell"], masks[i], tc.tail_round(tables[b][i], res[i]["ell"]), where)
        print(f"four launches in flight: {helped} adoptions in {tc.ROUNDS} rounds")
    finally:
        for b in Bs + refs:
            b.close()


# ----------------------------------------------------------------------------- 4. the handle route
@pytest.mark.parametrize("knobs", tc.HANDLE_KNOBS, ids=tc.config_id)
def test_handle_tail_under_a_decomposition(hiplib, knobs):
    """CVO_HIP_HANDLE_TAIL=kernel on one handle, the tracker's sequence match_odometry + compute_innerproduct(result) over four frames, at 1, 3 and 8
    workgroups: against the same handle with the mode off; a transform other than the result is not answered from the tail"""
    from helpers import make_tf
    p, q = (tc.small_pair(*s) for s in tc.HANDLE_PAIRS)
    tf = make_tf([0.3, -1.0, 0.2], 0.004, [0.003, -0.002, 0.002]).astype(np.float32)
    moved = lambda x: np.ascontiguousarray(x @ tf[:, :3].T + tf[:, 3], dtype=np.float32)
    frames = [(p[2], p[3]), (q[2], q[3]), (moved(p[2]), p[3]), (moved(q[2]), q[3])]
    for wgs in tc.HANDLE_WGS:
        with env(CVO_HIP_HANDLE_TAIL="kernel", **knobs):
            tail, off = hiplib.Cvo(), hiplib.Cvo()
            try:
                tail.set_tail_scores(1); off.set_tail_scores(0)
                for g in (tail, off):
                    g.set_workgroups(wgs); g.set_pcd(p[0], p[1])
                for k, (x, f) in enumerate(frames):
                    sc = {}
                    for g in (tail, off):
                        g.match_odometry(x, f)
                        other = np.array(g.transform, np.float32).copy(); other[0, 3] += 0.01
                        sc[g] = (g.compute_innerproduct(g.transform), g.compute_innerproduct(other), g.compute_innerproduct(g.transform))
                    where = (knobs, wgs, k)
                    np.testing.assert_array_equal(np.array(tail.transform, np.float32), np.array(off.transform, np.float32), err_msg=str(where))
                    assert (tail.get_iteration_number(), tail.get_A_nonzero(), tail.get_state()["ell"]) == (off.get_iteration_number(), off.get_A_nonzero(), off.get_state()["ell"]), where
                    _check(sc[tail][0], sc[off][0], 1e-6)
                    _check(sc[tail][2], sc[off][2], 1e-6)
                    assert sc[tail][1]["inn_post"] == sc[off][1]["inn_post"] and sc[tail][1]["inliers"] == sc[off][1]["inliers"], where      # the score kernel's own numbers
                    assert sc[tail][1]["inn_post"][0] != sc[tail][0]["inn_post"][0], where
            finally:
                tail.close(); off.close()


# ----------------------------------------------------------------------------- 5. the self-product table
def oracle_self_products(oracle, cloud, ells):
    """{ell: ((value, count) of fip(fixed, fixed), of fip(moving, moving))} by the oracle"""
    o = oracle.OracleCvo(); o.set_pcd(cloud[0], cloud[1]); o.set_pcd(cloud[2], cloud[3])
    st = o.get_state()
    out = {}
    for e in sorted(set(ells)):
        o.set_state(st["R"], st["T"], float(e))
        got = [o.function_inner_product(s, None, s) for s in (oracle.SLOT_FIXED, oracle.SLOT_MOVING)]
        assert all(rc == 0 for rc, _ in got)
        out[e] = tuple(v for _, v in got)
    return out


def check_self(got, want, where):
    for g, w in zip(got, want):
        assert g[1] == w[1], (where, g, w)
        assert g[0] == pytest.approx(w[0], rel=1e-5), (where, g, w)


EYE_R, ZERO_T = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)


def test_handle_self_products_past_four_length_scales(hiplib, oracle):
    """one handle, ell driven through the order of tests/tail_cases.py (e5 evicts e4, asking e4 again evicts e5, e1 stays resident): every answer bit-equal
    to a handle that never keeps one (CVO_HIP_SELF_CACHE=0) and within 1e-5 of the oracle -- a stale entry would be off by more than 1 %"""
    F, M = hiplib.api.SLOT_FIXED, hiplib.api.SLOT_MOVING
    c = tc.small_pair(*tc.TABLE_PAIR)
    want = oracle_self_products(oracle, c, tc.ELL_ORDER)
    with env(CVO_HIP_SELF_CACHE=0):
        u = hiplib.Cvo()
    g = hiplib.Cvo()
    try:
        for h in (g, u):
            h.set_pcd(c[0], c[1]); h.set_pcd(c[2], c[3])
        for k, e in enumerate(tc.ELL_ORDER):
            vals = {}
            for h in (g, u):
                h.set_state(EYE_R, ZERO_T, float(e))
                vals[h] = (h.function_inner_product(F, None, F), h.function_inner_product(M, None, M))
            print(f"ell {e}: cached {vals[g]}, swept {vals[u]}, oracle {want[e]}")
            assert vals[g] == vals[u], (k, e, vals[g], vals[u])
            check_self(vals[g], want[e], (k, e))
    finally:
        g.close(); u.close()


def self_of(scores):
    return (scores["inn_fixed_pcd"], scores["inn_moving_pcd"])


def test_batch_self_products_past_four_length_scales(hiplib, oracle):
    """the same order on one pair of a batch, the ell set through set_state and carried by a launch of one iteration (which leaves it alone): through the score
    launch (enqueue_innerproduct) and through the tail, whose bits 2 and 3 must be the table model's hit or miss; the values equal those of a batch that
    never keeps one, either way"""
    c = tc.small_pair(*tc.TABLE_PAIR)
    want = oracle_self_products(oracle, c, tc.ELL_ORDER)
    prm = hiplib.default_params(); prm.max_iter = 1
    with env(CVO_HIP_SELF_CACHE=0):
        U = hiplib.CvoBatch(1, prm)
    S, T = hiplib.CvoBatch(1, prm), hiplib.CvoBatch(1, prm)
    try:
        for b in (U, S, T):
            b.set_workgroups(1); b.set_pairs([c])
        T.set_tail_scores(True)
        tables = (tc.SelfTable(), tc.SelfTable())
        for k, e in enumerate(tc.ELL_ORDER):
            got = {}
            for b in (U, S):
                b.set_state(0, EYE_R, ZERO_T, float(e)); b.align_async(1); b.enqueue_innerproduct(1)
                res = b.wait(1); assert res[0]["status"] == 0 and np.float32(res[0]["ell"]) == e, (k, e, res[0])
                got[b] = b.innerproduct_results(1)[0]
            T.set_state(0, EYE_R, ZERO_T, float(e)); T.align_async(1)
            res = T.wait(1); assert res[0]["status"] == 0 and np.float32(res[0]["ell"]) == e, (k, e, res[0])
            mask = T.last_tail_answers(1)[0]; got[T] = T.innerproduct_results(1)[0]
            model = tc.tail_round(tables, e)
            print(f"ell {e}: mask {mask:05b}, model {model:05b}, fixed {got[T]['inn_fixed_pcd']} / {got[U]['inn_fixed_pcd']}")
            assert mask & (tc.FIXED | tc.MOVING) == model, (k, e, mask, model)
            assert bool(model) == tc.ELL_HITS[k]
            for b in (S, T):
                assert self_of(got[b]) == self_of(got[U]), (k, e, b is T, self_of(got[b]), self_of(got[U]))
                _check(got[b], got[U], 1e-6)
            check_self(self_of(got[T]), want[e], (k, e))
    finally:
        for b in (U, S, T):
            b.close()


def test_two_pairs_of_one_launch_share_a_cloud_at_two_length_scales(hiplib, oracle):
    """set_pairs_clouds with a repeated index: pairs 0 and 1 hold the same fixed cloud, at e1 and e2.  Both pairs' self products are right in every launch,
    and the shared table holds what the model says: of the requests of one score launch that name it only the first keeps it (cvo_capi.hip: score_enqueue),
    so the first fetch leaves e1 there, the second adds e2, and the third launch finds both"""
    import torch
    a, b = tc.small_pair(*tc.TABLE_PAIR), tc.small_pair(tc.TABLE_PAIR[0] + 1, tc.TABLE_PAIR[1])
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    clouds = [(dev(a[0]), dev(a[1]), "channels_first"), (dev(a[2]), dev(a[3]), "channels_first"), (dev(b[2]), dev(b[3]), "channels_first")]
    ells = (tc.E1, tc.E2)
    want = [oracle_self_products(oracle, (a[0], a[1], a[2], a[3]), ells)[tc.E1], oracle_self_products(oracle, (a[0], a[1], b[2], b[3]), ells)[tc.E2]]
    prm = hiplib.default_params(); prm.max_iter = 1
    with env(CVO_HIP_SELF_CACHE=0):
        U = hiplib.CvoBatch(2, prm)
    T = hiplib.CvoBatch(2, prm)
    try:
        for bt in (U, T):
            bt.set_workgroups(1); bt.set_pairs_clouds(clouds, [0, 0], [1, 2])
        T.set_tail_scores(True)
        shared, movs = tc.SelfTable(), (tc.SelfTable(), tc.SelfTable())
        seen = []
        for rnd in range(3):
            for bt in (U, T):
                for p in range(2):
                    bt.set_state(p, EYE_R, ZERO_T, float(ells[p]))
            U.align_async(2); U.enqueue_innerproduct(2); ures = U.wait(2); uw = U.innerproduct_results(2)
            T.align_async(2); res = T.wait(2); masks = T.last_tail_answers(2); got = T.innerproduct_results(2)
            model = tc.tail_launch([(shared, movs[0]), (shared, movs[1])], ells)
            print(f"shared cloud, launch {rnd}: masks {masks}, model {model}")
            for p in range(2):
                assert res[p]["status"] == 0 and ures[p]["status"] == 0 and np.float32(res[p]["ell"]) == ells[p], (rnd, p, res[p])
                assert masks[p] & (tc.FIXED | tc.MOVING) == model[p], (rnd, p, masks, model)
                assert self_of(got[p]) == self_of(uw[p]), (rnd, p, self_of(got[p]), self_of(uw[p]))
                _check(got[p], uw[p], 1e-6)
                check_self(self_of(got[p]), want[p], (rnd, p))
            seen.append([m & tc.FIXED for m in model])
        assert seen == [[0, 0], [tc.FIXED, 0], [tc.FIXED, tc.FIXED]] and shared.slots[:2] == [tc.E1, tc.E2]
    finally:
        U.close(); T.close()


def test_a_cloud_overwritten_at_a_cached_length_scale(hiplib, oracle):
    """set_pair with clouds of the same sizes and other points, at an ell both tables hold: the tables are emptied with the points, the tail declines the self
    products and the values are the new clouds'"""
    old, new = tc.small_pair(*tc.TABLE_PAIR), tc.small_pair(tc.TABLE_PAIR[0] + 2, tc.TABLE_PAIR[1])
    assert old[0].shape == new[0].shape and old[2].shape == new[2].shape
    want_old, want_new = (oracle_self_products(oracle, c, [tc.E1])[tc.E1] for c in (old, new))
    assert all(abs(o[0] - w[0]) > 1e-3 * abs(w[0]) for o, w in zip(want_old, want_new))          # the old value would not pass for the new one
    prm = hiplib.default_params(); prm.max_iter = 1
    T = hiplib.CvoBatch(1, prm)
    try:
        T.set_workgroups(1); T.set_tail_scores(True); T.set_pair(0, *old)
        tables = (tc.SelfTable(), tc.SelfTable())

        def launch(want, where):
            T.set_state(0, EYE_R, ZERO_T, float(tc.E1)); T.align_async(1); res = T.wait(1)
            assert res[0]["status"] == 0 and np.float32(res[0]["ell"]) == tc.E1, (where, res[0])
            mask = T.last_tail_answers(1)[0]; got = T.innerproduct_results(1)[0]
            assert mask & (tc.FIXED | tc.MOVING) == tc.tail_round(tables, tc.E1), (where, mask)
            check_self(self_of(got), want, where)
            return mask
        assert [launch(want_old, k) & 12 for k in range(2)] == [0, 12]
        T.set_pair(0, *new)
        for t in tables:
            t.clear()
        assert [launch(want_new, 2 + k) & 12 for k in range(2)] == [0, 12]
    finally:
        T.close()
