"""The inputs of tests/tail_cases.py are sharp: shown on the CPU, with the oracle and numpy alone.  Every (pair, configuration, round) of the decomposition
matrix is on one side of the inn_pre model or the other -- never between --, the two ROW_CAP=8 launches sit on opposite sides, and the order of length scales
that drives the self-product table evicts and keeps what it claims."""
import numpy as np
import pytest

import tail_cases as tc


def test_the_matrix_is_the_parity_list_and_more():
    """the 36 configurations of test_workgroup_counts_tiles_and_overflow_fallback_agree, the line-search table off, ROW_CAP=8 cut at ell 0.15 and, each in a
    process of its own, the three-wave build"""
    assert len(tc.PARITY_CONFIGS) == 36 and len(tc.CONFIGS) == 40
    assert sorted({c["wgs"] for c in tc.PARITY_CONFIGS}) == [1, 2, 3, 4, 5, 7, 32]
    seen = {k for c in tc.CONFIGS + tc.CHILD_CONFIGS for k in tc.knobs(c)}
    assert seen == {"CVO_HIP_" + k for k in ("TILE", "FLAT_CAP", "SKIN", "SKIN_ALPHA", "PREDICT", "PREDICT_STEPS", "NO_YLDS", "Y_MODE", "ROW_CAP", "WGS_PER_CU",
                                              "RESORT", "NO_TABLE", "WIDE")}
    assert {c["CVO_HIP_Y_MODE"] for c in tc.CONFIGS if "CVO_HIP_Y_MODE" in c} == {0, 2}
    assert {c["CVO_HIP_ROW_CAP"] for c in tc.CONFIGS if "CVO_HIP_ROW_CAP" in c} == {8, 16}
    assert len({tc.config_id(c) for c in tc.CONFIGS + tc.CHILD_CONFIGS}) == 42
    assert max(n for _, n in tc.PAIRS) == tc.NM_MAX == tc.NF_MAX


def test_list_capacity_of_each_configuration():
    assert tc.capn(dict(wgs=1)) == 512 and tc.capn(dict(CVO_HIP_ROW_CAP=8)) == 8 and tc.capn(dict(CVO_HIP_ROW_CAP=16)) == 16
    assert tc.capn(dict(CVO_HIP_ROW_CAP=1)) == 8 and tc.capn(dict(), 3000) == 1024 and tc.capn(dict(), 100) == 64


def test_the_alignment_ends_where_the_model_takes_its_ell(oracle):
    """a converged launch leaves ell at the end of the schedule and the warm rounds keep it; a launch cut at three iterations never leaves the first ell"""
    for pair in tc.PAIRS:
        full = tc.oracle_rounds(oracle, pair)
        assert [r["ell"] for r in full] == [np.float32(0.03)] * tc.ROUNDS
        assert 20 < full[0]["iter"] < tc.DEFAULT_MAX_ITER - 1               # stopped by its own tests, after the last change of ell (iteration 20)
        assert [r["ell"] for r in tc.oracle_rounds(oracle, pair, 3)] == [np.float32(0.15)] * tc.ROUNDS


def test_every_launch_of_the_matrix_is_on_one_side_of_the_inn_pre_model(oracle):
    sides = set()
    for cfg in tc.CONFIGS + tc.CHILD_CONFIGS:
        for pair in tc.PAIRS:
            for rnd, r in enumerate(tc.oracle_rounds(oracle, pair, tc.max_iter(cfg))):
                side = tc.pre_class(tc.small_pair(*pair), r["ell"], tc.capn(cfg))
                assert side is not None, (cfg, pair, rnd)
                sides.add((tc.capn(cfg), float(r["ell"]), pair, side))
    # both sides occur, and only the cut launch under ROW_CAP=8 declines: its two larger pairs, not its 300-point pair
    assert {s[:3] for s in sides if not s[3]} == {(8, float(np.float32(0.15)), tc.PAIRS[0]), (8, float(np.float32(0.15)), tc.PAIRS[1])}
    assert (8, float(np.float32(0.15)), tc.PAIRS[2], True) in sides and (8, float(np.float32(0.03)), tc.PAIRS[0], True) in sides


def test_neighbour_counts_of_the_900_point_pair():
    """what the two ROW_CAP=8 launches rest on: r_c = 10.0 cm at ell 0.15, where 227 fixed rows hold more than 8 moving points and the fullest 14; the fullest
    holds 10 at ell 0.10, 6 at 0.06 and 3 at 0.03 (the default sp_thres = 8e-3, sigma = 0.1: r_c = 0.668 ell).  The same counts at 1.01 r_c: no row is near
    the edge of either class."""
    c = tc.small_pair(*tc.PAIRS[0])
    assert np.sqrt(tc.r_c2(0.15)) == pytest.approx(0.1002, abs=1e-4)
    n15 = tc.row_counts(c, 0.15)
    assert int((n15 > 8).sum()) == 227 and int(n15.max()) == 14
    assert [int(tc.row_counts(c, e).max()) for e in (0.10, 0.06, 0.03)] == [10, 6, 3]
    assert [int(tc.row_counts(c, e, 1.01).max()) for e in (0.15, 0.10, 0.06, 0.03)] == [14, 10, 6, 3]
    # the count is the plain one: a brute-force loop over a few rows
    fx, mx = c[0].astype(np.float64), c[2].astype(np.float64)
    for i in (0, 17, 450, 899):
        assert n15[i] == sum(1 for j in range(mx.shape[0]) if ((fx[i] - mx[j]) ** 2).sum() < tc.r_c2(0.15))


def test_the_table_model_evicts_slot_three():
    t = tc.SelfTable()
    assert [t.ask(e) for e in tc.ELL_ORDER[:4]] == [False] * 4 and t.slots == [tc.E1, tc.E2, tc.E3, tc.E4]
    assert not t.ask(tc.E5) and t.slots == [tc.E1, tc.E2, tc.E3, tc.E5]          # no slot free: the last one is overwritten
    assert not t.ask(tc.E4) and t.slots[3] == tc.E4 and not t.hit(tc.E5)          # asking e4 again evicts e5
    assert not t.ask(tc.E5) and t.ask(tc.E1) and t.slots[0] == tc.E1               # e1 stayed resident
    assert not t.ask(tc.E6) and not t.ask(tc.E5)
    u = tc.SelfTable()
    assert tuple(u.ask(e) for e in tc.ELL_ORDER) == tc.ELL_HITS
    assert len(set(tc.ELL_ORDER)) == 6 > tc.SELF_CACHE_N
    u.clear()
    assert u.slots == [None] * 4 and not u.hit(tc.E1)
    assert t.hit(np.float32(0.15)) and not t.hit(np.nextafter(np.float32(0.15), np.float32(1)))      # an equal ell, not a near one


def test_tail_round_fills_what_it_declines():
    """round 0 on fresh clouds answers no self product, every later round at the same ell both; a shared table is asked once"""
    tabs = (tc.SelfTable(), tc.SelfTable())
    assert [tc.tail_round(tabs, tc.E4) for _ in range(3)] == [0, tc.FIXED | tc.MOVING, tc.FIXED | tc.MOVING]
    assert tc.tail_round(tabs, tc.E1) == 0 and tc.tail_round((tabs[0], tc.SelfTable()), tc.E1) == tc.FIXED
    # two pairs of one launch on one fixed cloud at two ells: the workgroups look up before anything is filled, and the one score launch that answers the
    # misses lets only its first request keep the shared table
    shared, m0, m1 = tc.SelfTable(), tc.SelfTable(), tc.SelfTable()
    seen = [tc.tail_launch([(shared, m0), (shared, m1)], (tc.E1, tc.E2)) for _ in range(3)]
    assert seen == [[0, 0], [tc.FIXED | tc.MOVING, tc.MOVING], [tc.FIXED | tc.MOVING] * 2] and shared.slots[:2] == [tc.E1, tc.E2]


def test_a_self_product_depends_strongly_on_ell(oracle):
    """a stale table entry shows: between any two length scales of the order the self product of the table pair's clouds differs by more than 1 %, a thousand
    times the tolerance against the oracle"""
    c = tc.small_pair(*tc.TABLE_PAIR)
    o = oracle.OracleCvo(); o.set_pcd(c[0], c[1]); o.set_pcd(c[2], c[3])
    st = o.get_state()
    vals = {}
    for e in sorted(set(tc.ELL_ORDER)):
        o.set_state(st["R"], st["T"], float(e))
        got = [o.function_inner_product(s, None, s) for s in (oracle.SLOT_FIXED, oracle.SLOT_MOVING)]
        assert all(rc == 0 for rc, _ in got)
        vals[e] = tuple(v[0] for _, v in got)
    es = sorted(vals)
    for a, b in zip(es, es[1:]):
        for q in range(2):
            assert abs(vals[a][q] - vals[b][q]) > 1e-2 * abs(vals[b][q]), (a, b, q, vals[a], vals[b])


def test_the_other_inputs_have_the_shapes_the_tests_are_there_for():
    from cvo_slam_amd import synth
    assert len(tc.QUEUE_PAIRS) == 13 and tc.QUEUE_PAIRS[5] == (905, 310)
    assert all(cap // g < len(tc.QUEUE_PAIRS) for g, cap in tc.QUEUE_LAUNCHES)          # fewer pair slots than pairs: a workgroup runs several pairs, several tails
    assert len(tc.FLIGHT_PAIRS) == 4 and all(len(b) == 8 and 500 <= min(n for _, n in b) and max(n for _, n in b) <= 900 for b in tc.FLIGHT_PAIRS)
    assert len({p for b in tc.FLIGHT_PAIRS for p in b}) == 32
    p = synth.make_small_pair(*tc.QUEUE_PAIRS[0][:1], n=tc.QUEUE_PAIRS[0][1])
    np.testing.assert_array_equal(p.fixed.xyz, tc.small_pair(*tc.QUEUE_PAIRS[0])[0])
