"""The reading of saving and restoring maps (tests/map_snapshot_reading.py) held to the reading of resident maps: restore(snapshot(M)) is M field
for field, a twin made that way goes on like the original through every later call, and each of the five refusal kinds is raised by an input
that breaks that rule alone.  No GPU: numpy against numpy."""
import numpy as np
import pytest

import map_reading as mr
import map_snapshot_reading as sr

VOXEL = 0.05


@pytest.fixture(scope="module")
def window():
    return mr.sliding_windows(np.random.default_rng(47), members=8, n=1200, stride=0.12)


def history(members, poses, upto):
    """integrations, removals, a revived row and (from step 6 on) a compaction that drops live rows"""
    M = mr.Map(100000, VOXEL)
    for t in range(upto):
        M.update([members[t]], [poses[t]], [t])
        if t == 2:                                                      # member 0 goes out and comes back under a new stamp: its rows are revived
            M.update([members[0]], [poses[0]], [0], -1)
            assert M.live < M.rows
            M.update([members[0]], [poses[0]], [40])
        if t >= 4:
            M.update([members[t - 3]], [poses[t - 3]], [t - 3], -2)
        if t == 5:
            e = M.extract(min_views=2)
            drop = np.zeros(M.rows, np.uint8); drop[e["row"][::5]] = 1
            assert drop.sum() > 5
            M.compact(min_views=2, probation_from=4, drop=drop)
    return M


@pytest.mark.parametrize("upto", [0, 1, 3, 5, 6, 8])
def test_restore_of_a_snapshot_is_the_map_field_for_field(window, upto):
    members, poses = window
    M = history(members, poses, upto)
    S = sr.snapshot(M)
    assert S["keys"].shape == (M.rows,) and S["sums"].shape == (M.rows, 8) and S["keys"].dtype == np.uint64 and S["count"].dtype == np.uint32
    if upto in (5, 8):
        assert (S["count"] == 0).any()                                  # dead rows are in the snapshot, in their place
    T = sr.restore(S, M.rows, VOXEL)                                    # (rows exactly max_rows)
    assert sr.same_map(T, M) and T.live == M.live and sr.same_snapshot(sr.snapshot(T), S)
    with pytest.raises(ValueError, match="max_rows"):
        sr.restore(S, M.rows - 1, VOXEL) if M.rows else sr.restore(dict(S, keys=np.ones(1, np.uint64)), 0, VOXEL)


def test_a_twin_goes_on_like_the_original(window):
    members, poses = window
    M = history(members, poses, 5)
    T = sr.restore(sr.snapshot(M), 100000, VOXEL)
    dead_before = [r for r in range(M.rows) if M.count[r] == 0]
    assert dead_before

    def both(call):
        a, b = call(M), call(T)
        assert sr.same_map(M, T)
        return a, b

    both(lambda X: X.update([members[5], members[0]], [poses[5], poses[0]], [5, 41]))     # adds to old rows, revives dead ones, bears new ones
    assert any(M.count[r] > 0 for r in dead_before) and M.rows > len(dead_before)
    both(lambda X: X.update([members[2]], [poses[2]], [2], -2))
    for flt in (dict(), dict(min_points=3), dict(min_views=2), dict(min_last_stamp=5)):
        a, b = both(lambda X: X.extract(**flt))
        assert a["n_out"] > 0 and mr.same_bytes(a, b)
    e = M.extract()
    drop = np.zeros(M.rows, np.uint8); drop[e["row"][::4]] = 1
    a, b = both(lambda X: X.compact(min_views=2, probation_from=5, drop=drop))
    assert np.array_equal(a, b) and (a < 0).sum() > drop.sum() > 0
    both(lambda X: X.update([members[6]], [poses[6]], [6]))
    assert sr.same_snapshot(sr.snapshot(M), sr.snapshot(T))


def good(n=6):
    keys = np.array([(1048576 + x) << 42 | (1048576 - x) << 21 | (1 + x) for x in range(n)], np.uint64)
    count = np.arange(n, dtype=np.uint32)                              # (row 0 is dead: eight zero sums)
    sums = (np.arange(8, dtype=np.int64)[None, :] - 3) * count.astype(np.int64)[:, None] * 1000
    return dict(keys=keys, sums=sums, count=count, view_mask=np.arange(n, dtype=np.uint64), last_stamp=np.arange(n, dtype=np.int32) + 3,
                born=np.arange(n, dtype=np.int32))


def broken(field, row, value, col=None):
    S = {k: v.copy() for k, v in good().items()}
    if col is None:
        S[field][row] = value
    else:
        S[field][row, col] = value
    return S


CASES = [
    ("bit 63", sr.BAD_KEY, broken("keys", 2, np.uint64(1 << 63 | 5 << 42 | 5 << 21 | 5))),
    ("all ones", sr.BAD_KEY, broken("keys", 5, np.uint64(2 ** 64 - 1))),
    ("x field 0", sr.BAD_KEY, broken("keys", 1, np.uint64(7 << 21 | 7))),
    ("y field 0", sr.BAD_KEY, broken("keys", 1, np.uint64(7 << 42 | 7))),
    ("z field 0", sr.BAD_KEY, broken("keys", 0, np.uint64(7 << 42 | 7 << 21))),
    # a count above the bound with sums that stay inside ITS bound: the count rule alone
    ("count", sr.BAD_COUNT, broken("count", 3, np.uint32(mr.MAX_COUNT + 1))),
    ("count 2^32 - 1", sr.BAD_COUNT, broken("count", 3, np.uint32(2 ** 32 - 1))),
    ("last_stamp", sr.BAD_STAMP, broken("last_stamp", 4, -1)),
    ("born", sr.BAD_STAMP, broken("born", 0, np.int32(-2 ** 31))),
    ("sum above", sr.BAD_SUM, broken("sums", 2, 2 * sr.SUM_BOUND + 1, col=7)),
    ("sum below", sr.BAD_SUM, broken("sums", 5, -5 * sr.SUM_BOUND - 1, col=0)),
    ("int64 min", sr.BAD_SUM, broken("sums", 1, np.int64(-2 ** 63), col=3)),
    ("a sum in a dead row", sr.BAD_SUM, broken("sums", 0, 1, col=4)),
    ("duplicate neighbours", sr.DUPLICATE, broken("keys", 3, good()["keys"][2])),
    ("duplicate of a dead row", sr.DUPLICATE, broken("keys", 5, good()["keys"][0])),
]


def test_the_good_rows_and_the_bounds_themselves_are_accepted():
    M = sr.restore(good(), 6, VOXEL)
    assert M.rows == 6 and M.live == 5 and M.index[int(good()["keys"][4])] == 4
    at = {k: v.copy() for k, v in good().items()}
    at["count"][3] = mr.MAX_COUNT; at["sums"][3, 0] = mr.MAX_COUNT * sr.SUM_BOUND; at["sums"][3, 1] = -mr.MAX_COUNT * sr.SUM_BOUND
    at["keys"][1] = np.uint64((2 ** 21 - 1) << 42 | 1 << 21 | (2 ** 21 - 1)); at["last_stamp"][2] = 2 ** 31 - 1; at["born"][2] = 0
    assert sr.refusal_bits(at) == 0 and mr.MAX_COUNT * sr.SUM_BOUND < 2 ** 63
    assert sr.restore({k: v[:0] for k, v in good().items()}, 1, VOXEL).rows == 0


@pytest.mark.parametrize("name,bit,arrays", CASES, ids=[c[0] for c in CASES])
def test_each_refusal_kind_is_raised_by_an_input_that_breaks_that_rule_alone(name, bit, arrays):
    assert sr.refusal_bits(arrays) == bit
    with pytest.raises(sr.Refused) as e:
        sr.restore(arrays, 100, VOXEL)
    assert e.value.bits == bit and isinstance(e.value, mr.Refused)


def test_two_kinds_in_one_map_give_both_bits():
    S = broken("keys", 3, good()["keys"][2]); S["last_stamp"][5] = -7
    assert sr.refusal_bits(S) == sr.DUPLICATE | sr.BAD_STAMP
    S = broken("count", 3, np.uint32(mr.MAX_COUNT + 1)); S["sums"][1, 1] = sr.SUM_BOUND + 1
    assert sr.refusal_bits(S) == sr.BAD_COUNT | sr.BAD_SUM
