"""The reading of resident maps (tests/map_reading.py) held to the reading of a fusion (tests/fuse_reading.py) on the consequences the header
states -- one call, any split into calls, removal, compaction -- and on its own rules: stamps past 63, every refusal, drop and new_row.  No
GPU: numpy against numpy."""
import numpy as np
import pytest

import fuse_reading as fr
import map_reading as mr

VOXEL = 0.05
FUSED = ("xyz", "feat", "count", "views", "view_mask")


@pytest.fixture(scope="module")
def window():
    members, poses = mr.sliding_windows(np.random.default_rng(31), members=8, n=1500, stride=0.12)
    assert min(x.shape[0] for x, f in members) > 500
    return members, poses


def integrated(members, poses, stamps, splits, max_rows=100000, voxel=VOXEL):
    M = mr.Map(max_rows, voxel)
    at = 0
    for k in splits:
        M.update(members[at:at + k], poses[at:at + k], stamps[at:at + k]); at += k
    assert at == len(members)
    return M


@pytest.mark.parametrize("min_points,min_views", [(1, 1), (2, 1), (1, 2), (3, 3)])
def test_one_call_is_the_fusion_in_bytes_and_order(window, min_points, min_views):
    members, poses = window
    M = integrated(members, poses, list(range(8)), [8])
    want = fr.fuse_reading(members, poses, VOXEL, fr.MEAN, min_points, min_views)
    got = M.extract(min_points, min_views)
    assert want["n_out"] > 20 and got["n_out"] == want["n_out"] and mr.same_bytes(got, want, FUSED)
    assert got["born"].min() == 0 and (got["last_stamp"] >= got["born"]).all() and (np.diff(got["row"]) > 0).all()


@pytest.mark.parametrize("splits", [[1] * 8, [3, 5], [5, 3], [2, 2, 2, 2], [7, 1]])
def test_any_split_into_consecutive_calls_gives_the_same_bytes(window, splits):
    members, poses = window
    whole = integrated(members, poses, list(range(8)), [8]).extract()
    parts = integrated(members, poses, list(range(8)), splits).extract()
    assert mr.same_bytes(parts, whole)
    assert mr.same_bytes(parts, fr.fuse_reading(members, poses, VOXEL), FUSED)


def test_a_sliding_window_is_the_fusion_of_the_window_as_a_set(window):
    members, poses = window
    M = mr.Map(100000, VOXEL)
    for t in range(8):
        M.update([members[t]], [poses[t]], [t])
        if t >= 3:
            M.update([members[t - 3]], [poses[t - 3]], [t - 3], -1)
        lo = max(0, t - 2)
        want = fr.fuse_reading(members[lo:t + 1], poses[lo:t + 1], VOXEL)
        got = M.extract()
        assert mr.row_set(got) == mr.row_set(want) and got["n_out"] == M.live
        by_row = {got["xyz"][r].tobytes(): int(got["view_mask"][r]) for r in range(got["n_out"])}
        for r in range(want["n_out"]):                                  # the fusion's member m is stamp lo + m: the bits sit at the stamps
            assert by_row[want["xyz"][r].tobytes()] == int(want["view_mask"][r]) << lo
    assert M.rows > M.live                                              # dead rows keep their place
    dead = [r for r in range(M.rows) if M.count[r] == 0]
    assert all((M.sums[r] == 0).all() and M.mask[r] == 0 for r in dead)


def test_a_dead_row_is_revived_with_a_new_born(window):
    members, poses = window
    M = mr.Map(100000, VOXEL)
    M.update([members[0]], [poses[0]], [4]); M.update([members[0]], [poses[0]], [4], -1)
    assert M.live == 0 and M.rows > 0 and M.extract()["n_out"] == 0
    M.update([members[0]], [poses[0]], [9])
    e = M.extract()
    assert e["n_out"] == M.rows and (e["born"] == 9).all() and (e["last_stamp"] == 9).all() and (e["view_mask"] == np.uint64(1 << 9)).all()


def test_stamps_past_63_wrap_onto_the_low_bits(window):
    members, poses = window
    M = integrated(members[:3], poses[:3], [64, 65, 130], [3])
    e = M.extract()
    assert int(np.bitwise_or.reduce(e["view_mask"])) == 0b111 and e["last_stamp"].max() == 130 and e["born"].min() == 64   # 64 -> bit 0, 130 -> bit 2
    both = integrated([members[0], members[0]], [poses[0], poses[0]], [0, 64], [2]).extract(min_views=1)
    assert (both["views"] == 1).all() and (both["view_mask"] == np.uint64(1)).all() and (both["last_stamp"] == 64).all()
    assert integrated([members[0], members[0]], [poses[0], poses[0]], [0, 64], [2]).extract(min_views=2)["n_out"] == 0


def test_every_refusal_leaves_the_map_as_it_was(window):
    members, poses = window
    need = integrated(members[:2], poses[:2], [0, 1], [2]).rows
    M = integrated(members[:1], poses[:1], [0], [1], max_rows=need - 1)
    before = M.extract()
    with pytest.raises(mr.Refused, match="max_rows"):
        M.update([members[1]], [poses[1]], [1])
    with pytest.raises(mr.Refused, match="absent"):
        M.update([members[1]], [poses[1]], [1], -1)
    with pytest.raises(mr.Refused, match="more members"):
        M.update([members[0], members[0]], [poses[0], poses[0]], [0, 0], -1)
    assert mr.same_bytes(M.extract(), before) and M.rows == before["n_out"]
    exact = integrated(members[:2], poses[:2], [0, 1], [1, 1], max_rows=need)
    assert exact.rows == need
    one = (np.full((1000, 3), 0.5, np.float32), np.ones((1000, 5), np.float32))
    C = mr.Map(1, 64.0)
    C.count, C.key, C.sums, C.mask, C.last, C.born = [mr.MAX_COUNT - 1000], [int(mr.call_cells([one], [np.eye(4)], 64.0)[0][0])], [np.zeros(8, np.int64)], [1], [0], [0]
    C.index = {C.key[0]: 0}
    C.update([one], [np.eye(4)], [1])
    assert C.count[0] == mr.MAX_COUNT
    with pytest.raises(mr.Refused, match="16777215"):
        C.update([(one[0][:1], one[1][:1])], [np.eye(4)], [2])
    assert C.count[0] == mr.MAX_COUNT and C.rows == 1


def test_compaction_keeps_order_and_drops_by_every_clause(window):
    members, poses = window
    M = integrated(members[:4], poses[:4], [0, 1, 2, 3], [1, 1, 1, 1])
    M.update([members[0]], [poses[0]], [0], -1)
    before = M.extract()
    old_rows, dead = M.rows, M.rows - M.live
    assert dead > 0
    new_row = M.compact()                                               # the defaults drop the dead rows alone
    assert M.rows == old_rows - dead == M.live and (new_row >= 0).sum() == M.rows
    after = M.extract()
    assert mr.same_bytes(after, before, mr.OUTPUTS[:-1]) and np.array_equal(new_row[before["row"]], after["row"])
    M.update([members[0]], [poses[0]], [0])                             # the rebuilt table still finds every cell
    assert mr.row_set(M.extract()) == mr.row_set(fr.fuse_reading(members[:4], poses[:4], VOXEL))
    e = M.extract()
    one_view = e["views"] == 1
    assert one_view.sum() > 10 and (~one_view).sum() > 10
    drop = np.zeros(M.rows, np.uint8); drop[e["row"][~one_view][:5]] = 1
    stays = ((e["views"] >= 2) | (e["born"] >= 2)) & (e["last_stamp"] >= 1) & (drop[e["row"]] == 0)
    new_row = M.compact(min_last_stamp=1, min_views=2, probation_from=2, drop=drop)
    assert 0 < stays.sum() < e["n_out"] and M.rows == stays.sum()
    assert np.array_equal(new_row >= 0, stays) and np.array_equal(new_row[stays], np.arange(M.rows))
    assert mr.same_bytes(M.extract(), {k: e[k][stays] for k in mr.OUTPUTS[:-1]} | dict(n_out=int(stays.sum())), mr.OUTPUTS[:-1])


# ---- compactions that drop live rows, and the removal that goes with them (sign -2)
def carving_loop(members, poses, K, steps, step_done=None):
    """the tracker loop of INTEGRATION.md on the reading: integrate keyframe t, remove keyframe t - K (what is still there), and a compaction
    that drops LIVE rows: a drop mask over every seventh extracted row, and one-view cells past a probation of one step"""
    M = mr.Map(100000, VOXEL)
    for t in range(steps):
        M.update([members[t]], [poses[t]], [t])
        if t >= K:
            M.update([members[t - K]], [poses[t - K]], [t - K], -2)
        e = M.extract(min_views=2)
        drop = np.zeros(M.rows, np.uint8); drop[e["row"][::7]] = 1
        M.compact(min_views=2, probation_from=t - 1, drop=drop)
        if step_done:
            step_done(t, M)
    return M


def test_the_loop_with_carving_and_probation_runs_past_the_window(window):
    members, poses = window
    K = 3
    cells = [mr.call_cells([m], [p], VOXEL) for m, p in zip(members, poses)]      # each member's own cells: keys, sums, counts
    skipped = []

    def holds_its_members(t, M):
        """every row is the sum of the window's members whose stamp bit it carries -- and of nothing else"""
        assert M.rows == M.live > 0
        want = {}
        for s in range(max(0, t - K + 1), t + 1):
            keys, sums, counts, _ = cells[s]
            for k, q, c in zip(keys.tolist(), sums, counts.tolist()):
                r = M.index.get(k, -1)
                if r >= 0 and M.mask[r] >> s & 1:
                    a = want.setdefault(r, [np.zeros(8, np.int64), 0]); a[0] = a[0] + q; a[1] += c
                else:
                    skipped.append((t, s))
        assert sorted(want) == list(range(M.rows))
        for r, (q, c) in want.items():
            assert M.count[r] == c and (M.sums[r] == q).all(), (t, r)

    M = carving_loop(members, poses, K, 8, holds_its_members)
    assert len(skipped) > 50 and {t for t, s in skipped} >= set(range(1, 8))       # members' points were dropped at every step, and the loop went on
    assert M.extract(min_views=2)["n_out"] > 50


def test_plain_removal_after_a_live_dropping_compaction_is_refused_or_wrong_and_sign_minus_2_is_neither(window):
    members, poses = window
    M = integrated(members[:2], poses[:2], [0, 1], [1, 1])
    e = M.extract()
    shared = e["views"] == 2
    assert shared.sum() > 20
    drop = np.zeros(M.rows, np.uint8); drop[e["row"][shared][:10]] = 1              # ten cells that both members hold, carved
    gone = [M.key[r] for r in e["row"][shared][:10]]
    M.compact(drop=drop)
    with pytest.raises(mr.Refused, match="absent"):
        M.update([members[0]], [poses[0]], [0], -1)
    M.update([members[2]], [poses[2]], [2])                                         # member 2 makes some of the carved cells again
    again = [k for k in gone if k in M.index]
    assert again, "the scene must re-create a carved cell"
    before = {k: (M.count[M.index[k]], M.sums[M.index[k]].copy(), M.mask[M.index[k]]) for k in again}
    M.update([members[0]], [poses[0]], [0], -2)                                     # skips the carved cells, re-created or not
    for k in again:
        r = M.index[k]
        assert (M.count[r], M.mask[r]) == (before[k][0], before[k][2]) and (M.sums[r] == before[k][1]).all() and M.mask[r] == 1 << 2
    assert mr.row_set(M.extract(min_views=1)) != [] and all(not (m & 1) for m in M.mask)
    rest = {k: r for k, r in M.index.items() if k not in gone}
    want = integrated(members[1:3], poses[1:3], [1, 2], [1, 1])                      # elsewhere: the fusion of members 1 and 2
    for k, r in rest.items():
        if M.count[r]:
            w = want.index[k]
            assert M.count[r] == want.count[w] and (M.sums[r] == want.sums[w]).all()
    # a group that is partly present in a row refuses
    P = integrated(members[:1], poses[:1], [0], [1])
    with pytest.raises(mr.Refused, match="partly"):
        P.update(members[:2], poses[:2], [0, 1], -2)
