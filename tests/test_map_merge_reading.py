"""The reading of merging maps (tests/map_merge_reading.py) held to the reading of resident maps (tests/map_reading.py) on the statements the
header makes: a coarse map merged from a fine map's rows is the map the same history builds at the coarser voxel -- every field but born, dead
rows included, in order; with no removals born too; a level-0 union of disjoint stamp sets is the one map of all integrations -- and on its own
rules: the key's shift at the cell edges, the filter, lo and hi, revival, born-dead rows, the refusals.  No GPU: numpy against numpy."""
import numpy as np
import pytest

import map_merge_reading as gr
import map_reading as mr
import map_snapshot_reading as sr

VOXEL = np.float32(0.05)
EXACT = ("key", "count", "mask", "last")


@pytest.fixture(scope="module")
def scene():
    members, poses = mr.sliding_windows(np.random.default_rng(5), members=10, n=3000)
    return members, poses


def history(scene, level, window=4, voxel=VOXEL):
    members, poses = scene
    return gr.window_history(mr.Map(100000, np.float32(np.ldexp(np.float32(voxel), level))), members, poses, window)


@pytest.fixture(scope="module")
def fine(scene):
    M = history(scene, 0)
    assert M.rows == 1953 and M.rows - M.live == 646                    # the scene the statement was first checked on
    return M


def same_but_born(A, B):
    return all(getattr(A, f) == getattr(B, f) for f in EXACT) and A.index == B.index and len(A.sums) == len(B.sums) and all((p == q).all() for p, q in zip(A.sums, B.sums))


@pytest.mark.parametrize("level,rows,neg_x,born_differs", [(1, 573, 285, 14), (2, 160, 80, 9), (3, 60, 30, 6), (4, 16, 8, None)])
def test_a_coarse_merge_is_the_history_at_the_coarser_voxel_but_for_born(scene, fine, level, rows, neg_x, born_differs):
    want = history(scene, level)
    got = gr.coarser(fine, level)
    assert same_but_born(got, want) and got.live == want.live
    assert any(c == 0 for c in got.count) or level == 4                  # dead rows are carried, in their place
    assert got.rows == rows and sum(1 for k in got.key if gr.cell_of(k)[0] < 0) == neg_x   # (negative cells: where a truncating shift would go wrong)
    if born_differs is not None:
        differs = [r for r in range(got.rows) if got.born[r] != want.born[r]]
        assert len(differs) == born_differs and all(got.count[r] >= 1 for r in differs)   # born cannot be rebuilt from rows: a revived child has lost its stamp
    assert all(got.born[r] >= want.born[r] for r in range(got.rows) if got.count[r] >= 1)


def test_with_dead_rows_skipped_the_order_differs(scene, fine):
    want = history(scene, 1)
    got = gr.merge(mr.Map(100000, np.float32(0.1)), fine, 1, all_rows=False, min_views=0)
    assert got.rows == want.live < want.rows and got.key != [k for k, c in zip(want.key, want.count) if c >= 1]
    live = {k: (c, m, l) for k, c, m, l in zip(want.key, want.count, want.mask, want.last) if c >= 1}
    assert {k: (c, m, l) for k, c, m, l in zip(got.key, got.count, got.mask, got.last)} == live


@pytest.mark.parametrize("level", [1, 2, 3, 4])
def test_without_removals_every_field_agrees(scene, level):
    members, poses = scene
    f = gr.window_history(mr.Map(100000, VOXEL), members, poses, window=99)
    want = gr.window_history(mr.Map(100000, np.float32(np.ldexp(VOXEL, level))), members, poses, window=99)
    assert f.live == f.rows and sr.same_map(gr.coarser(f, level), want)


def test_a_level_0_union_of_disjoint_stamps_is_the_one_map(scene):
    members, poses = scene
    A, B, whole = mr.Map(100000, VOXEL), mr.Map(100000, VOXEL), mr.Map(100000, VOXEL)
    for m in range(10):
        (A if m < 5 else B).update([members[m]], [poses[m]], [m])
        whole.update([members[m]], [poses[m]], [m])
    before = sr.snapshot(B)
    assert sr.same_map(gr.merge(A, B, 0), whole)                         # born included: no row of either was ever dead
    assert sr.same_snapshot(sr.snapshot(B), before)                      # the source is only read


def put(M, cell, count=1, mask=1, last=0, born=0, sums=None):
    M.index[gr.key_of(cell)] = M.rows
    M.key.append(gr.key_of(cell)); M.sums.append(np.full(8, count, np.int64) if sums is None else np.asarray(sums, np.int64)); M.count.append(count)
    M.mask.append(mask); M.last.append(last); M.born.append(born)
    return M


def test_the_shift_is_arithmetic_at_the_cell_edges():
    top = (1 << 20) - 1
    for level in range(5):
        for c in (-1, -2, -3, 0, 1, top, -top, -top + 1, 12345, -12345):
            want = int(np.floor(c / 2 ** level))
            assert gr.cell_of(gr.shifted(gr.key_of((c, -c, c)), level)) == (want, int(np.floor(-c / 2 ** level)), want)
            assert sr.key_ok(gr.shifted(gr.key_of((c, c, c)), level))
    assert gr.cell_of(gr.shifted(gr.key_of((-1, -2, -top)), 1)) == (-1, -1, -(1 << 19))
    assert gr.cell_of(gr.shifted(gr.key_of((-1, -2, top)), 4)) == (-1, -1, (1 << 16) - 1)
    # the float side of the claim: floorf(x / (voxel * 2^k)) is the shifted floorf(x / voxel), on both sides of 0
    x = np.random.default_rng(2).uniform(-40, 40, 20000).astype(np.float32)
    x[:4] = [-0.05, -0.1, -1e-30, 0.0]
    fine = np.floor(x / VOXEL).astype(np.int64)
    for level in range(1, 5):
        assert (np.floor(x / np.float32(np.ldexp(VOXEL, level))).astype(np.int64) == fine >> level).all()
    S = put(put(put(put(mr.Map(10, VOXEL), (-1, 0, 0)), (-2, 0, 0)), (top, -top, 0)), (0, 0, 0))
    D = gr.coarser(S, 1)
    assert [gr.cell_of(k) for k in D.key] == [(-1, 0, 0), (top >> 1, -(1 << 19), 0), (0, 0, 0)] and D.count == [2, 1, 1]


def test_lo_hi_mask_revival_and_rows_born_dead():
    S = mr.Map(10, VOXEL)
    put(S, (0, 0, 0), count=0, mask=0, last=9, born=1, sums=np.zeros(8))    # dead, the oldest born
    put(S, (1, 0, 0), count=3, mask=0b0110, last=4, born=5)
    put(S, (1, 1, 1), count=2, mask=0b1000, last=7, born=3)
    put(S, (2, 0, 0), count=0, mask=0, last=2, born=6, sums=np.zeros(8))    # a cell of dead rows alone
    put(S, (3, 1, 0), count=0, mask=0, last=8, born=4, sums=np.zeros(8))
    D = gr.coarser(S, 1)
    assert D.key == [gr.key_of((0, 0, 0)), gr.key_of((1, 0, 0))]
    assert D.count == [5, 0] and D.mask == [0b1110, 0] and D.last == [9, 8] and D.born == [3, 4] and D.live == 1     # lo: among the living; none: among all
    assert D.sums[0].tolist() == [5] * 8
    with_filter = gr.merge(mr.Map(10, np.float32(0.1)), S, 1, all_rows=False, min_views=2)
    assert with_filter.count == [3] and with_filter.born == [5] and with_filter.last == [4]
    # present rows: a dead one is revived by a cell with members and by no other
    T = put(put(mr.Map(10, np.float32(0.1)), (1, 0, 0), count=0, mask=0b1, last=1, born=0, sums=np.zeros(8)), (0, 0, 0), count=1, mask=0b1, last=20, born=2)
    gr.merge(T, S, 1)
    assert T.count == [0, 6] and T.born == [0, 2] and T.last == [8, 20] and T.mask == [1, 0b1111] and T.live == 1
    U = put(mr.Map(10, np.float32(0.1)), (0, 0, 0), count=0, mask=0, last=1, born=0, sums=np.zeros(8))
    gr.merge(U, S, 1)
    assert U.count == [5, 0] and U.born == [3, 4] and U.last == [9, 8]


def test_refusals_leave_the_destination_as_it_was():
    S = put(put(mr.Map(10, VOXEL), (0, 0, 0), count=mr.MAX_COUNT), (1, 0, 0), count=mr.MAX_COUNT)
    with pytest.raises(mr.Refused, match="count"):
        gr.coarser(S, 1)                                                 # two children of 16777215 each
    assert gr.coarser(S, 0).count == [mr.MAX_COUNT] * 2
    D = put(mr.Map(10, VOXEL), (0, 0, 0), count=1)
    before = sr.snapshot(D)
    with pytest.raises(mr.Refused, match="count"):
        gr.merge(D, S, 0)
    assert sr.same_snapshot(sr.snapshot(D), before)
    many = mr.Map(400, VOXEL)
    for j in range(300):                                                 # 300 siblings in one level-4 cell: the sum is above 2^32
        put(many, (j % 16, (j // 16) % 16, j // 256), count=mr.MAX_COUNT)
    assert 300 * mr.MAX_COUNT > 2 ** 32
    with pytest.raises(mr.Refused, match="count"):
        gr.coarser(many, 4)
    tight = put(mr.Map(2, VOXEL), (5, 5, 5))
    with pytest.raises(mr.Refused, match="max_rows"):
        gr.merge(tight, S, 0)
    assert tight.rows == 1 and gr.merge(put(mr.Map(3, VOXEL), (5, 5, 5)), put(put(mr.Map(9, VOXEL), (0, 0, 0)), (1, 0, 0)), 0).rows == 3
    for bad in (lambda: gr.merge(mr.Map(9, np.float32(0.1)), S, 0), lambda: gr.merge(mr.Map(9, VOXEL), S, 1), lambda: gr.merge(mr.Map(9, np.float32(1.6)), S, 5),
                lambda: gr.merge(mr.Map(9, np.float32(0.1000001)), S, 1)):
        with pytest.raises(ValueError):
            bad()
