"""The engineered clouds of tests/table_cases.py have the properties they are built for -- asserted here from a sequential simulation of
insertion with the numpy mirror of the hash, with no GPU.  These are conditions on the cases, not measurements of the kernels: the kernels
are held to the readings on these clouds in tests/test_gpu_table_cases.py, where the mirror itself is held to the device's function."""
import numpy as np
import pytest

import fuse_reading as fr
import table_cases as tc
import voxel_reading as vr


def sim(case, slots=None):
    ok, key = tc.keys_of(case["xyz"])
    return ok, key, tc.simulate(key, ok, case["slots"] if slots is None else slots)


def test_the_mirror_on_known_values():
    """the hash by python integers, apart from numpy's uint64: the same slots"""
    def by_hand(k, slots):
        m = (1 << 64) - 1
        h = k & m
        h ^= h >> 33; h = (h * 0xff51afd7ed558ccd) & m; h ^= h >> 33; h = (h * 0xc4ceb9fe1a85ec53) & m; h ^= h >> 33
        return ((h >> 32) * slots) >> 32
    rng = np.random.default_rng(5)
    keys = np.concatenate([rng.integers(0, 2 ** 63, 2000), [0, 1, 2 ** 63 - 1, (2 ** 21 - 1) << 42, 1 << 20]]).astype(np.int64)
    for slots in (1, 2, 6, 128, 130, 514, 2097150, 2 ** 32 - 1):
        got = tc.home_slot(keys, slots)
        assert got.tolist() == [by_hand(int(k), slots) for k in keys.tolist()]
        assert got.min() >= 0 and got.max() < slots
    assert len(np.unique(tc.home_slot(keys, 2097150))) > 2000                  # (it spreads)


@pytest.mark.parametrize("n", tc.SIZES)
def test_every_point_is_in_its_cell_at_its_home(n):
    for case in (tc.last_slot(n), tc.one_slot_twice(n), tc.staircase(n)):
        ok, c, key = vr.cells(vr.points8(case["xyz"], case["feat"]), tc.VOXEL)
        assert case["xyz"].shape == (n, 3) and case["slots"] == 2 * n and ok.all(), case["name"]
        assert np.array_equal(c.astype(np.int64), case["cells"]), case["name"]
        assert np.array_equal(tc.home_slot(key, 2 * n), case["homes"]), case["name"]
        assert not (case["xyz"] == 0).any()                                    # (no -0.0 for a pose to turn into +0.0)


@pytest.mark.parametrize("n", tc.SIZES)
def test_last_slot_wraps_every_insert_but_one(n):
    case = tc.last_slot(n)
    ok, key, s = sim(case)
    assert len(np.unique(key)) == n and (s["home"] == 2 * n - 1).all() and s["fresh"].all()
    assert int((s["wraps"] == 1).sum()) >= n - 1 and s["wraps"].max() <= 1
    assert int(s["distance"].max()) == n - 1                                   # the chain is n long
    assert tc.chain_order(s["table"], 2 * n - 1) == [2 * n - 1] + list(range(n - 1))


@pytest.mark.parametrize("n", tc.SIZES)
def test_one_slot_twice_finds_its_keys_deep_in_the_chain(n):
    case = tc.one_slot_twice(n)
    ok, key, s = sim(case)
    m = (n + 1) // 2
    assert len(np.unique(key)) == m and np.array_equal(key[m:], key[:n - m]) and (s["home"] == n).all()   # (slot n: the middle of 2 n)
    assert s["fresh"][:m].all() and not s["fresh"][m:].any()                   # the second occurrences are finds
    assert np.array_equal(s["slot"][m:], s["slot"][:n - m])
    if n > m:
        probes = s["distance"][m:] + 1                                         # slots looked at: the distance walked and the one that matches
        assert probes.mean() >= n / 4, (n, probes.mean())
    if n > 64:
        assert m >= 64                                                         # a second occurrence is at least a wave behind its first
    assert n == 1 or not np.array_equal(case["xyz"][m:], case["xyz"][:n - m])  # (another point of the same cell)


@pytest.mark.parametrize("n", tc.SIZES)
def test_staircase_merges_clusters_across_the_wrap(n):
    case = tc.staircase(n)
    ok, key, s = sim(case)
    homes = case["homes"]
    assert len(np.unique(key)) == n and s["fresh"].all()
    assert np.array_equal(homes, (homes[0] + np.arange(n) // 2) % (2 * n))     # h, h, h + 1, h + 1, ...
    assert int(s["distance"].max()) >= n // 2                                  # cell i lands i - i // 2 slots behind its home
    if n >= 2:                                                                 # (one cell alone cannot leave its home)
        assert int(s["wraps"].sum()) >= 1
    if n >= 3:
        assert homes.max() == 2 * n - 1 and homes.min() == 0                   # the homes themselves go on across the wrap
    occupied = np.flatnonzero(s["table"] >= 0)
    assert occupied.shape[0] == n and len(tc.chain_order(s["table"], int(homes[0]))) == n    # one merged cluster


def test_runs_has_the_stated_lengths_at_the_stated_lanes():
    case = tc.runs()
    ok, key = tc.keys_of(case["xyz"])
    n = case["xyz"].shape[0]
    assert n == 327 and n > 256                                                # two blocks; a last partial wave of 7
    got = tc.lane_run_lengths(key, ok)
    assert [[(length) for _, length, _ in w] for w in got[:4]] == [[1, 2, 3, 5, 8, 13, 31, 1], [64], [63, 1], [64]]
    assert got[2][0][:2] == (0, 63) and got[2][1][:2] == (63, 1)               # a run ends at lane 62, a run of 1 starts at lane 63
    assert got[3][0][2] == got[4][0][2] and got[4][0][:2] == (0, 1)            # the run of 65 goes on for one lane of the next wave
    assert [length for _, length, _ in got[4]] == [1, 4, 3, 5, 3, 1, 3, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, 28]
    assert [length for _, length, _ in got[5]] == [2, 1, 3, 1] and sum(length for _, length, _ in got[5]) == 7
    assert got[4][-1][2] == got[5][0][2]                                       # the run of 28 goes on in the partial wave
    w4 = [k for _, _, k in got[4]]
    assert w4[1] == w4[3] != w4[2]                                             # A B A
    assert w4[4] == w4[6] and w4[5] is None                                    # an invalid point inside a run
    assert w4[8] is None and got[4][8][1] == 2 and w4[7] != w4[9]              # invalid points between runs
    assert w4[10] == w4[12] == got[0][0][2] and w4[11] == got[1][0][2]         # cells of waves 0 and 1 come back
    assert w4[13] == w4[15] and w4[14] == w4[16] and w4[13] != w4[14]          # A B A B
    assert int((~ok).sum()) == 4
    # the prescription itself: every valid point's cell is its id's, distinct ids are distinct cells
    by_id = {}
    for i, c in enumerate(case["ids"]):
        assert ok[i] == (c is not None)
        if c is not None:
            assert by_id.setdefault(c, int(key[i])) == int(key[i])
    assert len(set(by_id.values())) == len(by_id) == 21
    red = vr.reduce_reading(case["xyz"], case["feat"], tc.VOXEL)
    assert red["n_out"] == 21 and red["count"].tolist()[:12] == [1 + 4, 2, 3, 5, 8, 13, 31, 1, 64 + 2, 63, 1, 65]   # (cells 0 and 8 come back)
    assert (red["count"] == 1).sum() >= 2


def test_homed_serves_any_table_and_avoids_cells():
    first = tc.last_slot(64, slots=400)
    more = tc.last_slot(64, slots=400, avoid=first["cells"])
    both = {tuple(c) for c in first["cells"].tolist()} | {tuple(c) for c in more["cells"].tolist()}
    assert len(both) == 128
    for case in (first, more):
        ok, key = tc.keys_of(case["xyz"])
        assert ok.all() and (tc.home_slot(key, 400) == 399).all()
    assert first["slots"] == 400 and np.array_equal(tc.last_slot(64, slots=400)["cells"], first["cells"])    # the same every time


@pytest.mark.parametrize("parts", [2, 3])
def test_split_members_move_back_onto_the_case(parts):
    for case in tc.all_cases():
        members, poses = tc.split(case, parts)
        xyz, feat, member, offsets = fr.moved_concat(members, poses)
        assert xyz.tobytes() == case["xyz"].tobytes() and feat.tobytes() == case["feat"].tobytes(), case["name"]
        assert len(members) == min(parts, case["xyz"].shape[0])
    # cells are shared between members where a case has a cell twice
    case = tc.one_slot_twice(257)
    members, poses = tc.split(case, 2)
    assert fr.fuse_reading(members, poses, tc.VOXEL)["views"].max() == 2
