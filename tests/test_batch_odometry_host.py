"""The host side of replaying many sequences at once (cvo_slam_amd/replay.py: plan_replay, group_by_size; scripts/replay_sequences.py's
list file): which sequence is in which slot at which step, without a GPU."""
import importlib.util
import os

import pytest

from conftest import ROOT


def frames_seen(plan, n_seq):
    seen = {i: [] for i in range(n_seq)}
    for st in plan:
        for p, i, f in st["advance"]:
            seen[i].append((st["step"], p, f))
    return seen


def test_every_frame_once_in_order_on_one_slot():
    lengths = [6, 4, 1, 5, 3, 6]
    plan = plan_of(lengths, 6)
    seen = frames_seen(plan, len(lengths))
    for i, n in enumerate(lengths):
        assert [f for _, _, f in seen[i]] == list(range(n))
        assert len({p for _, p, _ in seen[i]}) == 1                    # a sequence stays in its slot
        steps = [s for s, _, _ in seen[i]]
        assert steps == list(range(steps[0], steps[0] + n))            # one frame per step, no gaps
    assert [st["step"] for st in plan] == list(range(6))
    for st in plan:
        assert st["align"] == [a for a in st["advance"] if a[2] >= 1]  # frame 0 only fills the fixed cloud
        assert not st["resets"]
        assert len({p for p, _, _ in st["advance"]}) == len(st["advance"])


def test_late_starts_and_slot_reuse():
    lengths, starts = [6, 4, 1, 5, 3, 6], [0, 0, 0, 2, 0, 0]
    plan = plan_of(lengths, 3, starts)
    seen = frames_seen(plan, len(lengths))
    assert seen[3][0][0] >= 2                                          # not before its start
    assert seen[2] == [(0, 2, 0)]                                      # a single frame: one step, nothing aligned
    assert seen[4][0][:2] == (1, 2)                                    # takes slot 2 as soon as sequence 2 has left it (sequence 3 may not start yet)
    assert plan[1]["resets"] == [2]
    for st in plan:
        assert len(st["advance"]) <= 3
    # every slot is reset exactly when a new sequence follows another on it
    owner = {}
    for st in plan:
        for p, i, f in st["advance"]:
            if f == 0:
                assert (p in st["resets"]) == (p in owner)
            owner[p] = i
    assert sum(len(st["align"]) for st in plan) == sum(n - 1 for n in lengths)


def test_a_late_start_leaves_steps_out_and_empty_sequences_are_skipped():
    plan = plan_of([2, 0, 2], 1, [3, 0, 0])
    assert [(st["step"], st["advance"]) for st in plan] == [(0, [(0, 2, 0)]), (1, [(0, 2, 1)]), (3, [(0, 0, 0)]), (4, [(0, 0, 1)])]
    assert plan[2]["resets"] == [0]
    with pytest.raises(ValueError):
        plan_of([1, 2], 0)
    with pytest.raises(ValueError):
        plan_of([1, 2], 2, [0])


def test_grouping_by_image_size():
    from cvo_slam_amd.replay import group_by_size
    size = {0: (480, 640), 1: (456, 736), 2: (480, 640), 3: (456, 736), 4: (100, 100)}
    items = [(p, p, 0) for p in range(5)]
    groups = group_by_size(items, lambda a: size[a[1]])
    assert groups == [[items[0], items[2]], [items[1], items[3]], [items[4]]]
    assert group_by_size([], lambda a: 0) == []


def plan_of(lengths, n_slots, starts=None):
    from cvo_slam_amd.replay import plan_replay
    return plan_replay(lengths, n_slots, starts)


def _script():
    spec = importlib.util.spec_from_file_location("replay_sequences", os.path.join(ROOT, "scripts", "replay_sequences.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_list_file_parsing(tmp_path):
    mod = _script()
    lst = tmp_path / "seqs.txt"
    lst.write_text("# folder assoc calib [out]\n\n"
                   "data/fr1_desk  data/fr1_desk/assoc.txt  cfg/TUM1.yaml\n"
                   "/abs/eth  /abs/eth/assoc.txt  /abs/eth/calib.yaml  out/eth_traj.txt  # trailing comment\n")
    entries = mod.read_list(str(lst), out_dir=str(tmp_path / "trajs"))
    base = str(tmp_path)
    assert entries[0] == (os.path.join(base, "data/fr1_desk"), os.path.join(base, "data/fr1_desk/assoc.txt"), os.path.join(base, "cfg/TUM1.yaml"),
                          os.path.join(str(tmp_path / "trajs"), "fr1_desk.txt"))
    assert entries[1] == ("/abs/eth", "/abs/eth/assoc.txt", "/abs/eth/calib.yaml", os.path.join(base, "out/eth_traj.txt"))
    bad = tmp_path / "bad.txt"
    bad.write_text("only two\n")
    with pytest.raises(ValueError):
        mod.read_list(str(bad))
