"""The staged steps on the host (no GPU): the stage entry points are declared in include/cvo_hip.h, exported by the library and bound by the
Python mirror with the header's argument types; and `replay.stage_plan` -- which frames are handed over while a step runs -- stages exactly
what `plan_replay` makes the next step advance."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "cvo_hip.h")
LENGTHS = [6, 4, 1, 5, 3, 6]                                        # the fixture of tests/test_gpu_tracks.py
STAGE_SYMBOLS = ["cvo_batch_stage_images", "cvo_batch_advance_staged", "cvo_batch_staged_count",
                 "cvo_tracks_stage_async", "cvo_tracks_step_staged_async", "cvo_tracks_staged_count"]


def c_to_ctypes(decl, api):
    """one parameter declaration of the header -> the ctypes type the mirror must bind it with"""
    decl = re.sub(r"\s+", " ", decl).strip()
    kind = re.sub(r"\s*\b[a-z_0-9]+$", "", decl).strip()              # drop the parameter's name
    table = {
        "cvo_batch": C.c_void_p, "cvo_tracks": C.c_void_p, "void*": C.c_void_p, "int": C.c_int,
        "const int*": C.POINTER(C.c_int), "int*": C.POINTER(C.c_int), "long long*": C.POINTER(C.c_longlong),
        "const unsigned char* const*": C.POINTER(C.c_void_p), "const unsigned short* const*": C.POINTER(C.c_void_p),
        "const cvo_camera*": C.POINTER(api.Camera),
    }
    return table[kind]


def test_stage_symbols_are_declared_exported_and_bound(hiplib):
    from cvo_slam_amd import api
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    L = hiplib.load_library()
    exported = set(re.findall(r" T (cvo_[a-zA-Z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", hiplib.lib_path()], text=True)))
    for name in STAGE_SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name + " is not declared"
        assert name in api.ABI_SYMBOLS and name in exported, name
        want = [c_to_ctypes(p, api) for p in m.group(1).split(",")]
        assert list(getattr(L, name).argtypes) == want, (name, getattr(L, name).argtypes, want)
    # the stage calls take the arguments of the calls they stage for: advance_images without points_out, step_async without the stream handle
    assert list(L.cvo_batch_stage_images.argtypes) == list(L.cvo_batch_advance_images.argtypes)[:-1]
    assert list(L.cvo_tracks_stage_async.argtypes) == list(L.cvo_tracks_step_async.argtypes)[:-1]
    for cls, names in ((api.CvoBatch, ("stage_images", "advance_staged", "staged_count")),
                       (api.CvoTracks, ("stage_async", "step_staged_async", "step_staged", "staged_count"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls.__name__, n)


def test_stage_plan_is_the_next_steps_list():
    from cvo_slam_amd import replay
    for slots, starts in ((3, None), (4, [0, 0, 0, 2, 0, 0]), (6, None), (1, None)):
        plan = replay.plan_replay(LENGTHS, slots, starts)
        ahead = replay.stage_plan(plan)
        assert len(ahead) == len(plan)
        assert ahead[-1] == []                                      # nothing is staged after the last step
        for j in range(len(plan) - 1):
            assert ahead[j] == plan[j + 1]["advance"], (slots, j)    # what is staged while step j runs is what step j + 1 advances, in its order
            assert ahead[j], (slots, j)
        # every frame but the ones of the first step is staged exactly once, in sequence order
        staged = [(i, f) for lst in ahead for _, i, f in lst]
        first = [(i, f) for _, i, f in plan[0]["advance"]]
        assert sorted(staged + first) == sorted((i, f) for i, n in enumerate(LENGTHS) for f in range(n))
        if slots < len(LENGTHS):                                    # slots are reused: a staged frame 0 belongs to a slot the next step resets
            reused = [(j, p) for j in range(len(plan) - 1) for p in plan[j + 1]["resets"]]
            assert reused
            for j, p in reused:
                assert any(q == p and f == 0 for q, _, f in ahead[j]), (j, p)
    assert replay.stage_plan([]) == []


def test_replay_functions_take_stage_ahead_and_default_to_off():
    import inspect
    from cvo_slam_amd import replay
    for fn in (replay.replay_odometry_many, replay.replay_tracker_many):
        p = inspect.signature(fn).parameters["stage_ahead"]
        assert p.default is False
    for script in ("replay_sequences.py", "replay_tracker_sequences.py"):
        assert "--stage-ahead" in open(os.path.join(ROOT, "scripts", script)).read()
