"""The tracker streams on the host (no GPU): `keyframe_roles` -- which frame the keyframe object holds in which slot after every decision --
against the oracle's state machine, and the reset_initial arithmetic that the host entry point and the device's link kernel share
(cvo_slam_amd/csrc/cvo_math.hpp) built alone with g++ and compared bit for bit with the oracle's orc_reset_initial."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import tracks_cases

CSRC = os.path.join(ROOT, "cvo_slam_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "cvo_hip.h")
FIXED, MOVING, PREVIOUS = 0, 1, 2

PATTERNS = {
    "all accepted": [True] * 5,
    "rejected at the first phase-2 frame": [False, True, True, False],
    "A R A R R A": [True, False, True, False, False, True],
    "all rejected": [False] * 4,
}


def tiny_cloud(frame):
    """frame + 2 coincident points with equal features: fip(cloud, cloud) counts (frame + 2)^2 pairs, which names the frame"""
    n = frame + 2
    xyz = np.tile(np.array([[0.1, -0.2, 1.0]], np.float32), (n, 1))
    feat = np.tile(np.array([[10.0], [20.0], [30.0], [1.0], [2.0]], np.float32), (1, n))
    return xyz, feat


def oracle_slots(o):
    """the frame held in the oracle object's (fixed, moving, previous) slots, None for an empty slot"""
    out = []
    for slot in (FIXED, MOVING, PREVIOUS):
        rc, r = o.function_inner_product(slot, None, slot)
        if rc != 0:
            out.append(None); continue
        n = int(round(np.sqrt(r[1])))
        assert n * n == r[1] and n >= 2, r
        out.append(n - 2)
    return tuple(out)


@pytest.mark.parametrize("name", list(PATTERNS))
def test_keyframe_roles_follow_the_oracle_state_machine(oracle, name):
    from cvo_slam_amd import replay
    decisions = PATTERNS[name]
    roles = replay.keyframe_roles(decisions)
    assert len(roles) == len(decisions) + 2
    o = oracle.OracleCvo()
    eye = np.eye(3, 4, dtype=np.float32)
    o.set_pcd(*tiny_cloud(0))                                        # local_tracker.cpp:231
    assert oracle_slots(o) == roles[0] == (0, None, None)
    assert oracle_slots(o) == roles[1]                               # the second frame is not shown to the keyframe object (:233, :330-333)
    for j, d in enumerate(decisions):
        f = j + 2
        o.set_pcd(*tiny_cloud(f))                                    # match_keyframe's set_pcd (:415)
        assert oracle_slots(o)[MOVING] == f
        if d:
            o.update_previous_pcd()                                  # :506
        else:
            o.reset_keyframe(eye)                                    # :337 via :518, cvo.cpp:591-604
        assert oracle_slots(o) == roles[f], (name, f, oracle_slots(o), roles[f])


def test_both_reset_keyframe_branches_occur():
    """cvo.cpp:593-601: a rejection while no frame has been accepted or rejected-with-a-previous-cloud yet, and one after."""
    from cvo_slam_amd import replay
    seen = set()
    for decisions in PATTERNS.values():
        pre = False
        for j, d in enumerate(decisions):
            before = replay.keyframe_roles(decisions[:j])[-1]
            after = replay.keyframe_roles(decisions[:j + 1])[-1]
            if d:
                pre = True
                assert after == (before[0], None, j + 2)
            elif before[2] is None:
                seen.add("no frame accepted yet"); assert not pre
                assert after == (j + 2, None, None)                 # the frame itself becomes the fixed cloud; no previous cloud yet
            else:
                seen.add("otherwise"); pre = True
                assert after == (before[2], None, j + 2)
    assert seen == {"no frame accepted yet", "otherwise"}
    assert replay.keyframe_roles([False, None, True])[-2:] == [(2, None, None), (2, None, 4)]   # a frame the object does not see changes nothing


WRAP = r"""
#include "cvo_math.hpp"
extern "C" void many_reset_initial(int n, const float* tr, const float* od, float* R, float* T, float* inv) {
    for (int i = 0; i < n; ++i) cvohip::reset_initial_eval(tr + 12 * i, od + 12 * i, R + 9 * i, T + 3 * i, inv + 12 * i);
}
"""


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("tracks")
    src, so = d / "wrap.cpp", d / "libresetinitial.so"
    src.write_text(WRAP)
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-fPIC", "-shared", "-I" + CSRC, str(src), "-o", str(so)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = C.CDLL(str(so))
    fp = C.POINTER(C.c_float)
    L.many_reset_initial.argtypes = [C.c_int, fp, fp, fp, fp, fp]
    return L


def test_shared_reset_initial_equals_the_oracle_bit_for_bit(host_lib, oracle):
    tr, od = tracks_cases.reset_initial_cases()
    n = tr.shape[0]
    assert n >= 100_000
    R = np.zeros((n, 3, 3), np.float32); T = np.zeros((n, 3), np.float32); inv = np.zeros((n, 3, 4), np.float32)
    fp = C.POINTER(C.c_float)
    host_lib.many_reset_initial(n, *[a.ctypes.data_as(fp) for a in (tr, od, R, T, inv)])
    wR, wT, winv = tracks_cases.oracle_reset_initial(oracle, tr, od)
    for got, want, what in ((R, wR, "R"), (T, wT, "T"), (inv, winv, "init.inverse()")):
        bad = np.nonzero((tracks_cases.bits(got) != tracks_cases.bits(want)).reshape(n, -1).any(axis=1))[0]
        assert bad.size == 0, (what, bad.size, bad[:5])              # expected mismatches: 0 (the same restated sequence)
    assert np.all(np.isfinite(R)) and np.all(np.isfinite(inv))
    # the cases are what they claim: linear parts orthogonal only to float rounding, rotations up to pi, translations of metres
    prod = np.einsum("nij,nkj->nik", tr[:, :, :3].astype(np.float64), tr[:, :, :3].astype(np.float64))
    dev = np.abs(prod - np.eye(3)).max(axis=(1, 2))
    assert 0 < dev.max() < 1e-5 and np.count_nonzero(dev) > n // 2
    ang = np.arccos(np.clip((np.trace(tr[:, :, :3], axis1=1, axis2=2) - 1) / 2, -1, 1))
    assert ang.max() > 3.0 and np.abs(tr[:, :, 3]).max() > 3.0
    # R is the orthogonal factor and T the translation of (transform * odometry)^-1
    assert np.abs(np.einsum("nij,nkj->nik", R.astype(np.float64), R.astype(np.float64)) - np.eye(3)).max() < 1e-6


def test_header_declares_the_tracks():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("cvo_tracks_create", "cvo_tracks_destroy", "cvo_tracks_set_num_want", "cvo_tracks_set_arith_mode", "cvo_tracks_reset", "cvo_tracks_step_async",
                 "cvo_tracks_done", "cvo_tracks_wait", "cvo_tracks_commit", "cvo_tracks_get_cloud", "cvo_tracks_get_selected_points", "cvo_tracks_get_state",
                 "cvo_selftest_reset_initial"):
        assert re.search(r"int\s+" + name + r"\s*\(", src), name
    from cvo_slam_amd import api
    assert set(n for n in api.ABI_SYMBOLS if n.startswith("cvo_tracks_")) == set(re.findall(r"\b(cvo_tracks_[a-z_]+)\s*\(", src))
    # cvo_track_step as the Python mirror lays it out: the fields the header lists, in its order
    body = re.search(r"typedef struct cvo_track_step \{(.*?)\} cvo_track_step;", src, flags=re.S).group(1)
    fields = re.findall(r"\b(\w+)(?:\[\d+\])?;", body)
    assert fields == [f[0] for f in api.TrackStep._fields_]


def test_track_step_layout_matches_the_c_compiler(tmp_path):
    from cvo_slam_amd import api
    src = tmp_path / "layout.c"
    names = [f[0] for f in api.TrackStep._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cvo_hip.h"\nint main(void) { printf("%zu", sizeof(cvo_track_step));\n' +
                   "".join(f'printf(" %zu", offsetof(cvo_track_step, {n}));\n' for n in names) + "return 0; }\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(api.TrackStep)] + [getattr(api.TrackStep, n).offset for n in names]


def test_tracks_need_a_device(hiplib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(hiplib.CvoError) as e:
        hiplib.CvoTracks(4)
    assert e.value.code == 5                                         # CVO_ERR_NO_DEVICE
    from cvo_slam_amd import api
    with pytest.raises(hiplib.CvoError) as e:
        api.selftest_reset_initial(np.eye(3, 4)[None], np.eye(3, 4)[None])
    assert e.value.code == 5


def test_plan_and_poses_of_the_tracker_replay():
    """the host side of replay_tracker(_many): poses chained without an optimiser, from recorded steps"""
    from cvo_slam_amd import replay

    def tf(x):
        t = np.eye(3, 4, dtype=np.float32); t[0, 3] = x; return t
    ok = lambda x: dict(status=0, transform=tf(x))
    none = dict(status=1)
    steps = [dict(odometry=none, keyframe=none), dict(odometry=ok(1), keyframe=none), dict(odometry=ok(1), keyframe=ok(2.5)),
             dict(odometry=ok(1), keyframe=ok(9)), dict(odometry=ok(1), keyframe=ok(2.25)), dict(odometry=dict(status=2), keyframe=none),
             dict(odometry=ok(1), keyframe=dict(status=6))]
    poses = replay._tracker_poses(steps, [None, None, True, False, True, None, True])
    # frame 2 accepted: keyframe 0 x 2.5; frame 3 rejected: previous x 1, keyframe = frame 2; frame 4 accepted: pose(2) x 2.25;
    # frame 5 failed: repeats; frame 6 accepted but its keyframe alignment failed: previous x odometry
    assert [p[0, 3] for p in poses] == [0, 1, 2.5, 3.5, 4.75, 4.75, 5.75]


def test_cpp_mirror_has_the_tracks(tmp_path, hiplib):
    """cvo_hip.hpp's CvoTracks compiles with a plain C++11 compiler, links against the library, and fails loudly without a device"""
    src = tmp_path / "use_tracks.cpp"
    src.write_text('#include "cvo_hip.hpp"\n#include <cstdio>\n'
                   "int main() { try { cvo_hip::CvoTracks t(4); int s[1] = {0}, a[1] = {1}; t.commit(1, s, a); t.reset(0); (void)t.done(); }\n"
                   '  catch (const std::exception& e) { std::printf("%s\\n", e.what()); return 3; } return 0; }\n')
    exe = str(tmp_path / "use_tracks")
    libdir = os.path.dirname(hiplib.lib_path())
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", exe, f"-L{libdir}", "-lcvo_hip", f"-Wl,-rpath,{libdir}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 3 and "cvo_tracks_create" in r.stdout
