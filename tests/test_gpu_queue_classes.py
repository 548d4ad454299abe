"""Queue classes of batch streams (cvo_batch_queue_class): with Q hardware queues per stream priority the
first Q batch objects alive on a device take the normal priority, the next Q the least one, and their launches return exactly what
one object alone returns.  A class-1 object that plans a launch with more than one workgroup per pair moves to class 0 first.
Q is read from GPU_MAX_HW_QUEUES (4 when unset), as the library reads it; nothing here sets it.

The dealer counts every engine stream the library has made in the process, and a process that has run other tests keeps a few alive (the
image generator's own handle per thread, for one).  So the exact order "Q times class 0, Q times class 1, then class 0" is asserted in a
fresh child process, where the counts start at zero; in this process the same order is asserted from the first free class-0 place on:
k <= Q objects of class 0, then Q of class 1."""
import gc
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

ADOPT_GMAX = 4
N_PAIRS = 8


def _q():
    try:
        v = int(os.environ.get("GPU_MAX_HW_QUEUES", "0"))
    except ValueError:
        v = 0
    return v if v > 0 else 4


def _capacity():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count       # one 512-thread workgroup per CU


def _batch(hiplib, pairs, adoption, workgroups=1):
    b = hiplib.CvoBatch(len(pairs))
    b.set_workgroups(workgroups)
    b.set_adoption(adoption)
    for i, p in enumerate(pairs):
        b.set_pair(i, p.fixed.xyz, p.fixed.feat, p.moving.xyz, p.moving.feat)
    return b


def _same(want, got):
    assert len(got) == len(want)
    for w, g in zip(want, got):
        assert g["status"] == 0 and g["iter"] == w["iter"] and g["iterations_run"] == w["iterations_run"] and g["A_nonzero"] == w["A_nonzero"]
        assert np.array_equal(g["transform"], w["transform"])


@pytest.fixture(scope="module")
def pairs():
    from cvo_slam_amd import synth
    return [synth.make_small_pair(500 + i, n=300) for i in range(N_PAIRS)]


@pytest.fixture(scope="module")
def want(hiplib, pairs):
    """the 8 pairs on one object alone, adoption off"""
    ref = _batch(hiplib, pairs, False)
    ref.align_async(len(pairs)); w = ref.wait(len(pairs))
    ref.close()
    return w


@pytest.fixture()
def no_live_objects(want):
    gc.collect()                                              # objects of earlier tests that nobody holds any more give their places back


def _leading_class0(classes, Q):
    """k: the class-0 places that were free; the objects after them must be Q of class 1"""
    k = 0
    while k < len(classes) and classes[k] == 0 and k < Q:
        k += 1
    assert classes[:k + Q] == ([0] * k + [1] * Q)[:len(classes)], classes
    return k


def test_two_classes_in_flight_change_no_result(hiplib, pairs, want, no_live_objects):
    Q, n, cap = _q(), len(pairs), _capacity()
    bs = [_batch(hiplib, pairs, True) for _ in range(2 * Q + 1)]
    try:
        classes = [b.queue_class() for b in bs]
        assert all(lim == Q for _, lim in classes), classes
        before = [c for c, _ in classes]
        k = _leading_class0(before, Q)
        if k >= 1:                                            # class 0 held exactly Q after them, class 1 holds Q now: the tie goes to class 0, then class 1 has fewer
            assert before[k + Q:] == ([0, 1] * Q)[:len(before) - k - Q], classes
        for rnd in range(3):
            for b in bs:
                b.reset_states(); b.align_async(n)
            for b in bs:
                _same(want, b.wait(n))
                info = b.last_launch()
                assert 1 <= info["concurrent"] <= 2 * Q, info
                if cap // info["concurrent"] > n:
                    assert info["grid"] == min(cap // info["concurrent"], ADOPT_GMAX * n) and info["helpers"] == info["grid"] - n, info
                else:
                    assert info["grid"] == n and info["helpers"] == 0, info
        assert [b.queue_class()[0] for b in bs] == before     # launches of one workgroup per pair move nobody
    finally:
        for b in bs: b.close()


def test_cooperating_workgroups_leave_the_second_class(hiplib, pairs, want, no_live_objects):
    Q, n = _q(), len(pairs)
    fill = []
    while len(fill) < Q:                                      # take the free class-0 places: the next object is class 1
        f = hiplib.CvoBatch(1)
        if f.queue_class()[0] == 1:
            f.close(); break
        fill.append(f)
    b = _batch(hiplib, pairs, False, workgroups=2)
    try:
        assert b.queue_class()[0] == 1
        b.align_async(n); _same(want, b.wait(n))
        assert b.queue_class()[0] == 0
        b.set_workgroups(1)
        b.reset_states(); b.align_async(n); _same(want, b.wait(n))
        assert b.queue_class()[0] == 0
        later = hiplib.CvoBatch(1)                            # class 0 now holds more than Q, class 1 none
        assert later.queue_class()[0] == 1
        later.close()
    finally:
        b.close()
        for f in fill: f.close()


def test_places_given_back_are_dealt_again(hiplib, no_live_objects):
    Q = _q()
    bs = [hiplib.CvoBatch(1) for _ in range(2 * Q)]
    try:
        k = _leading_class0([b.queue_class()[0] for b in bs], Q)
        for b in bs[:k]: b.close()
        fresh = [hiplib.CvoBatch(1) for _ in range(k)]
        bs += fresh
        assert [b.queue_class()[0] for b in fresh] == [0] * k
    finally:
        for b in bs: b.close()


CHILD = r"""
import json, sys
import torch  # noqa: F401  (first: one HIP runtime per process, tests/conftest.py)
sys.path.insert(0, sys.argv[1])
import cvo_slam_amd as ca
from cvo_slam_amd import synth
Q, n = int(sys.argv[2]), int(sys.argv[3])
pairs = [synth.make_small_pair(500 + i, n=300) for i in range(n)]
bs = []
for _ in range(2 * Q + 1):
    b = ca.CvoBatch(n); b.set_workgroups(1); b.set_adoption(True)
    for i, p in enumerate(pairs):
        b.set_pair(i, p.fixed.xyz, p.fixed.feat, p.moving.xyz, p.moving.feat)
    bs.append(b)
out = {"classes": [b.queue_class()[0] for b in bs], "results": []}
for b in bs:
    b.align_async(n)
for b in bs:
    out["results"].append([[r["status"], r["iter"], r["iterations_run"], r["A_nonzero"], r["transform"].astype("float32").tobytes().hex()] for r in b.wait(n)])
    out.setdefault("concurrent", []).append(b.last_launch()["concurrent"])
for b in bs:
    b.close()
print(json.dumps(out))
"""


def _child(env, Q, n):
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(Q), str(n)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def _child_results_equal(out, want, n):
    for got in out["results"]:
        assert len(got) == n
        for w, g in zip(want, got):
            assert g[:4] == [0, w["iter"], w["iterations_run"], w["A_nonzero"]]
            assert g[4] == np.asarray(w["transform"], np.float32).tobytes().hex()


def test_fresh_process_deals_class0_then_class1(hiplib, pairs, want):
    """counts that start at zero: the first Q objects are class 0, the next Q class 1, the tie after them goes to class 0"""
    Q, n = _q(), len(pairs)
    out = _child({k: v for k, v in os.environ.items() if k != "CVO_HIP_QUEUE_CLASSES"}, Q, n)
    assert out["classes"] == [0] * Q + [1] * Q + [0]
    assert all(1 <= c <= 2 * Q for c in out["concurrent"]), out["concurrent"]
    _child_results_equal(out, want, n)


def test_knob_zero_keeps_every_stream_normal(hiplib, pairs, want):
    """CVO_HIP_QUEUE_CLASSES is read at first use: a fresh child process."""
    Q, n = _q(), len(pairs)
    out = _child(dict(os.environ, CVO_HIP_QUEUE_CLASSES="0"), Q, n)
    assert out["classes"] == [0] * (2 * Q + 1)
    assert all(1 <= c <= Q for c in out["concurrent"]), out["concurrent"]      # one class: never more than Q side by side
    _child_results_equal(out, want, n)
