"""Queue classes of the batch streams on the host (no GPU): the two pure functions of cvo_slam_amd/csrc/cvo_queue_classes.hpp built
alone with g++ -- which class the dealer gives the next engine, and what a launch can count on (concurrent / deferred) from the
launches in flight per class.  The header has no HIP includes; the library's host code calls the same functions."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "cvo_slam_amd", "csrc")

WRAP = r"""
#include "cvo_queue_classes.hpp"
static_assert(cvo_qc::CLASSES == 2, "two classes");
extern "C" int choose_class(const int* live, int Q, int dealt, int second_class) { return cvo_qc::choose_class(live, Q, dealt != 0, second_class != 0); }
extern "C" void launch_share(const int* inflight, int mine, int Q, int* concurrent, int* deferred) {
    bool d = false; cvo_qc::launch_share(inflight, mine, Q, concurrent, &d); *deferred = d ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def qc(tmp_path_factory):
    d = tmp_path_factory.mktemp("qc")
    src, so = d / "wrap.cpp", d / "libqc.so"
    src.write_text(WRAP)
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I" + CSRC, str(src), "-o", str(so)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = C.CDLL(str(so))
    ip = C.POINTER(C.c_int)
    L.choose_class.argtypes = [ip, C.c_int, C.c_int, C.c_int]; L.choose_class.restype = C.c_int
    L.launch_share.argtypes = [ip, C.c_int, C.c_int, ip, ip]; L.launch_share.restype = None
    return L


def test_header_has_no_hip_includes():
    src = open(os.path.join(CSRC, "cvo_queue_classes.hpp")).read()
    assert "#include" not in src.replace("#pragma once", "")


class Dealer:
    """the bookkeeping Engine::make_stream / Engine::forget keep around choose_class"""
    def __init__(self, L, Q, second=True):
        self.L, self.Q, self.second, self.live = L, Q, second, [0, 0]

    def take(self, dealt=True):
        c = self.L.choose_class((C.c_int * 2)(*self.live), self.Q, int(dealt), int(self.second))
        self.live[c] += 1
        return c

    def give_back(self, c):
        self.live[c] -= 1


def test_dealing_at_four_queues(qc):
    d = Dealer(qc, 4)
    assert [d.take() for _ in range(10)] == [0, 0, 0, 0, 1, 1, 1, 1, 0, 1]
    assert d.live == [5, 5]


def test_a_released_class0_place_is_dealt_next(qc):
    d = Dealer(qc, 4)
    got = [d.take() for _ in range(6)]
    assert got == [0, 0, 0, 0, 1, 1]
    d.give_back(0)
    assert d.take() == 0 and d.take() == 1
    # all of class 0 released: the next Q are class 0 again, class 1 keeps what it has
    for _ in range(4):
        d.give_back(0)
    assert [d.take() for _ in range(4)] == [0, 0, 0, 0] and d.live == [4, 3]


def test_an_engine_that_is_not_dealt_is_class0_and_counted(qc):
    d = Dealer(qc, 4)
    assert [d.take(dealt=False) for _ in range(6)] == [0] * 6 and d.live == [6, 0]
    assert d.take() == 1                                      # class 0 is full of handles: the first batch goes to class 1
    d2 = Dealer(qc, 4)
    assert [d2.take(dealt=(i != 1)) for i in range(6)] == [0, 0, 0, 0, 1, 1]
    assert d2.take(dealt=False) == 0 and d2.live == [5, 2]


def test_no_level_below_normal_means_class0(qc):
    d = Dealer(qc, 4, second=False)
    assert [d.take() for _ in range(12)] == [0] * 12 and d.live == [12, 0]


def _share(L, inflight, mine, Q):
    c, d = C.c_int(-1), C.c_int(-1)
    L.launch_share((C.c_int * 2)(*inflight), mine, Q, C.byref(c), C.byref(d))
    return c.value, bool(d.value)


@pytest.mark.parametrize("Q", [1, 2, 4, 8])
def test_one_class_in_use_is_the_single_class_rule(qc, Q):
    for inflight in range(0, 20):
        want = (min(Q, inflight + 1), inflight >= Q)
        assert _share(qc, [inflight, 0], 0, Q) == want
        assert _share(qc, [0, inflight], 1, Q) == want


@pytest.mark.parametrize("inflight, mine, Q, concurrent, deferred", [
    ((4, 3), 1, 4, 8, False),        # the eighth of eight streams at four queues: a full device, a queue of its own
    ((4, 4), 1, 4, 8, True),         # a ninth launch: behind one of its class
    ((4, 4), 0, 4, 8, True),
    ((3, 4), 0, 4, 8, False),
    ((4, 0), 1, 4, 5, False),        # class 0 full, the first of class 1
    ((6, 1), 1, 4, 6, False),        # class 0 over its queues counts Q
    ((6, 1), 0, 4, 5, True),
    ((2, 1), 0, 2, 3, True),         # Q = 2 with 2 + 1
    ((2, 1), 1, 2, 4, False),
    ((0, 0), 0, 4, 1, False),
    ((0, 0), 1, 4, 1, False),
])
def test_two_classes(qc, inflight, mine, Q, concurrent, deferred):
    assert _share(qc, list(inflight), mine, Q) == (concurrent, deferred)
