"""Point matches on the host (no GPU): the five entry points are declared in include/cvo_hip.h, exported by the library and bound by the
Python mirror; the mirror's records have the header's layout; Cvo, CvoBatch and CvoTracks have point_matches; and cvo_slam_amd.matches
(fitness, rmse, mutual, residuals) does the right thing on an example worked by hand."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "cvo_hip.h")
SYMBOLS = ["cvo_point_matches", "cvo_batch_point_matches", "cvo_batch_point_matches_device", "cvo_tracks_point_matches", "cvo_tracks_point_matches_device"]


def test_symbols_are_declared_exported_and_bound(hiplib):
    from cvo_slam_amd import api
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    L = hiplib.load_library()
    exported = set(re.findall(r" T (cvo_[a-zA-Z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", hiplib.lib_path()], text=True)))
    vp, ip, fp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)
    dst = C.POINTER(api.PointMatchesDst)
    want = {"cvo_point_matches": [vp, C.c_int, fp, C.c_int, dst, C.c_int, C.c_int],
            "cvo_batch_point_matches": [vp, C.c_int, ip, dst], "cvo_batch_point_matches_device": [vp, C.c_int, ip, dst, vp],
            "cvo_tracks_point_matches": [vp, C.c_int, C.c_int, ip, dst], "cvo_tracks_point_matches_device": [vp, C.c_int, C.c_int, ip, dst, vp]}
    for name in SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name + " is not declared"
        assert len(m.group(1).split(",")) == len(want[name]), name
        assert name in api.ABI_SYMBOLS and name in exported, name
        assert list(getattr(L, name).argtypes) == want[name], name
    for cls in (api.Cvo, api.CvoBatch, api.CvoTracks):
        assert callable(getattr(cls, "point_matches")), cls.__name__


def test_records_have_the_headers_fields():
    from cvo_slam_amd import api
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct cvo_point_matches_dst \{(.*?)\} cvo_point_matches_dst;", src, flags=re.S).group(1)
    assert re.findall(r"\b(\w+)\s*;", body) == [f[0] for f in api.PointMatchesDst._fields_]
    assert C.sizeof(api.PointMatchesDst) == 11 * C.sizeof(C.c_void_p)
    body = re.search(r"typedef struct cvo_match_fit \{(.*?)\} cvo_match_fit;", src, flags=re.S).group(1)
    assert re.findall(r"\b(\w+)\s*;", body) == [f[0] for f in api.MatchFit._fields_] == list(api._MATCH_FIT_DTYPE.names)
    assert C.sizeof(api.MatchFit) == api._MATCH_FIT_DTYPE.itemsize == 24
    assert [api.MatchFit.sum_w.offset, api.MatchFit.sum_w_res2.offset] == [8, 16]
    raw = np.zeros(2, api._MATCH_FIT_DTYPE); raw[0] = (5, 3, 0.5, 2e-4); raw[1] = (4, 0, 0.0, 0.0)
    fm, ff = api.match_fit_records(raw.view(np.uint8))
    assert fm == dict(rows=5, matched=3, sum_w=0.5, sum_w_res2=2e-4) and ff == dict(rows=4, matched=0, sum_w=0.0, sum_w_res2=0.0)


def test_summaries_on_an_example_worked_by_hand():
    from cvo_slam_amd import api, matches
    fit = dict(rows=8, matched=6, sum_w=0.5, sum_w_res2=0.5 * 0.01 ** 2)
    assert matches.fitness(fit) == 0.75
    assert matches.rmse(fit) == pytest.approx(0.01, rel=1e-12)
    assert matches.fitness(api.MatchFit(8, 6, 0.5, 5e-5)) == 0.75 and matches.rmse(api.MatchFit(8, 6, 0.5, 5e-5)) == pytest.approx(0.01, rel=1e-12)
    empty = dict(rows=8, matched=0, sum_w=0.0, sum_w_res2=0.0)
    assert matches.fitness(empty) == 0.0 and math.isnan(matches.rmse(empty))
    assert matches.fitness(dict(rows=0, matched=0, sum_w=0.0, sum_w_res2=0.0)) == 0.0
    # moving 0 <-> fixed 2 and moving 3 <-> fixed 0 choose each other; moving 1 wants fixed 2, which prefers moving 0; moving 2 has no partner;
    # fixed 1 wants moving 3, which prefers fixed 0; fixed 3 has no partner
    best_moving = np.array([2, 2, -1, 0], np.int32); best_fixed = np.array([3, 3, 0, -1], np.int32)
    got = matches.mutual(best_moving, best_fixed)
    assert got.tolist() == [[0, 2], [3, 0]]
    assert matches.mutual(np.array([-1, -1], np.int32), np.array([-1], np.int32)).shape == (0, 2)
    with pytest.raises(ValueError):
        matches.mutual(np.array([4], np.int32), best_fixed)
    mean = np.array([[1, 2, 3], [0, 0, 0]], np.float32); pts = np.array([[1, 2, 2.5], [4, 5, 6]], np.float32)
    assert matches.residuals(mean, pts).tolist() == [[0, 0, 0.5], [-4, -5, -6]]
    with pytest.raises(ValueError):
        matches.residuals(mean, pts[:1])
