"""The host side of device-resident point clouds (cvo_device_cloud): the ABI names, the descriptor the python wrapper makes from the shape
and strides of two __cuda_array_interface__ carriers, and what it refuses before any library call.  No GPU: the carriers are fakes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvo_check_device_clouds", "cvo_batch_set_pairs_device_clouds", "cvo_batch_advance_device_clouds",
       "cvo_tracks_step_device_clouds_async", "cvo_selftest_ingest_clouds"]


class Fake:
    """what a device tensor shows of itself: __cuda_array_interface__ (version 2: strides None when C-contiguous) and .shape"""
    def __init__(self, shape, typestr, ptr, strides=None):
        self.shape = tuple(shape)
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(ptr, False), strides=strides, version=2)


def test_header_and_python_mirror_name_the_new_symbols():
    from cvo_slam_amd import api
    src = open(os.path.join(ROOT, "include", "cvo_hip.h")).read()
    assert "typedef struct cvo_device_cloud" in src
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in api.ABI_SYMBOLS, name
    assert [f for f, _ in api.DeviceCloud._fields_] == ["xyz", "feat", "xyz_stride", "feat_point_stride", "feat_channel_stride", "n", "pad_"]
    assert C.sizeof(api.DeviceCloud) == 48
    # the struct in the header has the same members in the same order
    body = re.search(r"typedef struct cvo_device_cloud \{(.*?)\} cvo_device_cloud;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == [f for f, _ in api.DeviceCloud._fields_]


def fields(d):
    return (d.xyz, d.feat, d.xyz_stride, d.feat_point_stride, d.feat_channel_stride, d.n)


def test_descriptor_from_shape_and_strides():
    from cvo_slam_amd.api import device_cloud
    n = 700
    # tight: the reference layout
    d = device_cloud(Fake((n, 3), "<f4", 0x1000), Fake((5, n), "<f4", 0x9000))
    assert fields(d) == (0x1000, 0x9000, 12, 4, 4 * n, n)
    # row-strided xyz: columns 2..4 of an (n, 8) tensor
    d = device_cloud(Fake((n, 3), "<f4", 0x1008, (32, 4)), Fake((5, n), "<f4", 0x9000))
    assert fields(d) == (0x1008, 0x9000, 32, 4, 4 * n, n)
    # float4 points
    d = device_cloud(Fake((n, 3), "<f4", 0x1000, (16, 4)), Fake((5, n), "<f4", 0x9004))
    assert fields(d) == (0x1000, 0x9004, 16, 4, 4 * n, n)
    # points-first features
    d = device_cloud(Fake((n, 3), "<f4", 0x1000), Fake((n, 5), "<f4", 0x9000))
    assert fields(d) == (0x1000, 0x9000, 12, 20, 4, n)
    # channels first with a padded channel stride (rows of a (5, n + 3) tensor)
    d = device_cloud(Fake((n, 3), "<f4", 0x1000), Fake((5, n), "<f4", 0x9000, (4 * (n + 3), 4)))
    assert fields(d) == (0x1000, 0x9000, 12, 4, 4 * (n + 3), n)
    # every second point of a channels-first tensor
    d = device_cloud(Fake((n, 3), "<f4", 0x1000, (24, 4)), Fake((5, n), "<f4", 0x9000, (8 * n, 8)))
    assert fields(d) == (0x1000, 0x9000, 24, 8, 8 * n, n)
    # an empty cloud needs no pointers
    d = device_cloud(Fake((0, 3), "<f4", 0), Fake((5, 0), "<f4", 0))
    assert fields(d) == (None, None, 0, 0, 0, 0)


def test_five_by_five_needs_a_layout():
    from cvo_slam_amd.api import device_cloud
    x, f = Fake((5, 3), "<f4", 0x1000), Fake((5, 5), "<f4", 0x9000)
    with pytest.raises(ValueError, match="feat_layout"):
        device_cloud(x, f)
    assert fields(device_cloud(x, f, "channels_first")) == (0x1000, 0x9000, 12, 4, 20, 5)
    assert fields(device_cloud(x, f, "points_first")) == (0x1000, 0x9000, 12, 20, 4, 5)
    with pytest.raises(ValueError):
        device_cloud(x, f, "rows")
    # a stated layout is checked against the shape like an inferred one
    with pytest.raises(ValueError):
        device_cloud(Fake((7, 3), "<f4", 0x1000), Fake((5, 7), "<f4", 0x9000), "points_first")


@pytest.mark.parametrize("xyz,feat", [
    (Fake((70, 3), "<f8", 4), Fake((5, 70), "<f4", 8)),                             # double positions
    (Fake((70, 3), "<f4", 4), Fake((5, 70), "<f2", 8)),                             # half features
    (Fake((70, 3), "<f4", 4), Fake((5, 70), ">f4", 8)),                             # big-endian
    (Fake((70, 3), "<i4", 4), Fake((5, 70), "<f4", 8)),                             # integers
    (Fake((210,), "<f4", 4), Fake((5, 70), "<f4", 8)),                              # flat positions
    (Fake((70, 4), "<f4", 4), Fake((5, 70), "<f4", 8)),                             # four columns: slice them
    (Fake((70, 3), "<f4", 4), Fake((350,), "<f4", 8)),                              # flat features
    (Fake((70, 3), "<f4", 4), Fake((1, 5, 70), "<f4", 8)),                          # rank 3
    (Fake((70, 3), "<f4", 4), Fake((4, 70), "<f4", 8)),                             # four channels
    (Fake((70, 3), "<f4", 4), Fake((5, 71), "<f4", 8)),                             # point counts differ
    (Fake((70, 3), "<f4", 4), Fake((69, 5), "<f4", 8)),
    (Fake((70, 3), "<f4", 4, (-12, 4)), Fake((5, 70), "<f4", 8)),                   # flipped
    (Fake((70, 3), "<f4", 4), Fake((5, 70), "<f4", 8, (280, -4))),
    (Fake((70, 3), "<f4", 4), Fake((5, 70), "<f4", 8, (-280, 4))),
    (Fake((70, 3), "<f4", 4, (14, 4)), Fake((5, 70), "<f4", 8)),                    # row stride not a multiple of 4
    (Fake((70, 3), "<f4", 4, (8, 4)), Fake((5, 70), "<f4", 8)),                     # rows overlap: below 12 bytes
    (Fake((70, 3), "<f4", 4, (12, 8)), Fake((5, 70), "<f4", 8)),                    # every second coordinate
    (Fake((70, 3), "<f4", 4), Fake((5, 70), "<f4", 8, (282, 4))),                   # channel stride not a multiple of 4
    (Fake((70, 3), "<f4", 4), Fake((70, 5), "<f4", 8, (22, 4))),                    # point stride not a multiple of 4
    (Fake((70, 3), "<f4", 4), Fake((5, 70), "<f4", 8, (0, 4))),                     # a broadcast channel
    (Fake((70, 3), "<f4", 6), Fake((5, 70), "<f4", 8)),                             # base not 4-byte aligned
    (Fake((70, 3), "<f4", 4), Fake((5, 70), "<f4", 9)),
    (Fake((70, 3), "<f4", 0), Fake((5, 70), "<f4", 8)),                             # null
    (Fake((70, 3), "<f4", 4), Fake((5, 70), "<f4", 0)),
    (np.zeros((70, 3), np.float32), Fake((5, 70), "<f4", 8)),                       # a host array
    (Fake((70, 3), "<f4", 4), np.zeros((5, 70), np.float32)),
    (Fake((65536, 3), "<f4", 4), Fake((5, 65536), "<f4", 8)),                       # above the 16-bit column indices
])
def test_what_the_wrapper_refuses(xyz, feat):
    from cvo_slam_amd.api import device_cloud
    with pytest.raises(ValueError):
        device_cloud(xyz, feat)


def test_methods_refuse_before_they_touch_the_library():
    from cvo_slam_amd import api
    B = api.CvoBatch.__new__(api.CvoBatch); T = api.CvoTracks.__new__(api.CvoTracks)   # no handle: a library call would fail differently
    good = (Fake((70, 3), "<f4", 4), Fake((5, 70), "<f4", 8))
    host = (np.zeros((70, 3), np.float32), np.zeros((5, 70), np.float32))
    for call in (lambda: B.set_pairs_clouds([good, host], [0], [1]), lambda: B.advance_clouds([0, 1], [good, host]),
                 lambda: T.step_clouds_async([0, 1], [good, host]), lambda: T.step_clouds([0, 1], [good, host]),
                 lambda: api.check_device_clouds([host]), lambda: api.selftest_ingest_clouds([host])):
        with pytest.raises(ValueError, match="__cuda_array_interface__"):
            call()
    with pytest.raises(ValueError, match="one slot per cloud"):
        B.advance_clouds([0], [good, good])
    with pytest.raises(ValueError, match="one stream per cloud"):
        T.step_clouds_async([0, 1, 2], [good, good])
    with pytest.raises(ValueError, match="one entry per pair"):
        B.set_pairs_clouds([good, good], [0, 0], [1])
    with pytest.raises(ValueError, match="no clouds"):
        B.set_pairs_clouds([], [], [])
