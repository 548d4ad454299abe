"""The host side of device-resident frames (cvo_device_image): the ABI names, the descriptor the python wrapper makes from the shape and
strides of a __cuda_array_interface__ carrier, what it refuses before any library call, and replay's grouping on objects that only have
a shape.  No GPU: the carriers are fakes."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvo_check_device_images", "cvo_selftest_ingest_images", "cvo_batch_set_pairs_device_images", "cvo_batch_advance_device_images",
       "cvo_batch_stage_device_images", "cvo_tracks_step_device_async", "cvo_tracks_stage_device_async"]


class Fake:
    """what a device tensor shows of itself: __cuda_array_interface__ (version 2: strides None when C-contiguous) and .shape"""
    def __init__(self, shape, typestr, ptr, strides=None):
        self.shape = tuple(shape)
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(ptr, False), strides=strides, version=2)


def test_header_and_python_mirror_name_the_new_symbols():
    from cvo_slam_amd import api
    src = open(os.path.join(ROOT, "include", "cvo_hip.h")).read()
    assert "typedef struct cvo_device_image" in src
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in api.ABI_SYMBOLS, name
    fields = [f for f, _ in api.DeviceImage._fields_]
    assert fields == ["bgr8", "depth16", "bgr_pitch", "depth_pitch", "pixel_bytes", "swap_rb"]
    import ctypes as C
    assert C.sizeof(api.DeviceImage) == 40


def fields(d):
    return (d.bgr8, d.depth16, d.bgr_pitch, d.depth_pitch, d.pixel_bytes, d.swap_rb)


def test_descriptor_from_shape_and_strides():
    from cvo_slam_amd.api import device_image
    h, w = 48, 70
    # tight
    d, gw, gh = device_image(Fake((h, w, 3), "|u1", 0x1000), Fake((h, w), "<u2", 0x9000))
    assert (gw, gh) == (w, h) and fields(d) == (0x1000, 0x9000, 3 * w, 2 * w, 3, 0)
    # row-pitched (a crop of a wider image), swap_rb
    d, _, _ = device_image(Fake((h, w, 3), "|u1", 0x1003, (3 * w + 21, 3, 1)), Fake((h, w), "<u2", 0x9002, (2 * w + 6, 2)), swap_rb=True)
    assert fields(d) == (0x1003, 0x9002, 3 * w + 21, 2 * w + 6, 3, 1)
    # the first three channels of a BGRA tensor, contiguous and as a crop
    d, _, _ = device_image(Fake((h, w, 3), "|u1", 0x2000, (4 * w, 4, 1)), Fake((h, w), "<u2", 0x9000))
    assert fields(d) == (0x2000, 0x9000, 4 * w, 2 * w, 4, 0)
    d, _, _ = device_image(Fake((h, w, 4), "|u1", 0x2000), Fake((h, w), "<u2", 0x9000))
    assert fields(d) == (0x2000, 0x9000, 4 * w, 2 * w, 4, 0)
    d, _, _ = device_image(Fake((h, w, 3), "|u1", 0x2010, (4 * (w + 9), 4, 1)), Fake((h, w), "<u2", 0x9000))
    assert fields(d)[2:5] == (4 * (w + 9), 2 * w, 4)
    # int16 depth is the same bits
    d, _, _ = device_image(Fake((h, w, 3), "|u1", 0x1000), Fake((h, w), "<i2", 0x9000))
    assert fields(d) == (0x1000, 0x9000, 3 * w, 2 * w, 3, 0)


@pytest.mark.parametrize("bgr,depth", [
    (Fake((48, 70, 3), "<f4", 1), Fake((48, 70), "<u2", 2)),                        # colour not uint8
    (Fake((48, 70, 3), "|u1", 1), Fake((48, 70), "<f4", 2)),                        # float depth
    (Fake((48, 70, 3), "|u1", 1), Fake((48, 70), ">u2", 2)),                        # big-endian depth
    (Fake((48, 70), "|u1", 1), Fake((48, 70), "<u2", 2)),                           # grey image
    (Fake((48, 70, 2), "|u1", 1), Fake((48, 70), "<u2", 2)),                        # two channels
    (Fake((48, 70, 3), "|u1", 1, (210, 1, 70 * 48)), Fake((48, 70), "<u2", 2)),     # planar colour: channel stride not 1
    (Fake((48, 70, 3), "|u1", 1, (8 * 70, 8, 1)), Fake((48, 70), "<u2", 2)),        # every second pixel
    (Fake((48, 70, 4), "|u1", 1, (3 * 70, 3, 1)), Fake((48, 70), "<u2", 2)),        # four channels three bytes apart
    (Fake((48, 70, 3), "|u1", 1, (3 * 70 - 1, 3, 1)), Fake((48, 70), "<u2", 2)),    # rows overlap
    (Fake((48, 70, 3), "|u1", 1, (-210, 3, 1)), Fake((48, 70), "<u2", 2)),          # flipped
    (Fake((48, 70, 3), "|u1", 1), Fake((48, 71), "<u2", 2)),                        # sizes differ
    (Fake((48, 70, 3), "|u1", 1), Fake((48, 70), "<u2", 2, (280, 4))),              # every second depth column
    (Fake((48, 70, 3), "|u1", 1), Fake((48, 70), "<u2", 2, (138, 2))),              # depth rows overlap
    (Fake((48, 70, 3), "|u1", 0), Fake((48, 70), "<u2", 2)),                        # null
    (Fake((48, 70, 3), "|u1", 1), np.zeros((48, 70), np.uint16)),                   # a host depth image
])
def test_what_the_wrapper_refuses(bgr, depth):
    from cvo_slam_amd.api import device_image
    with pytest.raises(ValueError):
        device_image(bgr, depth)


def test_host_and_device_images_do_not_mix():
    from cvo_slam_amd import api
    dev = (Fake((64, 64, 3), "|u1", 1), Fake((64, 64), "<u2", 2))
    host = (np.zeros((64, 64, 3), np.uint8), np.zeros((64, 64), np.uint16))
    assert api._images_on_device([dev, dev]) is True and api._images_on_device([host, host]) is False
    for mixed in ([dev, host], [host, dev], [(dev[0], host[1])]):
        with pytest.raises(ValueError):
            api._images_on_device(mixed)
    # every image method dispatches on that before it touches the library: no handle is needed to see the refusal
    B = api.CvoBatch.__new__(api.CvoBatch); T = api.CvoTracks.__new__(api.CvoTracks)
    cam = (5000.0, 500.0, 500.0, 32.0, 32.0)
    for call in (lambda: B.advance_images([0, 1], [dev, host], cam), lambda: B.stage_images([0, 1], [dev, host], cam),
                 lambda: B.set_pairs_images([dev, host], [0], [1], cam), lambda: T.step_async([0, 1], [dev, host], cam),
                 lambda: T.stage_async([0, 1], [dev, host], cam), lambda: T.step([0, 1], [dev, host], cam)):
        with pytest.raises(ValueError, match="mixed"):
            call()
    with pytest.raises(ValueError, match="swap_rb"):
        api._device_images([dev, dev], [True])


def test_group_by_size_needs_only_a_shape():
    from cvo_slam_amd.replay import frame_size, group_by_size

    class OnlyShape:
        def __init__(self, *shape): self.shape = shape
        def __array__(self, *a, **k): raise AssertionError("a device frame must not be converted")
    a, b, c = OnlyShape(480, 640), OnlyShape(456, 736), OnlyShape(480, 640)
    assert group_by_size([a, b, c]) == [[a, c], [b]]
    frames = {0: (OnlyShape(480, 640, 3), a), 1: (OnlyShape(456, 736, 3), b), 2: (OnlyShape(480, 640, 3), c)}
    assert frame_size(frames[1]) == (456, 736)
    assert group_by_size([0, 1, 2], lambda k: frame_size(frames[k])) == [[0, 2], [1]]
    assert frame_size((np.zeros((4, 5, 3), np.uint8), np.zeros((4, 5), np.uint16))) == (4, 5)
